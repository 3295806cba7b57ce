// gpis_sdf.hpp — ProceduralMean over the reference's SDF shapes (GPF.hpp:1049-1087, GPF.cpp:279-296; math/SdfFunctions.cpp:67-189),
// restated in the reference's arithmetic: fp32 where it computes in float, double exactly where it promotes (the smooth union /
// subtraction, `p *= 1. / scale`, `PI / 3.`), Vec::dot / lengthSq summed left to right, lerp as a*(1-t) + b*t, min / max as the
// comparisons of MathUtil.hpp:14-29, length() through the correctly rounded sqrtf, no contraction.  The three Mat4f::rotAxis
// matrices (Mat4f.cpp:132-148: sin / cos of a float from the host libm) and the inverse of the mean's "transform" come from the host
// in DevModel; nothing here evaluates a sine or a cosine.
//
// Included by gpis_device.hpp in front of the path section.  Only the all-features path instance reaches it (GPIS_FLAG_sdf_mean);
// the bodies are out of line so that instance's register budget does not carry them.  The two out-of-line functions also serve
// TabulatedMean (gpis_grid_mean.hpp): DevModel::sdf_mean says "a slot in use needs the out-of-line mean".
#pragma once

#pragma clang fp contract(off)

namespace gpis {
namespace sdf {

#define GPIS_SDF_FN static __device__ __attribute__((noinline))

GPIS_DEV float fmin_ref(float a, float b) { return a < b ? a : b; }      // MathUtil.hpp:14-17
GPIS_DEV float fmax_ref(float a, float b) { return a > b ? a : b; }      // MathUtil.hpp:26-29
GPIS_DEV float len2(float x, float y) { float r = 0.f; r += x * x; r += y * y; return sqrtf(r); }
GPIS_DEV float len3(V3 a) { float r = 0.f; r += a.x * a.x; r += a.y * a.y; r += a.z * a.z; return sqrtf(r); }
GPIS_DEV V3 rot(const float *m, V3 b)                                    // Mat4f::transformVector, Mat4f.hpp:159-166
{
    return V3{m[0] * b.x + m[1] * b.y + m[2] * b.z, m[3] * b.x + m[4] * b.y + m[5] * b.z, m[6] * b.x + m[7] * b.y + m[8] * b.z};
}

GPIS_DEV float sd_sphere(V3 v, float r) { return len3(v) - r; }
GPIS_DEV float sd_torus(V3 p, float tx, float ty) { return len2(len2(p.x, p.z) - tx, p.y) - ty; }
GPIS_DEV float sd_cone(V3 p, float cx, float cy) { const float q = len2(p.x, p.y); return cx * q + cy * p.z; }
GPIS_DEV float sd_capped_cylinder(V3 p, float h, float r)
{
    const float dx = fabsf(len2(p.x, p.z)) - h, dy = fabsf(p.y) - r;
    const float mx = 0.0f > dx ? 0.0f : dx, my = 0.0f > dy ? 0.0f : dy;          // max(d, Vec2f(0)), MathUtil.hpp:48-56
    return fmin_ref(fmax_ref(dx, dy), 0.0f) + len2(mx, my);
}
GPIS_DEV float sd_tri_prism(V3 p, float hx, float hy)
{
    const float qx = fabsf(p.x), qz = fabsf(p.z);
    return fmax_ref(qz - hy, fmax_ref(qx * 0.866025f + p.y * 0.5f, -p.y) - hx * 0.5f);
}
GPIS_DEV float lerp_f(float a, float b, float t) { return a * (1.0f - t) + b * t; }   // MathUtil.hpp:91-94
GPIS_DEV float op_smooth_union(float d1, float d2, float k)
{
    const float h = fmin_ref(fmax_ref(0.5f + 0.5f * (d2 - d1) / k, 0.0f), 1.0f);
    return (float)((double)lerp_f(d2, d1, h) - (double)(k * h) * (1.0 - (double)h));
}
GPIS_DEV float ssub(float d1, float d2, float k)
{
    double hd = 0.5 - 0.5 * (double)(d2 + d1) / (double)k;
    hd = hd > 0.0 ? hd : 0.0;
    hd = hd < 1.0 ? hd : 1.0;
    const float h = (float)hd;
    return (float)((double)lerp_f(d2, -d1, h) + (double)(k * h) * (1.0 - (double)h));
}

constexpr float kPi = 3.1415926536f;                     // Angle.hpp:8
constexpr float kConeA = (float)((double)kPi / 3.);      // Vec2f(PI / 3., PI / 3.): the double quotient narrowed
constexpr float kConeB = kPi / 3.f;
constexpr float kK002 = (float)0.02, kK01 = (float)0.1, kR07 = (float)0.7;

GPIS_DEV float sd_base(const DevModel &M, V3 p)
{
    const float *Rm90 = M.sdf_rot[0], *Rp90 = M.sdf_rot[1];
    float base = op_smooth_union(sd_cone(rot(Rm90, V3{p.x + 0.f, p.y + .9f, p.z + 0.f}), kConeA, kConeA),
                                 sd_cone(rot(Rp90, V3{p.x - 0.f, p.y - .9f, p.z - 0.f}), kConeB, kConeB), kK002);
    base = fmax_ref(base, sd_capped_cylinder(p, 1.1f, 0.25f)) * 0.7f;
    base = fmax_ref(-sd_capped_cylinder(p, 0.6f, 0.3f), base);
    base = fmax_ref(-sd_tri_prism(rot(Rp90, V3{p.x + 0.f, p.y + 0.f, p.z + -1.f}), 1.2f, 0.3f), base);
    return base;
}
// sdKnob (outer = false) and sdKnobOuter (outer = true) differ in one line
GPIS_DEV float sd_knob(const DevModel &M, V3 p, bool outer)
{
    const float sphere = sd_sphere(p, 1.0f);
    const float cutout = sd_sphere(V3{p.x - 0.0f, p.y - 0.5f, p.z - 0.5f}, kR07);
    const float etch = sd_torus(rot(M.sdf_rot[2], V3{p.x - 0.0f, p.y - 0.2f, p.z - 0.2f}), 1.0f, 0.05f);
    const float inner = sd_sphere(V3{p.x - 0.0f, p.y - 0.0f, p.z - 0.0f}, 0.75f);
    float d = ssub(cutout, sphere, kK01);
    d = outer ? fmax_ref(d, -inner) : fmin_ref(d, inner);
    d = fmax_ref(-etch, d);
    d = fmin_ref(ssub(sphere, sd_base(M, V3{p.x - 0.f, p.y - -.775f, p.z - 0.f}), kK01), d);
    return d;
}

// SdfFunctions::eval (SdfFunctions.hpp:47-55)
GPIS_DEV float eval(const DevModel &M, int func, V3 p)
{
    constexpr float scale = (float)0.8;
    constexpr float inv = (float)(1. / (double)scale);          // `p *= 1. / scale` on a Vec3f: the double narrowed to the element type
    if (func == GPIS_SDF_PLANE)
        return p.y;
    if (func == GPIS_SDF_TWO_SPHERES)
        return fmin_ref(len3(V3{p.x - 0.f, p.y - 10.f, p.z - 0.f}) - 9.5f, len3(V3{p.x - 0.f, p.y - -10.f, p.z - 0.f}) - 9.5f);
    const V3 q{p.x * inv, p.y * inv, p.z * inv};
    if (func == GPIS_SDF_KNOB_INNER)
        return sd_sphere(V3{q.x - 0.0f, q.y - 0.0f, q.z - 0.0f}, 0.75f) * scale;
    return sd_knob(M, q, func == GPIS_SDF_KNOB_OUTER) * scale;
}

// _invConfigTransform.transformPoint(vec_conv<Vec3f>(a)), Mat4f.hpp:168-175
GPIS_DEV V3 to_local(const DevModel &M, int w, V3d a)
{
    const float *T = M.sdf_inv[w];
    const V3 b{(float)a.x, (float)a.y, (float)a.z};
    return V3{T[0] * b.x + T[1] * b.y + T[2] * b.z + T[3], T[4] * b.x + T[5] * b.y + T[6] * b.z + T[7], T[8] * b.x + T[9] * b.y + T[10] * b.z + T[11]};
}
// ProceduralMean::mean, GPF.cpp:279-285
GPIS_DEV double procedural_mean(const DevModel &M, int w, V3d a)
{
    const gpis_mean &mu = M.mean[w];
    float m = eval(M, mu.func, to_local(M, w, a));
    m *= mu.scale;
    const float v = m + mu.offset;
    return (double)(mu.min > v ? mu.min : v);
}
GPIS_DEV double slot_mean(const DevModel &M, int w, V3d a)
{
    if (M.mean[w].type == GPIS_MEAN_TABULATED)
        return tabulated_mean(M, w, a);
    return M.mean[w].type == GPIS_MEAN_PROCEDURAL ? procedural_mean(M, w, a) : mean_eval(M, w, a);
}

// GaussianProcess::mean_weight_space (GaussianProcess.cpp:379-393) of a medium with a procedural or tabulated mean in either slot
struct MeanId { double mean; int id; };
GPIS_SDF_FN MeanId mean_weight_space(const DevModel *Mp, double ax, double ay, double az)
{
    const DevModel &M = *Mp;
    const V3d a{ax, ay, az};
    double m = slot_mean(M, 0, a);
    int i = 0;
    if (M.has_mean_additional) {
        const double add = slot_mean(M, 1, a);
        if (add < m) { m = add; i = 1; }
    }
    return MeanId{m, i};
}
// dmean_da of slot w: ProceduralMean's one-sided difference (GPF.cpp:287-296; the order a, +x, +y, +z), TabulatedMean's
// (GPF.cpp:179-190: a double eps, the order +x, +y, +z, a) or the analytic gradient
GPIS_SDF_FN V3d mean_grad(const DevModel *Mp, int w, double ax, double ay, double az)
{
    const DevModel &M = *Mp;
    const V3d a{ax, ay, az};
    if (M.mean[w].type == GPIS_MEAN_TABULATED)
        return tabulated_mean_grad(M, w, a);
    if (M.mean[w].type != GPIS_MEAN_PROCEDURAL) {
        return gpis::mean_grad(M, w, a);
    }
    const double eps = 0.001f;
    double v0 = 0., v1 = 0., v2 = 0., v3 = 0.;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {     // one body, four trips: the shape's code is emitted once
        V3d q = a;                    // mean(a), then mean(a + Vec3d(eps, 0.f, 0.f)), ...
        if (k) { q.x = ax + (k == 1 ? eps : 0.); q.y = ay + (k == 2 ? eps : 0.); q.z = az + (k == 3 ? eps : 0.); }
        const double v = procedural_mean(M, w, q);
        v0 = k == 0 ? v : v0; v1 = k == 1 ? v : v1; v2 = k == 2 ? v : v2; v3 = k == 3 ? v : v3;
    }
    return V3d{(v1 - v0) / eps, (v2 - v0) / eps, (v3 - v0) / eps};
}
// the point MeanFunction::color is evaluated at (GPF.hpp:1065-1073): T^-1 . Vec3f(a), widened, when the primary mean is procedural
GPIS_DEV V3d color_point(const DevModel &M, V3d a)
{
    if (M.mean[0].type != GPIS_MEAN_PROCEDURAL)
        return a;
    return to_d(to_local(M, 0, a));
}

#undef GPIS_SDF_FN

}   // namespace sdf
}   // namespace gpis
