/* TEST INFRASTRUCTURE: plain-C restatement of the reference's ProceduralMean over its SDF shapes — the tests' reference for the
 * mean, written independently of csrc/gpis_sdf.hpp.  Sources: math/SdfFunctions.cpp:67-189 (the shapes), math/SdfFunctions.hpp:47-55
 * (eval), math/GPFunctions.cpp:279-296 (ProceduralMean::mean / dmean_da), math/Mat4f.hpp:75-101, 159-175 (invert, transformVector,
 * transformPoint), math/Mat4f.cpp:132-148 (rotAxis), math/MathUtil.hpp:14-29, 73-76, 91-94 (min, max, clamp, lerp),
 * math/Vec.hpp:134-145, 200-206 (lengthSq, length, dot), GaussianProcess.cpp:379-393 (the CSG minimum of two means).
 * Built with -msse4.2 -mno-fma -ffp-contract=off (tests/sdf_mean_ref.py): every float operation rounds once, as in the reference's
 * SSE4.2 build.  Each min / max / clamp of sdKnob, sdKnobOuter and sdBase records which outcome it took in a bit mask (sdf_ref_trace):
 * the pin generator asserts that the pin points reach every outcome. */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float x, y, z; } v3;

static const float PI_F = 3.1415926536f;

/* ---- outcome trace: two bits per two-way choice (bit 2k: first outcome, bit 2k+1: second), three per clamp ---- */
static uint64_t g_trace;
enum {
    T_UNION_CLAMP = 0,      /* opSmoothUnion's clamp: low, interior, high                       bits 0..2   */
    T_SSUB1_CLAMP = 3,      /* ssub(cutout, sphere): low, interior, high                         bits 3..5   */
    T_SSUB2_CLAMP = 6,      /* ssub(sphere, base): low, interior, high                           bits 6..8   */
    T_BASE_MAX_CYL = 9,     /* max(base, cylinder): base, cylinder                               bits 9..10  */
    T_BASE_MAX_DIG = 11,    /* max(-cylinder, base)                                              bits 11..12 */
    T_BASE_MAX_PIE = 13,    /* max(-prism, base)                                                 bits 13..14 */
    T_KNOB_EYE = 15,        /* min(d, inner) / max(d, -inner): first, second                     bits 15..16 */
    T_KNOB_ETCH = 17,       /* max(-etch, d)                                                     bits 17..18 */
    T_KNOB_BASE = 19,       /* min(ssub(sphere, base), d)                                        bits 19..20 */
    T_CYL_MIN = 21,         /* sdCappedCylinder: min(max(dx, dy), 0): inside, outside            bits 21..22 */
    T_CYL_MAX = 23,         /* sdCappedCylinder: max(dx, dy): dx, dy                             bits 23..24 */
    T_PRISM_OUTER = 25,     /* sdTriPrism: outer max: first, second                              bits 25..26 */
    T_PRISM_INNER = 27,     /* sdTriPrism: inner max: first, second                              bits 27..28 */
    T_BITS = 29
};
static void tr(int base, int which) { g_trace |= (uint64_t)1 << (base + which); }

static float minf_t(float a, float b, int t) { if (a < b) { tr(t, 0); return a; } tr(t, 1); return b; }
static float maxf_t(float a, float b, int t) { if (a > b) { tr(t, 0); return a; } tr(t, 1); return b; }
static float minf_(float a, float b) { return a < b ? a : b; }
static float maxf_(float a, float b) { return a > b ? a : b; }

static float length2(float a, float b)
{
    float r = 0.0f;
    r += a * a;
    r += b * b;
    return sqrtf(r);
}
static float length3(v3 a)
{
    float r = 0.0f;
    r += a.x * a.x;
    r += a.y * a.y;
    r += a.z * a.z;
    return sqrtf(r);
}
static v3 add3(v3 a, float x, float y, float z) { v3 r = {a.x + x, a.y + y, a.z + z}; return r; }
static v3 sub3(v3 a, float x, float y, float z) { v3 r = {a.x - x, a.y - y, a.z - z}; return r; }

/* Mat4f::rotAxis, upper-left 3x3 */
static void rot_axis(float ax, float ay, float az, float degrees, float *m)
{
    float angle = degrees * (PI_F / 180.0f);
    float s = sinf(angle);
    float c = cosf(angle);
    float c1 = 1.0f - c;
    float x = ax, y = ay, z = az;
    m[0] = c + x * x * c1; m[1] = x * y * c1 - z * s; m[2] = x * z * c1 + y * s;
    m[3] = y * x * c1 + z * s; m[4] = c + y * y * c1; m[5] = y * z * c1 - x * s;
    m[6] = z * x * c1 - y * s; m[7] = z * y * c1 + x * s; m[8] = c + z * z * c1;
}
void sdf_ref_rot_axis_x(float degrees, float *out9) { rot_axis(1.f, 0.f, 0.f, degrees, out9); }
static v3 transform_vector(const float *m, v3 b)
{
    v3 r;
    r.x = m[0] * b.x + m[1] * b.y + m[2] * b.z;
    r.y = m[3] * b.x + m[4] * b.y + m[5] * b.z;
    r.z = m[6] * b.x + m[7] * b.y + m[8] * b.z;
    return r;
}

static float sd_sphere(v3 v, float r) { return length3(v) - r; }
static float sd_torus(v3 p, float tx, float ty)
{
    float qx = length2(p.x, p.z) - tx, qy = p.y;
    return length2(qx, qy) - ty;
}
static float sd_cone(v3 p, float cx, float cy)
{
    float q = length2(p.x, p.y);
    return cx * q + cy * p.z;
}
static float sd_capped_cylinder(v3 p, float h, float r)
{
    float dx = fabsf(length2(p.x, p.z)) - h;
    float dy = fabsf(p.y) - r;
    float mx = dx, my = dy;              /* max(d, Vec2f(0)): replaces a component when 0 > it */
    if (0.0f > dx) mx = 0.0f;
    if (0.0f > dy) my = 0.0f;
    return minf_t(maxf_t(dx, dy, T_CYL_MAX), 0.0f, T_CYL_MIN) + length2(mx, my);
}
static float sd_tri_prism(v3 p, float hx, float hy)
{
    float qx = fabsf(p.x), qz = fabsf(p.z);
    return maxf_t(qz - hy, maxf_t(qx * 0.866025f + p.y * 0.5f, -p.y, T_PRISM_INNER) - hx * 0.5f, T_PRISM_OUTER);
}
static float lerpf_(float a, float b, float t) { return a * (1.0f - t) + b * t; }
static float op_smooth_union(float d1, float d2, float k)
{
    float v = 0.5f + 0.5f * (d2 - d1) / k;
    float h = minf_(maxf_(v, 0.0f), 1.0f);
    tr(T_UNION_CLAMP, v > 0.0f ? (v < 1.0f ? 1 : 2) : 0);
    return lerpf_(d2, d1, h) - k * h * (1.0 - h);
}
static float ssub(float d1, float d2, float k, int t)
{
    double v = 0.5 - 0.5 * (d2 + d1) / k;
    double c = v > 0.0 ? v : 0.0;
    c = c < 1.0 ? c : 1.0;
    float h = c;
    tr(t, v > 0.0 ? (v < 1.0 ? 1 : 2) : 0);
    return lerpf_(d2, -d1, h) + k * h * (1.0 - h);
}

static float sd_base(v3 p)
{
    float rm90[9], rp90[9];
    rot_axis(1.f, 0.f, 0.f, -90, rm90);
    rot_axis(1.f, 0.f, 0.f, 90, rp90);
    float ca = PI_F / 3.;                   /* Vec2f(PI / 3., PI / 3.): double quotient, narrowed */
    float cb = PI_F / 3.f;
    float base = op_smooth_union(sd_cone(transform_vector(rm90, add3(p, 0.f, .9f, 0.f)), ca, ca),
                                 sd_cone(transform_vector(rp90, sub3(p, 0.f, .9f, 0.f)), cb, cb), 0.02);
    base = maxf_t(base, sd_capped_cylinder(p, 1.1f, 0.25f), T_BASE_MAX_CYL) * 0.7f;
    base = maxf_t(-sd_capped_cylinder(p, 0.6f, 0.3f), base, T_BASE_MAX_DIG);
    base = maxf_t(-sd_tri_prism(transform_vector(rp90, add3(p, 0.f, 0.f, -1.f)), 1.2f, 0.3f), base, T_BASE_MAX_PIE);
    return base;
}
static float sd_knob_any(v3 p, int outer)
{
    float rm45[9];
    rot_axis(1.f, 0.f, 0.f, -45, rm45);
    float sphere = sd_sphere(p, 1.0);
    float cutout = sd_sphere(sub3(p, 0.0f, 0.5f, 0.5f), 0.7);
    float cutout_etch = sd_torus(transform_vector(rm45, sub3(p, 0.0f, 0.2f, 0.2f)), 1.0f, 0.05f);
    float innersphere = sd_sphere(sub3(p, 0.0f, 0.0f, 0.0f), 0.75);
    float d = ssub(cutout, sphere, 0.1, T_SSUB1_CLAMP);
    if (outer)
        d = maxf_t(d, -innersphere, T_KNOB_EYE);
    else
        d = minf_t(d, innersphere, T_KNOB_EYE);
    d = maxf_t(-cutout_etch, d, T_KNOB_ETCH);
    d = minf_t(ssub(sphere, sd_base(sub3(p, 0.f, -.775f, 0.f)), 0.1, T_SSUB2_CLAMP), d, T_KNOB_BASE);
    return d;
}

/* SdfFunctions::eval; func in the order of SdfFunctions::Function */
static float sdf_eval(int func, v3 p)
{
    const float scale = 0.8;
    if (func == 4)
        return p.y;
    if (func == 3)
        return minf_(length3(sub3(p, 0., 10., 0.f)) - 9.5f, length3(sub3(p, 0.f, -10.f, 0.f)) - 9.5f);
    float inv = 1. / scale;                 /* Vec3f *= double: the factor is narrowed to the element type first */
    p.x *= inv; p.y *= inv; p.z *= inv;
    if (func == 1)
        return sd_sphere(sub3(p, 0.0f, 0.0f, 0.0f), 0.75) * scale;
    return sd_knob_any(p, func == 2) * scale;
}

/* ---- Mat4f ---- */
/* Mat4f::invert (Mat4f.hpp:75-101): the adjugate over the determinant, in float.  inv[4 i + j] is the cofactor of (row j, column i):
 * with r0 < r1 < r2 the rows other than j and c0 < c1 < c2 the columns other than i, six triple products (a*b)*c summed left to
 * right in the order and with the signs below (all flipped when i + j is odd) — the order the reference's expanded lines have.
 * det = a[0] inv[0] + a[1] inv[4] + a[2] inv[8] + a[3] inv[12]; det == 0 gives the identity. */
void sdf_ref_mat4_invert(const float *a, float *out)
{
    static const int pick[6][3] = {{0, 1, 2}, {0, 1, 2}, {1, 0, 2}, {1, 0, 2}, {2, 0, 1}, {2, 0, 1}};     /* rows of the three factors */
    static const int cols[6][3] = {{0, 1, 2}, {0, 2, 1}, {0, 1, 2}, {0, 2, 1}, {0, 1, 2}, {0, 2, 1}};     /* their columns */
    static const int minus[6] = {0, 1, 1, 0, 0, 1};
    float inv[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            int r[3], c[3];
            for (int k = 0, nr = 0, nc = 0; k < 4; ++k) {
                if (k != j) r[nr++] = k;
                if (k != i) c[nc++] = k;
            }
            const int flip = (i + j) & 1;
            float acc = 0.0f;
            for (int t = 0; t < 6; ++t) {
                const float term = a[4 * r[pick[t][0]] + c[cols[t][0]]] * a[4 * r[pick[t][1]] + c[cols[t][1]]] * a[4 * r[pick[t][2]] + c[cols[t][2]]];
                const int neg = minus[t] ^ flip;
                if (t == 0) acc = neg ? -term : term;
                else acc = neg ? acc - term : acc + term;
            }
            inv[4 * i + j] = acc;
        }
    const float det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (det == 0.0f) {
        for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        return;
    }
    const float invDet = 1.0f / det;
    for (int i = 0; i < 16; ++i) out[i] = inv[i] * invDet;
}
static v3 transform_point(const float *m, v3 b)
{
    v3 r;
    r.x = m[0] * b.x + m[1] * b.y + m[2] * b.z + m[3];
    r.y = m[4] * b.x + m[5] * b.y + m[6] * b.z + m[7];
    r.z = m[8] * b.x + m[9] * b.y + m[10] * b.z + m[11];
    return r;
}
void sdf_ref_transform_point(const float *m16, size_t n, const float *p3, float *out3)
{
    for (size_t i = 0; i < n; ++i) {
        v3 b = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
        v3 r = transform_point(m16, b);
        out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
    }
}

/* ---- the four exported functions (plus plane), on float triples ---- */
void sdf_ref_eval(int func, size_t n, const float *p3, float *out)
{
    for (size_t i = 0; i < n; ++i) {
        v3 p = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
        out[i] = sdf_eval(func, p);
    }
}
/* as sdf_ref_eval, returning the union of the outcome bits the points took (T_* above) */
uint64_t sdf_ref_trace(int func, size_t n, const float *p3)
{
    g_trace = 0;
    for (size_t i = 0; i < n; ++i) {
        v3 p = {p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
        (void)sdf_eval(func, p);
    }
    return g_trace;
}
int sdf_ref_trace_bits(void) { return T_BITS; }

/* ---- one mean slot: type 0..3 as gpis_mean_type; the analytic ones as GPF.hpp:867-1005 ---- */
typedef struct {
    int32_t type, func;
    float radius, offset, scale, min;
    double center[3], dir[3];         /* dir: normalised by the caller */
    float inv_transform[16];          /* procedural: _invConfigTransform */
} sdf_ref_slot;

static double procedural_mean(const sdf_ref_slot *s, double ax, double ay, double az)
{
    v3 p = {(float)ax, (float)ay, (float)az};
    p = transform_point(s->inv_transform, p);
    float m = sdf_eval(s->func, p);
    m *= s->scale;
    return maxf_(s->min, m + s->offset);
}
static double slot_mean(const sdf_ref_slot *s, const double *a)
{
    if (s->type == 3)
        return procedural_mean(s, a[0], a[1], a[2]);
    if (s->type == 0)
        return (double)s->offset;
    double dx = a[0] - s->center[0], dy = a[1] - s->center[1], dz = a[2] - s->center[2];
    if (s->type == 1) {
        double l = 0.;
        l += dx * dx; l += dy * dy; l += dz * dz;
        return sqrt(l) - (double)s->radius;
    }
    double dt = dx * s->dir[0];
    dt += dy * s->dir[1];
    dt += dz * s->dir[2];
    double v = dt * (double)s->scale, mn = (double)s->min;
    return v > mn ? v : mn;
}
static void slot_grad(const sdf_ref_slot *s, const double *a, double *g)
{
    if (s->type == 3) {
        double eps = 0.001f;
        double vals[4];
        vals[0] = procedural_mean(s, a[0], a[1], a[2]);
        vals[1] = procedural_mean(s, a[0] + eps, a[1] + 0.f, a[2] + 0.f);
        vals[2] = procedural_mean(s, a[0] + 0.f, a[1] + eps, a[2] + 0.f);
        vals[3] = procedural_mean(s, a[0] + 0.f, a[1] + 0.f, a[2] + eps);
        g[0] = (vals[1] - vals[0]) / eps;
        g[1] = (vals[2] - vals[0]) / eps;
        g[2] = (vals[3] - vals[0]) / eps;
        return;
    }
    g[0] = g[1] = g[2] = 0.;
    if (s->type == 0)
        return;
    double dx = a[0] - s->center[0], dy = a[1] - s->center[1], dz = a[2] - s->center[2];
    if (s->type == 1) {
        double l = 0.;
        l += dx * dx; l += dy * dy; l += dz * dz;
        double inv = 1.0 / sqrt(l);
        g[0] = dx * inv; g[1] = dy * inv; g[2] = dz * inv;
        return;
    }
    double dt = dx * s->dir[0];
    dt += dy * s->dir[1];
    dt += dz * s->dir[2];
    if (dt * (double)s->scale < (double)s->min)
        return;
    for (int k = 0; k < 3; ++k) g[k] = s->dir[k] * (double)s->scale;
}
/* GaussianProcess::mean_weight_space over n points: value, chosen slot, dmean_da of that slot; slots[1] may be null */
void sdf_ref_mean(const sdf_ref_slot *s0, const sdf_ref_slot *s1, size_t n, const double *p3, double *value, int32_t *id, double *grad3)
{
    for (size_t i = 0; i < n; ++i) {
        const double *a = p3 + 3 * i;
        double m = slot_mean(s0, a);
        int w = 0;
        if (s1) {
            double add = slot_mean(s1, a);
            if (add < m) { m = add; w = 1; }
        }
        value[i] = m;
        id[i] = w;
        slot_grad(w ? s1 : s0, a, grad3 + 3 * i);
    }
}
size_t sdf_ref_slot_size(void) { return sizeof(sdf_ref_slot); }
