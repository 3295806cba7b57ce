// gpis_ws.hpp — the weight-space GP medium (random Fourier features): one wave per segment.
//
//   WeightSpaceGaussianProcessMedium::{intersectGP, sampleGradient}   media/WeightSpaceGaussianProcessMedium.cpp:64-291 (WSM)
//   WeightSpaceRealization::{evaluate, evaluateGradient}, WeightSpaceBasis::{evaluate, evaluateGradient, sample},
//   WeightSpaceRealization::sample                                     math/WeightSpaceGaussianProcess.cpp:26-76, 120-240 (WSG)
//   SquaredExponentialCovariance::sample_spectral_density_3d           math/GPFunctions.hpp:1812-1815
//   sample_standard_normal                                             sampling/Gaussian.cpp:104-119
//
// A realization is N basis functions (d_i, omega_i, phi_i) and N weights w_i.  Basis function i uses draws 5i .. 5i+4 of the
// basis stream (phi, then two Box–Muller pairs of which the fourth normal is discarded), weight i uses draws 2(i/2), 2(i/2)+1 of
// the weight stream: lane j builds functions j, j+64, ... by PCG jump-ahead, in any order, with the values the serial loop makes.
//
// The field is a sum over the basis in basis order (WSG:123-124).  Tree reductions would reorder it, so a wave evaluates up to
// kWsK points at once: in each round of 64 basis functions lane j computes function j's term for every point and stages it in
// LDS, then lane k adds point k's 64 terms in basis order — the reference's association, no reordering.  The points of a march
// are known ahead of their values (t_{k+1} = t_k + step in double; the refinement candidates lerp(t - step, t, intp 0.9^j)), so
// the march evaluates them speculatively in batches and discards everything after the first point the serial loop stops at.
//
// Eigen evaluation orders of the reference build (vendored Eigen, SSE2 packets of two doubles, no FMA):
//   dirs.row(row).dot(p) (a row of a dynamic MatrixXd by a Vector3d): (c0 + c1) + c2 — Core/Redux.h, the linear (non-vectorised)
//       traversal of a strided block;
//   Matrix3d::determinant: m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20) + m02 (m10 m21 - m11 m20) — LU/Determinant.h
//       (bruteforce_det3_helper);
//   Matrix3d::inverse: cofactors, det = (c00 m00 + c10 m10) + c20 m20, r = cofactor * (1 / det) — LU/InverseImpl.h
//       (compute_inverse_size3_helper; the double twin of eig_inverse3 in gpis_device.hpp, with the packet sum order);
//   Matrix3d * Vector3d: row i = (m(i,0) v0 + m(i,1) v1) + m(i,2) v2 — Core/products/GeneralMatrixVector.h via the lazy product.
#pragma once
#include "gpis_device.hpp"

#pragma clang fp contract(off)

namespace gpis {

constexpr int kWsK = 32;                         // points per evaluation batch
constexpr int kWsStride = kWsK + 1;              // LDS row stride of the term table (odd: conflict-free column writes)
constexpr int kWsMaxRefine = 4096;               // refinement candidates before the collapse is forced (see ws_intersect)
constexpr uint32_t kWsHandleTag = 0x57534D31u;   // first word of a weight-space handle ("WSM1"); a gpis_medium starts with abi_version
constexpr float kWsTwoPiF = 3.1415926536f * 2.0f;   // TWO_PI, math/Angle.hpp:8-10 (float)

// Host-precomputed constants of one weight-space medium (read through scalar loads)
struct WsModel {
    DevModel base;               // means, colour ramp, sigma_s / sigma_t, absorption_only, max_bounces, sigma_raw, k_l, fs_aniso
    int32_t n;                   // basis functions
    int32_t normal_method;       // gpis_normal_method (conditioned_gaussian / finite_differences)
    int32_t single;              // single_realization
    int32_t ctx;                 // gpis_corr_ctx
    uint32_t seed, min_step;
    float step_size;             // _rayMarchStepSize
    float l;                     // lengthScale
    float sqrt_aniso[3];         // std::sqrt(float) of "aniso" (the float overload: Vec.hpp:16 `using std::sqrt`)
    int32_t _pad;
    double sqrt2n;               // sqrt(2. / N) (host libm); unused when N == 0
    const double *basis;         // single realization: the basis of pss (0,0,0,0), structure of arrays [6][N]
};
struct WsCounters { unsigned long long n_eval, n_spec, n_seg, arg_overflow; };

struct WsLds {
    double term[64 * kWsStride];                 // round table: [basis lane j][point k]
    double px[kWsK], py[kWsK], pz[kWsK];         // the batch's points
    double val[kWsK];                            // value points: the field value; gradient points: the raw basis sum
    int32_t kind[kWsK];                          // 0 = value, 1..3 = gradient component x..z
    int32_t id[kWsK];                            // gp id of a value point
    uint32_t ov;                                 // bit k: some term of point k had a cos / sin argument beyond the restated range
};
static_assert(sizeof(WsLds) <= 20 * 1024, "eight one-wave workgroups (two per SIMD) share the LDS of one CU");

struct WsTally { unsigned long long eval, spec; };

// ---- realization ---------------------------------------------------------------------------------------------------------
// PCG32 jump: state after n further draws = A s + C (mod 2^64)
GPIS_DEV void ws_jump(uint64_t n, uint64_t &A, uint64_t &C)
{
    uint64_t a = kPcgMult, c = 1ULL;
    A = 1ULL; C = 0ULL;
    while (n) {
        if (n & 1ULL) { A = A * a; C = C * a + c; }
        c = (a + 1ULL) * c;
        a = a * a;
        n >>= 1;
    }
}
// the pixelSampleSegment a realization is drawn from (WSM:41-47, 164-173)
GPIS_DEV void ws_pss(const WsModel &W, uint32_t px, uint32_t py, uint32_t spp, uint32_t seg, uint32_t pss[4])
{
    if (W.single) { pss[0] = pss[1] = pss[2] = pss[3] = 0u; return; }
    pss[0] = px; pss[1] = py; pss[2] = spp; pss[3] = W.ctx == GPIS_CTX_GLOBAL ? 0u : seg;
}
// streams after the UniformPathSampler constructors (state = seed, then next2D): WSG:161 and WSG:236
GPIS_DEV void ws_streams(const WsModel &W, const uint32_t pss[4], uint64_t &sb, uint64_t &sw)
{
    const uint32_t h = xxhash32_4(pss[0], pss[1], pss[2], pss[3]);
    Pcg32 s;
    s.set_state((uint64_t)h);
    sb = s.state;
    s.set_state((uint64_t)(uint32_t)(W.seed + h));
    sw = s.state;
}
// basis function i and weight i: out = d.x, d.y, d.z, omega, phi, w (WSG:166-198 with d = 3; WSG:238)
GPIS_DEV void ws_gen(const WsModel &W, uint64_t sb, uint64_t sw, int i, double out[6])
{
    uint64_t A, C;
    ws_jump(5ull * (uint64_t)i, A, C);
    Pcg32 s;
    s.state = A * sb + C;
    out[4] = (double)(normalized_uint(s.next_i()) * kWsTwoPiF);     // sampler->next1D() * TWO_PI, in float
    double z0, z1, z2, z3;
    rand_normal_2(s, z0, z1);
    rand_normal_2(s, z2, z3);                                        // sample_standard_normal(3): the odd tail takes .x
    const double il = (double)W.l;
    const double v0 = (z0 / il) * (double)W.sqrt_aniso[0];
    const double v1 = (z1 / il) * (double)W.sqrt_aniso[1];
    const double v2 = (z2 / il) * (double)W.sqrt_aniso[2];
    double l2 = v0 * v0; l2 += v1 * v1; l2 += v2 * v2;               // Vec::lengthSq
    const double len = sqrt(l2);
    const double inv = 1.0 / len;                                    // Vec::normalized
    out[0] = v0 * inv; out[1] = v1 * inv; out[2] = v2 * inv;
    out[3] = len;
    ws_jump(2ull * (uint64_t)(i >> 1), A, C);
    s.state = A * sw + C;
    double wx, wy;
    rand_normal_2(s, wx, wy);
    out[5] = (i & 1) ? wy : wx;
}
// lane's share of one realization into a structure-of-arrays buffer [6][ld]
GPIS_DEV void ws_build(const WsModel &W, const uint32_t pss[4], double *B, int ld, int lane)
{
    uint64_t sb, sw;
    ws_streams(W, pss, sb, sw);
    for (int i = lane; i < W.n; i += 64) {
        double f[6];
        ws_gen(W, sb, sw, i, f);
        for (int c = 0; c < 6; ++c) B[c * ld + i] = f[c];
    }
}

// ---- field ----------------------------------------------------------------------------------------------------------------
// sqrt((*_cov)(None, None, p, p)) — the squared exponential in its GP form, as fs_cov
GPIS_DEV double ws_scale(const WsModel &W, V3d p)
{
    const DevModel &M = W.base;
    const V3d an{(double)M.fs_aniso[0], (double)M.fs_aniso[1], (double)M.fs_aniso[2]};
    const V3d d{p.x - p.x, p.y - p.y, p.z - p.z};
    const V3d ad{an.x * d.x, an.y * d.y, an.z * d.z};
    double absq = d.x * ad.x; absq += d.y * ad.y; absq += d.z * ad.z;
    const float s2 = M.sigma_raw * M.sigma_raw, l2 = M.k_l * M.k_l;
    return sqrt((double)s2 * exp_glibc(-absq / (double)(2 * l2)));
}
GPIS_DEV bool ws_arg_overflow(double x)
{
    const uint32_t k = (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32) & 0x7fffffffu;
    return k >= 0x419921fbu && k < 0x7ff00000u;      // finite and beyond the restated range of cos_glibc / sin_glibc
}
// Evaluates the cnt points staged in L (px/py/pz/kind).  Afterwards L.val[k] is the field value (kind 0, with L.id[k]) or the
// raw sum sum_i ((d_c omega_i) w_i)(-sin(.)) of gradient component c = kind - 1, and L.ov[k] says whether one of the point's
// arguments left the restated range.  Only the points the reference evaluates count (ws_keep): a speculative point the serial
// loop never reaches is discarded with its flag.  Wave-uniform call.
GPIS_DEV void ws_eval_points(const WsModel &W, WsLds &L, const double *__restrict__ B, int cnt, int lane)
{
    const int N = W.n;
    double acc = 0.0;
    for (int r0 = 0; r0 < N; r0 += 64) {
        const int m = N - r0 < 64 ? N - r0 : 64;
        if (lane < m) {
            const int i = r0 + lane;
            const double d0 = B[i], d1 = B[N + i], d2 = B[2 * N + i], om = B[3 * N + i], ph = B[4 * N + i], w = B[5 * N + i];
            uint32_t ov = 0;                                     // bit k: point k met an argument beyond the range
            for (int k = 0; k < cnt; ++k) {
                const double dot = (d0 * L.px[k] + d1 * L.py[k]) + d2 * L.pz[k];
                const double arg = dot * om + ph;
                ov |= (uint32_t)ws_arg_overflow(arg) << k;
                const int kd = L.kind[k];
                double t;
                if (kd == 0) {
                    t = w * cos_glibc(arg);
                } else {
                    const double dc = kd == 1 ? d0 : (kd == 2 ? d1 : d2);
                    t = ((dc * om) * w) * -sin_glibc(arg);
                }
                L.term[lane * kWsStride + k] = t;
            }
            if (ov) atomicOr(&L.ov, ov);
        }
        __syncthreads();
        if (lane < cnt)
            for (int j = 0; j < m; ++j)
                acc = acc + L.term[j * kWsStride + lane];
        __syncthreads();
    }
    if (lane < cnt) {
        if (L.kind[lane] == 0) {
            const V3d p{L.px[lane], L.py[lane], L.pz[lane]};
            const double basis = N == 0 ? 0.0 : acc * W.sqrt2n;
            double mean;
            int id;
            mean_weight_space(W.base, p, mean, id);
            L.val[lane] = ws_scale(W, p) * basis + mean;
            L.id[lane] = id;
        } else {
            L.val[lane] = acc;
        }
    }
    __syncthreads();
}
GPIS_DEV void ws_put(WsLds &L, int k, V3d p, int kind, int lane)
{
    if (lane == 0) {
        L.px[k] = p.x; L.py[k] = p.y; L.pz[k] = p.z; L.kind[k] = kind;
        if (k == 0) L.ov = 0u;                               // every batch is staged from point 0
    }
}
// point k's value is one the reference computes: its range flag counts
GPIS_DEV void ws_keep(const WsLds &L, int k, bool &overflow) { overflow |= ((L.ov >> k) & 1u) != 0; }

// ---- gradient (WSM:64-156) ----------------------------------------------------------------------------------------------------
GPIS_DEV double ws_det3(const double *m)
{
    return GM(m, 0, 0) * (GM(m, 1, 1) * GM(m, 2, 2) - GM(m, 1, 2) * GM(m, 2, 1)) - GM(m, 0, 1) * (GM(m, 1, 0) * GM(m, 2, 2) - GM(m, 1, 2) * GM(m, 2, 0)) +
           GM(m, 0, 2) * (GM(m, 1, 0) * GM(m, 2, 1) - GM(m, 1, 1) * GM(m, 2, 0));
}
GPIS_DEV double ws_cofactor3(const double *m, int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return GM(m, i1, j1) * GM(m, i2, j2) - GM(m, i1, j2) * GM(m, i2, j1);
}
// jac.inverse().transpose() * g
GPIS_DEV V3d ws_inv_t_mul(const double *m, V3d g)
{
    double c[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) GM(c, i, j) = ws_cofactor3(m, i, j);
    const double det = (GM(c, 0, 0) * GM(m, 0, 0) + GM(c, 1, 0) * GM(m, 1, 0)) + GM(c, 2, 0) * GM(m, 2, 0);
    const double invdet = 1.0 / det;
    double t[9];                                 // transpose of the inverse: t(i, j) = inverse(j, i) = cofactor(i, j) / det
    for (int i = 0; i < 9; ++i) t[i] = c[i] * invdet;
    return V3d{(GM(t, 0, 0) * g.x + GM(t, 0, 1) * g.y) + GM(t, 0, 2) * g.z,
               (GM(t, 1, 0) * g.x + GM(t, 1, 1) * g.y) + GM(t, 1, 2) * g.z,
               (GM(t, 2, 0) * g.x + GM(t, 2, 1) * g.y) + GM(t, 2, 2) * g.z};
}
// sampleGradient with the medium's normal method at p (wave-uniform)
GPIS_DEV V3d ws_gradient(const WsModel &W, WsLds &L, const double *B, V3d p, int lane, bool &overflow, WsTally &tally)
{
    if (W.normal_method == GPIS_NORMAL_FINITE_DIFFERENCES) {
        const float eps = 0.0001f;
        const double e = (double)eps;
        ws_put(L, 0, V3d{p.x + e, p.y + 0.0, p.z + 0.0}, 0, lane);
        ws_put(L, 1, V3d{p.x + 0.0, p.y + e, p.z + 0.0}, 0, lane);
        ws_put(L, 2, V3d{p.x + 0.0, p.y + 0.0, p.z + e}, 0, lane);
        ws_put(L, 3, V3d{p.x - e, p.y - 0.0, p.z - 0.0}, 0, lane);
        ws_put(L, 4, V3d{p.x - 0.0, p.y - e, p.z - 0.0}, 0, lane);
        ws_put(L, 5, V3d{p.x - 0.0, p.y - 0.0, p.z - e}, 0, lane);
        __syncthreads();
        ws_eval_points(W, L, B, 6, lane);
        for (int k = 0; k < 6; ++k) ws_keep(L, k, overflow);
        tally.eval += 6; tally.spec += 6;
        const double den = (double)(2 * eps);
        return V3d{(L.val[0] - L.val[3]) / den, (L.val[1] - L.val[4]) / den, (L.val[2] - L.val[5]) / den};
    }
    // ConditionedGaussian: WeightSpaceRealization::evaluateGradient (WSG:50-76) with the identity shell embedding
    for (int c = 0; c < 3; ++c) ws_put(L, c, p, c + 1, lane);
    __syncthreads();
    ws_eval_points(W, L, B, 3, lane);
    for (int k = 0; k < 3; ++k) ws_keep(L, k, overflow);
    tally.eval += 1; tally.spec += 1;
    V3d g{0., 0., 0.};
    if (W.n > 0) g = V3d{L.val[0] * W.sqrt2n, L.val[1] * W.sqrt2n, L.val[2] * W.sqrt2n};
    const double scale = ws_scale(W, p);
    g = V3d{scale * g.x, scale * g.y, scale * g.z};
    double eps = 0.0001, jac[9];
    do {
        const V3d a{p.x + eps, p.y + 0., p.z + 0.}, b{p.x + 0., p.y + eps, p.z + 0.}, c{p.x + 0., p.y + 0., p.z + eps};
        GM(jac, 0, 0) = (a.x - p.x) / eps; GM(jac, 0, 1) = (a.y - p.y) / eps; GM(jac, 0, 2) = (a.z - p.z) / eps;
        GM(jac, 1, 0) = (b.x - p.x) / eps; GM(jac, 1, 1) = (b.y - p.y) / eps; GM(jac, 1, 2) = (b.z - p.z) / eps;
        GM(jac, 2, 0) = (c.x - p.x) / eps; GM(jac, 2, 1) = (c.y - p.y) / eps; GM(jac, 2, 2) = (c.z - p.z) / eps;
        eps *= 2;
    } while (ws_det3(jac) < 0.0001);
    g = ws_inv_t_mul(jac, g);
    double mean;
    int id;
    mean_weight_space(W.base, p, mean, id);
    const V3d mg = mean_grad(W.base, id, p);
    return V3d{g.x + mg.x, g.y + mg.y, g.z + mg.z};
}

// ---- march (WSM:236-290, step_size > 0) ---------------------------------------------------------------------------------------
GPIS_DEV int ws_sign(double v) { return v < 0 ? -1 : 1; }
GPIS_DEV bool ws_intersect(const WsModel &W, WsLds &L, const double *B, V3d p, V3d rd, float nearT, float farT, float u, bool first_scatter,
                           double &t_out, int &last_gp_id, int lane, bool &overflow, WsTally &tally)
{
    float step_size = (farT - nearT) / (float)W.min_step;
    if (W.step_size < step_size)
        step_size = W.step_size;
    const double farD = (double)farT;
    double t = (double)(nearT + step_size * u);      // float sum, widened
    int sign0 = 1, step = 0;
    double pf = 0.;
    bool have_f0 = false;
    for (;;) {
        int cnt = 0;
        if (!have_f0)
            ws_put(L, cnt++, ray_at(p, rd, (double)nearT), 0, lane);
        for (double tq = t; cnt < kWsK && tq < farD; tq += step_size)
            ws_put(L, cnt++, ray_at(p, rd, tq), 0, lane);
        if (cnt == 0)
            break;
        __syncthreads();
        ws_eval_points(W, L, B, cnt, lane);
        tally.spec += cnt;
        int k = 0;
        if (!have_f0) {
            pf = L.val[0];
            sign0 = ws_sign(pf);
            have_f0 = true;
            k = 1;
            tally.eval++;
            ws_keep(L, 0, overflow);
        }
        for (; k < cnt; ++k) {
            step++;
            const double fc = L.val[k];
            const int signc = ws_sign(fc);
            tally.eval++;
            ws_keep(L, k, overflow);
            if (!first_scatter && step == 1) {
                sign0 = signc;
            } else if (signc != sign0) {
                // refinement (WSM:258-281): candidates lerp(t - step, t, intp 0.9^j), evaluated in batches
                double intp = pf / (pf - fc);
                const double a = t - (double)step_size;
                double t_prev = lerp_d(a, t, intp);
                int gid = L.id[k];
                int tried = 0;
                for (;;) {
                    __syncthreads();
                    int c = 0;
                    for (double ip = intp; c < kWsK;) {
                        ws_put(L, c++, ray_at(p, rd, lerp_d(a, t, ip)), 0, lane);
                        ip *= 0.9;
                        if (ip <= 0.01) break;
                    }
                    __syncthreads();
                    ws_eval_points(W, L, B, c, lane);
                    tally.spec += c;
                    for (int j = 0; j < c; ++j) {
                        const double t_test = lerp_d(a, t, intp);
                        gid = L.id[j];
                        tally.eval++;
                        ws_keep(L, j, overflow);
                        if (ws_sign(L.val[j]) == sign0) {
                            t_out = t_prev; last_gp_id = gid;
                            return true;
                        }
                        intp *= 0.9;
                        // the reference loops for ever when intp is NaN (an infinite field value); stop after kWsMaxRefine
                        if (intp <= 0.01 || ++tried >= kWsMaxRefine) {
                            t_out = 0.; last_gp_id = gid;
                            return true;
                        }
                        t_prev = t_test;
                    }
                }
            }
            pf = fc;
            t += step_size;
        }
        __syncthreads();
        if (!(t < farD))
            break;
    }
    t_out = farD;
    return false;
}

// ---- GaussianProcessMedium::sampleDistance / transmittance (GPM.cpp:221-393) -------------------------------------------------
struct WsRay {
    V3 pos, dir;
    V3d ro, rd, rdn;             // Vec3d(pos), Vec3d(dir), Vec3d(dir).normalized()
    double startT;
    float farT, maxT;
};
GPIS_DEV WsRay ws_ray(const gpis_ray_in &r)
{
    WsRay R;
    R.pos = v3(r.pos[0], r.pos[1], r.pos[2]);
    R.dir = v3(r.dir[0], r.dir[1], r.dir[2]);
    R.ro = to_d(R.pos);
    R.rd = to_d(R.dir);
    double l2 = R.rd.x * R.rd.x; l2 += R.rd.y * R.rd.y; l2 += R.rd.z * R.rd.z;
    const double inv = 1.0 / sqrt(l2);
    R.rdn = V3d{R.rd.x * inv, R.rd.y * inv, R.rd.z * inv};
    R.startT = (double)r.near_t;
    R.farT = r.far_t;
    if (!__builtin_isfinite(R.farT)) R.farT = (float)(R.startT + 2000);
    R.maxT = R.farT;
    return R;
}
// one pass of the do-while of GPM.cpp:268-297 (WSM's intersectGP handles the whole segment in one call)
GPIS_DEV bool ws_transmittance_one(const WsModel &W, WsLds &L, const double *B, const gpis_ray_in &ray, bool &first_scatter, int &last_gp_id,
                                   V3d &last_aniso, int lane, bool &overflow, WsTally &tally)
{
    const WsRay R = ws_ray(ray);
    double startT = R.startT, t = (double)R.maxT;
    bool exited;
    do {
        exited = !ws_intersect(W, L, B, R.ro, R.rd, (float)startT, R.farT, ray.u_jitter, first_scatter, t, last_gp_id, lane, overflow, tally);
        if (t < (double)R.maxT) {
            const V3d grad = ws_gradient(W, L, B, ray_at(R.ro, R.rdn, t), lane, overflow, tally);
            last_aniso = grad;
            first_scatter = false;
            if (!__builtin_isfinite((grad.x + grad.y + grad.z) / 3.0))
                return false;
        }
        startT = t;
    } while (t < (double)R.maxT && exited);
    return exited;
}

// GaussianProcessMedium::sampleDistance (GPM.cpp:299-393) of one segment over the realization B (wave-uniform)
GPIS_DEV gpis_seg_out ws_sample_distance(const WsModel &W, WsLds &L, const double *B, const gpis_ray_in &ray, int lane, bool &overflow, WsTally &tally)
{
    const DevModel &M = W.base;
    bool first_scatter = ray.first_scatter != 0;
    int last_gp_id = ray.last_gp_id;
    V3d last_aniso{ray.last_aniso[0], ray.last_aniso[1], ray.last_aniso[2]};
    gpis_seg_out o{};
    const WsRay R = ws_ray(ray);
    double startT = R.startT;
    const float maxT = R.maxT;
    o.gp_id = last_gp_id;
    o.last_val = ray.last_val;
    V3d aniso = last_aniso;
    bool finished = false;
    if (ray.bounce >= M.max_bounces) {
        o.ok = 0;
        finished = true;
    } else if (maxT == 0.f) {
        o.sample_t = maxT;
        o.weight[0] = o.weight[1] = o.weight[2] = 1.f;
        o.exited = 1;
        const V3 pp = R.pos + R.dir * o.sample_t;
        o.p[0] = pp.x; o.p[1] = pp.y; o.p[2] = pp.z;
        o.scheme = GPIS_UNI;
        o.ok = 1;
        finished = true;
    } else if (M.absorption_only) {
        if (maxT == __builtin_huge_valf()) {
            o.ok = 0;
            finished = true;
        } else {
            o.sample_t = maxT;
            const bool vis = ws_transmittance_one(W, L, B, ray, first_scatter, last_gp_id, last_aniso, lane, overflow, tally);
            o.weight[0] = o.weight[1] = o.weight[2] = vis ? 1.f : 0.f;
            o.exited = 1;
            o.scheme = GPIS_UNI;
            aniso = last_aniso;
        }
    } else {
        double t = (double)maxT;
        bool exited;
        do {
            exited = !ws_intersect(W, L, B, R.ro, R.rd, (float)startT, R.farT, ray.u_jitter, first_scatter, t, last_gp_id, lane, overflow, tally);
            if (t < (double)maxT) {
                const V3d grad = ws_gradient(W, L, B, ray_at(R.ro, R.rdn, t), lane, overflow, tally);
                aniso = grad;
                first_scatter = false;
                if (!__builtin_isfinite((aniso.x + aniso.y + aniso.z) / 3.0)) {
                    aniso = V3d{1., 0., 0.};
                    o.t = t; o.exited = exited; o.ok = 0; o.gp_id = last_gp_id;
                    finished = true;
                    break;
                }
            }
            startT = t;
        } while (t < (double)maxT && exited);
        if (!finished) {
            o.t = t;
            o.exited = exited;
            if (!exited) {
                double d = aniso.x * (double)R.dir.x; d += aniso.y * (double)R.dir.y; d += aniso.z * (double)R.dir.z;
                double l2 = 0.; l2 += aniso.x * aniso.x; l2 += aniso.y * aniso.y; l2 += aniso.z * aniso.z;
                if (d > 0) {
                    o.gp_id = last_gp_id; o.ok = 0;
                    finished = true;
                } else if (l2 < (double)0.0000001f) {
                    aniso = V3d{1., 0., 0.};
                    o.gp_id = last_gp_id; o.ok = 0;
                    finished = true;
                } else {
                    const float col = M.color.enabled ? (float)ramp_eval(M.color, ray_at(R.ro, R.rdn, t)) : 1.f;
                    o.weight[0] = o.weight[1] = o.weight[2] = col;
                    o.continued_weight[0] = o.continued_weight[1] = o.continued_weight[2] = col;
                }
            } else {
                aniso = ws_gradient(W, L, B, ray_at(R.ro, R.rdn, t), lane, overflow, tally);   // GPM.cpp:319
                o.weight[0] = o.weight[1] = o.weight[2] = 1.f;
                o.continued_weight[0] = o.continued_weight[1] = o.continued_weight[2] = 1.f;
            }
            if (!finished) {
                const float ft = (float)t;
                o.sample_t = ft < maxT ? ft : maxT;
                o.continued_t = (float)t;
                for (int c = 0; c < 3; ++c) {
                    o.weight[c] *= M.sigma_s_over_t[c];
                    o.continued_weight[c] *= M.sigma_s_over_t[c];
                }
                o.scheme = GPIS_UNI;
            }
        }
    }
    if (!finished) {
        const V3 pp = R.pos + R.dir * o.sample_t;
        o.p[0] = pp.x; o.p[1] = pp.y; o.p[2] = pp.z;
        o.gp_id = last_gp_id;
        o.ok = 1;
    }
    o.last_val = ray.last_val;
    o.aniso[0] = aniso.x; o.aniso[1] = aniso.y; o.aniso[2] = aniso.z;
    return o;
}

// the end of a marching kernel: lane 0 adds the wave's work counts to the handle's counters
GPIS_DEV void ws_flush_counters(WsCounters *__restrict__ counters, const WsTally &tally, unsigned long long segs, bool overflow, int lane)
{
    if (lane == 0 && counters && segs) {
        atomicAdd(&counters->n_eval, tally.eval);
        atomicAdd(&counters->n_spec, tally.spec);
        atomicAdd(&counters->n_seg, segs);
    }
    // a kept point met an argument beyond the restated range (the flag is wave-uniform: read from LDS by every lane)
    if (lane == 0 && overflow && counters)
        atomicAdd(&counters->arg_overflow, 1ull);
}

template <bool WANT_SAMPLE>
__global__ void __launch_bounds__(64) k_ws_march(const WsModel *__restrict__ Wp, size_t n_rays, const gpis_ray_in *__restrict__ rays,
                                                 gpis_seg_out *__restrict__ outs, uint8_t *__restrict__ visible, double *__restrict__ workspace,
                                                 WsCounters *__restrict__ counters)
{
    __shared__ WsLds L;
    const WsModel &W = *Wp;
    const int lane = (int)threadIdx.x;
    double *own = workspace ? workspace + (size_t)blockIdx.x * 6 * (size_t)W.n : nullptr;
    WsTally tally{0, 0};
    bool overflow = false;
    unsigned long long segs = 0;
    for (size_t idx = blockIdx.x; idx < n_rays; idx += gridDim.x) {
        const gpis_ray_in ray = rays[idx];
        const double *B = W.basis;
        if (!W.single) {
            uint32_t pss[4];
            ws_pss(W, ray.pixel[0], ray.pixel[1], ray.spp, ray.segment, pss);
            ws_build(W, pss, own, W.n, lane);        // each lane reads back only the functions it wrote
            B = own;
        }
        segs++;
        __syncthreads();
        if (!WANT_SAMPLE) {
            bool first_scatter = ray.first_scatter != 0;
            int last_gp_id = ray.last_gp_id;
            V3d last_aniso{ray.last_aniso[0], ray.last_aniso[1], ray.last_aniso[2]};
            const bool vis = ws_transmittance_one(W, L, B, ray, first_scatter, last_gp_id, last_aniso, lane, overflow, tally);
            if (lane == 0) visible[idx] = vis ? 1 : 0;
            continue;
        }
        const gpis_seg_out o = ws_sample_distance(W, L, B, ray, lane, overflow, tally);
        if (lane == 0) outs[idx] = o;
    }
    ws_flush_counters(counters, tally, segs, overflow, lane);
}

// test surface: value, gradient and gp id of the realization of each query (one wave per query)
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_ws_eval(const WsModel *__restrict__ Wp, size_t n, const gpis_ws_query *__restrict__ q,
                                                               double *__restrict__ value, double *__restrict__ grad3, int32_t *__restrict__ gp_id,
                                                               double *__restrict__ workspace, WsCounters *__restrict__ counters)
{
    __shared__ WsLds L;
    const WsModel &W = *Wp;
    const int lane = (int)threadIdx.x;
    double *own = workspace ? workspace + (size_t)blockIdx.x * 6 * (size_t)W.n : nullptr;
    WsTally tally{0, 0};
    bool overflow = false;
    for (size_t idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const gpis_ws_query Q = q[idx];
        const double *B = W.basis;
        if (!W.single) {
            uint32_t pss[4];
            ws_pss(W, Q.pixel[0], Q.pixel[1], Q.spp, Q.segment, pss);
            ws_build(W, pss, own, W.n, lane);
            B = own;
        }
        const V3d p{Q.p[0], Q.p[1], Q.p[2]};
        __syncthreads();
        ws_put(L, 0, p, 0, lane);
        __syncthreads();
        ws_eval_points(W, L, B, 1, lane);
        ws_keep(L, 0, overflow);
        const double v = L.val[0];
        const int id = L.id[0];
        __syncthreads();
        const V3d g = ws_gradient(W, L, B, p, lane, overflow, tally);
        __syncthreads();
        if (lane == 0) {
            if (value) value[idx] = v;
            if (gp_id) gp_id[idx] = id;
            if (grad3) { grad3[3 * idx] = g.x; grad3[3 * idx + 1] = g.y; grad3[3 * idx + 2] = g.z; }
        }
    }
    if (lane == 0 && overflow && counters)
        atomicAdd(&counters->arg_overflow, 1ull);
}

// the basis of n realizations: lane = basis function.  aos: out[r][i][6] (the export), else out[6][N] (the global basis)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_ws_basis(const WsModel *__restrict__ Wp, size_t n, const uint32_t *__restrict__ pss4,
                                                                 double *__restrict__ out, int aos)
{
    const WsModel &W = *Wp;
    const size_t total = n * (size_t)W.n;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t r = g / (size_t)W.n;
        const int i = (int)(g % (size_t)W.n);
        uint32_t pss[4] = {0u, 0u, 0u, 0u};
        if (pss4) ws_pss(W, pss4[4 * r], pss4[4 * r + 1], pss4[4 * r + 2], pss4[4 * r + 3], pss);
        uint64_t sb, sw;
        ws_streams(W, pss, sb, sw);
        double f[6];
        ws_gen(W, sb, sw, i, f);
        if (aos) {
            for (int c = 0; c < 6; ++c) out[g * 6 + c] = f[c];
        } else {
            for (int c = 0; c < 6; ++c) out[(size_t)c * W.n + i] = f[c];
        }
    }
}

}   // namespace gpis
