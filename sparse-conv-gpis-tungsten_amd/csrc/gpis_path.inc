// gpis_path.inc — the flag-dependent part of the device path (covariance layer, noise evaluators,
// conditioning, NEE, intersectGP, sampleDistance, transmittance).  Included by gpis_device.hpp once
// per specialisation with GPIS_PATH_NS and the GPIS_FLAG_* macros set; no include guard on purpose.
#pragma clang fp contract(off)

namespace gpis {
namespace GPIS_PATH_NS {

// ---- means: the analytic ones of gpis_device.hpp or, in the all-features instance, a procedural SDF or tabulated mean (gpis_sdf.hpp) ----
GPIS_DEV void path_mean_weight_space(const DevModel &M, V3d p, double &mean, int &id)
{
    if (GPIS_FLAG_sdf_mean(M)) {
        const sdf::MeanId r = sdf::mean_weight_space(&M, p.x, p.y, p.z);
        mean = r.mean;
        id = r.id;
        return;
    }
    mean_weight_space(M, p, mean, id);
}
GPIS_DEV V3d path_mean_grad(const DevModel &M, int id, V3d p)
{
    if (GPIS_FLAG_sdf_mean(M))
        return sdf::mean_grad(&M, id, p.x, p.y, p.z);
    return mean_grad(M, id, p);
}
// conditioning_finish3d / 1d are shared with the persistent march (gpis_persist.inc), which does not serve procedural / tabulated means: its
// calls take the default SDF_MEAN = false and compile to the analytic means alone, as before
template <bool SDF_MEAN> GPIS_DEV void cond_mean_weight_space(const DevModel &M, V3d p, double &mean, int &id)
{
    if (SDF_MEAN) path_mean_weight_space(M, p, mean, id);
    else mean_weight_space(M, p, mean, id);
}
template <bool SDF_MEAN> GPIS_DEV V3d cond_mean_grad(const DevModel &M, int id, V3d p)
{
    if (SDF_MEAN) return path_mean_grad(M, id, p);
    return mean_grad(M, id, p);
}
// the point of MeanFunction::color on a hit (GPM.cpp:316; ProceduralMean::color, GPF.hpp:1065-1073)
GPIS_DEV V3d path_color_point(const DevModel &M, V3d p) { return GPIS_FLAG_sdf_mean(M) ? sdf::color_point(M, p) : p; }

// ---- covariance layer --------------------------------------------------------------------
GPIS_DEV float ls_field(const DevModel &M, V3d p)   // getKernelScale: the largest component of the ProceduralNoiseVec, GPF.cpp:87-120, 1729-1735
{
    if (GPIS_FLAG_fbm_noise(M) && M.grid.on)
        return grid_kernel_scale(M.grid, (float)p.x, (float)p.y, (float)p.z);          // GridNonstationaryCovariance, GPF.cpp:1409-1420
    if (GPIS_FLAG_fbm_noise(M) && M.ls.type >= GPIS_NOISE_SANDSTONE) {
        double ls[3];
        field_vec(M.ls, p, true, ls);
        const float lx = (float)ls[0], ly = (float)ls[1], lz = (float)ls[2];
        const float mxy = lx < ly ? ly : lx;
        return mxy < lz ? lz : mxy;
    }
    return (float)ramp_eval(M.ls, p);
}
GPIS_DEV float cov_lateral_scale(const DevModel &M, V3 p) { return GPIS_FLAG_nonstationary(M) ? ls_field(M, to_d(p)) : 1.0f; }
GPIS_DEV float cov_ns_scale(const DevModel &M, V3 p)
{
    if (!GPIS_FLAG_nonstationary(M) || GPIS_FLAG_multi_resolution_grid(M))
        return 1.f;
    return cov_lateral_scale(M, p) / M.ls_maxval;
}
GPIS_DEV float cov_world_sampling_scale(const DevModel &M) { return GPIS_FLAG_nonstationary(M) ? M.ls_maxval : 1.f; }
GPIS_DEV float cov_kernel_radius(const DevModel &M, bool isIdentity, float localScale)
{
    if (!GPIS_FLAG_nonstationary(M))
        return isIdentity ? M.radius_iso : (localScale == 1.0f ? M.radius_world : M.kernel_scale * localScale * M.mtx_factor);
    localScale = (float)((double)localScale * (GPIS_FLAG_multi_resolution_grid(M) ? 1.0 : (double)M.ls_maxval));
    localScale *= GPIS_FLAG_aniso_field(M) ? 1.5f : 1.f;            // sparseConvNoiseMaxAnisotropyScale(), GPF.cpp:1743-1747
    if (isIdentity)
        return M.kernel_scale;
    return M.kernel_scale * localScale * M.mtx_factor;
}
GPIS_DEV float se_variance3d(const DevModel &M, float dens, float R, bool isIdentity, float globalScale, float localScale)
{
    double idua = (double)(dens / (R * R * R));
    double cds = 1.0;
    if (!isIdentity) {
        cds = M.cov_det_sqrt_world;
        cds *= pow_glibc((double)globalScale, 3.0);
    }
    if (localScale != 1.0f)               // pow(1, 3) = 1 exactly; the multi-resolution grid always passes 1 (one call per evaluation saved)
        cds *= pow_glibc((double)localScale, 3.0);
    double iks = M.pi_pow_1_5 * cds;
    return (float)(idua * iks);
}
GPIS_DEV float se_variance1d(const DevModel &M, float dens, float R, float localScale)
{
    double idua = (double)(dens / R);
    double iks = M.sqrt_pi * (double)localScale;
    return (float)(idua * iks);
}
GPIS_DEV float cov_norm3d(const DevModel &M, V3 p, float dens, float R, bool isIdentity, float globalScale)
{
    if (!GPIS_FLAG_nonstationary(M))
        return isIdentity ? M.norm3d_iso : M.norm3d_world;
    float localScale = GPIS_FLAG_multi_resolution_grid(M) ? 1.0f : cov_ns_scale(M, p);
    return sqrtf(se_variance3d(M, dens, R, isIdentity, globalScale, localScale));
}
GPIS_DEV float cov_norm1d(const DevModel &M, V3 p, float dens, float R)
{
    if (!GPIS_FLAG_nonstationary(M))
        return M.norm1d;
    return sqrtf(se_variance1d(M, dens, R, cov_ns_scale(M, p)));
}
GPIS_DEV float cov_xf_scale(const DevModel &M, float globalScale)
{
    if (!GPIS_FLAG_nonstationary(M))
        return globalScale;
    return GPIS_FLAG_multi_resolution_grid(M) ? globalScale : M.ls_maxval;
}
// x / 1.0f and x * 1.0f are exact, so the (wave-uniform) unit scale of stationary kernels skips the IEEE divide
GPIS_DEV V3 cov_pos_w2l(const DevModel &M, V3 v, float s) { float c = cov_xf_scale(M, s); V3 r = eig_matvec(M.w2l, v); return c == 1.0f ? r : r / c; }
GPIS_DEV V3 cov_grad_w2l(const DevModel &M, V3 v, float s) { float c = cov_xf_scale(M, s); V3 r = eig_matvec(M.l2w_T, v); return c == 1.0f ? r : r * c; }
GPIS_DEV V3 cov_grad_l2w(const DevModel &M, V3 v, float s) { float c = cov_xf_scale(M, s); V3 r = eig_matvec(M.w2l_T, v); return c == 1.0f ? r : r / c; }
GPIS_DEV float cov_splat_cov_1d(const DevModel &M, V3 pq, V3 pc)
{
    if (!GPIS_FLAG_nonstationary(M))
        return 1.0f;
    float a = cov_ns_scale(M, pq), b = cov_ns_scale(M, pc);
    float scale = (float)(0.5 * (double)(a * a + b * b));
    return sqrtf(scale);
}

GPIS_DEV void mat3_matmul_eig(const float *a, const float *b, float *out)
{
    float t[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            GM(t, r, c) = sum3e(GM(a, r, 0) * GM(b, 0, c), GM(a, r, 1) * GM(b, 1, c), GM(a, r, 2) * GM(b, 2, c));
    for (int i = 0; i < 9; ++i) out[i] = t[i];
}
// inverse of getNonstationaryAniso3D(p_world) (GPF.cpp:1678-1689, compute_ansio_full GPF.cpp:27-40): false without a field.
// cosf and sinf of one angle: one sincosf call in a gcc build — the host's, restated in gpis_libm.hpp.
GPIS_DEV bool cov_ns_aniso3d_inv(const DevModel &M, V3 p_world, float *inv)
{
    if (!GPIS_FLAG_aniso_field(M))
        return false;
    const float pi_half = 3.1415926536f * 0.5f;
    const float angle = (float)(field_scalar(M.aniso, to_d(p_world), GPIS_FLAG_fbm_noise(M)) * (double)pi_half);
    float cs, sn;
    sincosf_glibc(angle, &sn, &cs);
    const float V[9] = {cs, sn, 0.f, -sn, cs, 0.f, 0.f, 0.f, 1.f}, S[9] = {1.5f, 0.f, 0.f, 0.f, 1.f / 1.5f, 0.f, 0.f, 0.f, 1.f};
    float SV[9], SVt[9], an[9];
    mat3_matmul_eig(S, V, SV);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) GM(SVt, r, c) = GM(SV, c, r);
    mat3_matmul_eig(SVt, SV, an);
    eig_inverse3(an, inv);
    return true;
}
// invSigma^T * aniso_inv * invSigma (GPF.cpp:716-726, 776-786)
GPIS_DEV void se_sandwich(const DevModel &M, bool isIso, bool divideGlobal, float globalScale, const float *aniso_inv, float *out)
{
    float iS[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, iSt[9], T[9];
    if (!isIso) {
        for (int i = 0; i < 9; ++i) iS[i] = M.w2l[i];
        if (divideGlobal)
            for (int i = 0; i < 9; ++i) iS[i] /= globalScale;
    }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) GM(iSt, r, c) = GM(iS, c, r);
    mat3_matmul_eig(iSt, aniso_inv, T);
    mat3_matmul_eig(T, iS, out);
}
// SE::getInvCovMtx, GPF.cpp:774-802
GPIS_DEV void se_inv_cov_mtx(const DevModel &M, bool isCov, bool isIso, float globalScale, float localScale, float *A, const float *aniso_inv = nullptr)
{
    if (aniso_inv) {
        se_sandwich(M, isIso, true, globalScale, aniso_inv, A);
    } else if (isIso) {
        for (int i = 0; i < 9; ++i) A[i] = 0.f;
        A[0] = A[4] = A[8] = 1.f;
    } else {
        float g2 = globalScale * globalScale;
        for (int i = 0; i < 9; ++i) A[i] = M.invcov_world[i] / g2;
    }
    if (isCov)
        for (int i = 0; i < 9; ++i) A[i] *= 0.5f;
    float l2 = localScale * localScale;
    for (int i = 0; i < 9; ++i) A[i] /= l2;
    for (int i = 0; i < 9; ++i) A[i] *= 0.5f;
}
// Matérn (v = 0.5, 1.5, 2.5) and Gabor splatting kernels, value and gradient (GPF.cpp:1048-1082, 1140-1150, 1205-1214): evaluated
// in double like the reference (device exp / pow / sin / cos: toleranced parity)
GPIS_DEV V4 other_splat3d(const DevModel &M, V3 ab)
{
    const double kPi = 3.14159265358979323846;
    const float l = M.k_l, a = M.gabor_a, f = M.gabor_f;
    if (M.kernel_type == GPIS_KERNEL_MATERN) {
        double abLen = (double)length(ab);
        float val, gs;
        if (M.matern_v == 0.5f) {
            const double e = exp_glibc(-abLen / (double)l);
            val = (float)(e / abLen);
            gs = -(float)(e * (1 / pow_glibc(abLen, 3.0) - 1 / ((abLen * abLen) * (double)l)));      // pow(x, 2.0) is x * x in a gcc build
        } else if (M.matern_v == 1.5f) {                      // GPF.cpp:1053-1056, 1071-1074 (own K0 / K1: gpis_device.hpp)
            const double r_scl = sqrt(3.) * abLen / (double)l;
            double k0, k1;
            bessel_k01(r_scl, &k0, &k1);
            val = (float)k0;
            gs = -(float)(k1 * sqrt(3.) / (double)l / abLen);
        } else {
            const double e = exp_glibc(-sqrt(5.) * abLen / (double)l);
            val = (float)e;
            gs = -(float)(e * sqrt(5.) / (double)l / abLen);
        }
        return v4(val, gs * ab.x, gs * ab.y, gs * ab.z);
    }
    if (M.kernel_type == GPIS_KERNEL_GABOR_ANISO) {
        const V3 om = v3(M.gabor_omega[0], M.gabor_omega[1], M.gabor_omega[2]);
        const float od = dot(om, ab);
        const float l2 = length_sq(ab);
        const double env = exp_glibc(-kPi * (double)(a * a) * (double)l2);
        const double ph = (double)2.f * kPi * (double)f * (double)od;
        double sph, cph;                 // the value function takes the cosine alone (cos), the gradient function both (one sincos
        sincos_glibc(ph, &sph, &cph);    // call in a gcc build): different last bits, gpis_libm.hpp
        const float val = (float)(env * cos_glibc(ph));
        const float A = (float)env, B = (float)cph;
        const float c1 = -(float)((double)A * sph * (double)2.f * kPi * (double)f);
        const float c2 = (float)((double)(B * A * 2.f) * kPi * (double)(a * a));        // B A 2.f: float products (GPF.cpp:1148)
        const V3 g = om * c1 - ab * c2;
        return v4(val, g.x, g.y, g.z);
    }
    const float r = length(ab);
    const float ar = a * r;
    double s2, c2;                       // value: sin alone; gradient: both (sincos)
    sincos_glibc(2 * kPi * (double)f * (double)r, &s2, &c2);
    const float val = (float)(exp_glibc(-kPi * (double)(ar * ar)) * 2 * (double)f / (double)r * sin_glibc(2 * kPi * (double)f * (double)r));
    const float gs = (float)(2 * (double)f * exp_glibc(-kPi * (double)(a * a) * (double)length_sq(ab)) *
                             (-s2 / pow_glibc((double)r, 3.0) - 2 * kPi * (double)(a * a) * s2 / (double)r + 2 * kPi * (double)f * c2 / (double)(r * r)));
    return v4(val, gs * ab.x, gs * ab.y, gs * ab.z);
}
// splattingKernel3D (value, gradient) for a given matrix, GPF.cpp:552-562, 804-817
GPIS_DEV V4 se_splat3d(V3 ab, const float *A)
{
    V3 t = eig_row_times(ab, A);
    float absq = sum3e(t.x * ab.x, t.y * ab.y, t.z * ab.z);
    float f = expf_glibc(-absq);
    return v4(f, -2.f * t.x * f, -2.f * t.y * f, -2.f * t.z * f);
}
// splattingKernel3DGrad, GPF.cpp:564-577, 819-833
GPIS_DEV V4 se_splat3d_grad(V3 ab, const float *A, V3 coeff)
{
    V3 t = eig_row_times(ab, A);
    float absq = sum3e(t.x * ab.x, t.y * ab.y, t.z * ab.z);
    float f = expf_glibc(-absq);
    float dx = -2.f * t.x, dy = -2.f * t.y, dz = -2.f * t.z;
    float gx = dx * f, gy = dy * f, gz = dz * f;
    float h00 = (dx * dx - 2.f * GM(A, 0, 0)) * f, h11 = (dy * dy - 2.f * GM(A, 1, 1)) * f, h22 = (dz * dz - 2.f * GM(A, 2, 2)) * f;
    float h01 = (dx * dy - 2.f * GM(A, 0, 1)) * f, h02 = (dx * dz - 2.f * GM(A, 0, 2)) * f, h12 = (dy * dz - 2.f * GM(A, 1, 2)) * f;
    V4 vx = v4(gx, h00, h01, h02), vy = v4(gy, h01, h11, h12), vz = v4(gz, h02, h12, h22);
    return (vx * coeff.x + vy * coeff.y) + vz * coeff.z;
}
// SE 1D family, GPF.cpp:835-865
GPIS_DEV float se_splat1d_val(float ab, float ls)
{
    float den = (float)(2.0 * (double)(ls * ls));
    return expf_glibc(-(ab * ab / den));
}
GPIS_DEV float sqrt2_scaled(float ls) { return (float)((double)ls * 1.4142135623730951); }   // ls * sqrt(2) in double
GPIS_DEV float se_splat1d_grad(float ab, float ls)
{
    float f = se_splat1d_val(ab, ls);
    float den = (float)(2.0 * (double)(ls * ls));
    return (float)(-2.0 * (double)ab / (double)den * (double)f);
}
GPIS_DEV float se_cov1d_val(float ab, float ls) { return se_splat1d_val(ab, sqrt2_scaled(ls)); }
GPIS_DEV float se_cov1d_grad(float ab, float ls) { return se_splat1d_grad(ab, sqrt2_scaled(ls)); }
GPIS_DEV float se_cov2d_2nd(float ab, float ls)
{
    float f = se_cov1d_val(ab, ls);
    float den = (float)(4.0 * (double)(ls * ls));
    float g1 = (float)(-2.0 * (double)ab / (double)den);
    return (float)(((double)(g1 * g1) - 2.0 / (double)den) * (double)f);
}
GPIS_DEV float se_cov2d_2nd_normal(float ab, float ls)
{
    float f = se_cov1d_val(ab, ls);
    float den = (float)(4.0 * (double)(ls * ls));
    return (float)(-2.0 / (double)den * (double)f);
}
// sparseConvNoiseOneOverSecondDerivative, GPF.cpp:713-739
GPIS_DEV void cov_one_over_second_derivative(const DevModel &M, V3 p_world, bool isIso, float *out)
{
    float S[9], An[9], Ai[9];
    const bool has = cov_ns_aniso3d_inv(M, p_world, Ai);
    if (has)
        se_sandwich(M, isIso, false, 1.f, Ai, An);
    for (int i = 0; i < 9; ++i) {
        float a = has ? An[i] : (isIso ? ((i == 0 || i == 4 || i == 8) ? 1.f : 0.f) : M.invcov_world[i]);
        a *= 0.25f;
        S[i] = -2.f * a;
    }
    eig_inverse3(S, out);
}

// ---- noise evaluator (SCN.cpp) -----------------------------------------------------------
GPIS_DEV uint32_t compute_seed(const DevModel &M, const RayInfo &info)   // SCN.cpp:40-49
{
    uint32_t seed = M.seed;
    if (!M.single_realization) {
        uint32_t w = M.ctx == GPIS_CTX_GLOBAL ? 0u : info.seg;
        seed += xxhash32_4(info.px, info.py, info.spp, w) + xxhash32_1(info.scene_seed);
    }
    return seed;
}

// kernelScaleLevelRatio, SCN.cpp:60-70 (+ the additional_seed of SCN.cpp:252 from the host tables)
GPIS_DEV LevelInfo kernel_scale_level_ratio(const DevModel &M, V3 p)
{
    LevelInfo L;
    float ls = cov_lateral_scale(M, p);
    float level_low = floorf(logf_glibc(ls) / M.log_base);
    int li = (int)level_low;
    li = li < kLevelMin ? kLevelMin : (li > kLevelMax - 1 ? kLevelMax - 1 : li);
    L.lo = M.level_scale[li - kLevelMin];
    L.hi = M.level_scale[li + 1 - kLevelMin];
    L.add_lo = M.level_addseed[li - kLevelMin];
    L.add_hi = M.level_addseed[li + 1 - kLevelMin];
    float frac = (ls - L.lo) / (L.hi - L.lo);
    double fd = (double)frac;
    double den = sqrt(1.0 - 2.0 * fd + 2.0 * fd * fd);
    L.ratio_lo = (float)((1.0 - fd) / den);
    L.ratio_hi = (float)(fd / den);
    return L;
}

// cell3D, SCN.cpp:375-395.  A = getInvCovMtx for this evaluation (constant over the cell).
GPIS_DEV V4 cell3d(const DevModel &M, uint32_t ci, uint32_t cj, uint32_t ck, V3 p, uint32_t seed, float R, const float *A, bool diag)
{
    Pcg32 s;
    s.set_state((uint64_t)(uint32_t)(xxhash32_4(ck, cj, ci, seed) + 1u));
    V4 sum = v4(0.f, 0.f, 0.f, 0.f);
    const V3 Rp = R * p;
    const uint32_t n = M.n_impulses;
    for (uint32_t k = 0u; k < n; ++k) {
        float pz = normalized_uint(s.next_i());
        float py = normalized_uint(s.next_i());
        float px = normalized_uint(s.next_i());
        uint32_t wi = s.next_i();
        V3 to_point = p - v3(px, py, pz);
        if (length_sq(to_point) < 1.0f) {
            V3 ab = Rp - R * v3(px, py, pz);
            V4 k4;
            if (GPIS_FLAG_other_kernels(M)) {
                k4 = other_splat3d(M, ab);
            } else {
                V3 t = diag ? v3(ab.x * A[0], ab.y * A[4], ab.z * A[8]) : eig_row_times(ab, A);
                float absq = sum3e(t.x * ab.x, t.y * ab.y, t.z * ab.z);
                float f = expf_glibc(-absq);
                k4 = v4(f, -2.f * t.x * f, -2.f * t.y * f, -2.f * t.z * f);
            }
            // Bernoulli(next1D(), -1, 1, 0.5): rv < 0.5  ⇔  top mantissa bit clear
            float w_i = (wi >> 31) ? 1.f : -1.f;
            sum = sum + w_i * k4;
        }
    }
    return sum;
}
// noise3D, SCN.cpp:362-373.  In the all-features instance the lattice sum is ONE out-of-line function (the kernel matrix travels
// in registers): that instance reaches it from ~100 inlined call sites (world / isotropic-ray, two levels, diagonal / full
// matrix, times every evaluation site of the march), each with the Matern / Gabor branches inside — inlined, the one kernel took
// seven minutes to compile.  The specialised instances keep it inline.
#ifdef GPIS_PATH_OUTLINE_NOISE3D
GPIS_DEV V4 noise3d_body(const DevModel &M, V3 p, uint32_t seed, float R, const float *A, bool diag);
static __device__ __attribute__((noinline)) V4 noise3d_outlined(const DevModel *Mp, float px, float py, float pz, uint32_t seed, float R, Mat9 A, bool diag)
{
    return noise3d_body(*Mp, v3(px, py, pz), seed, R, A.m, diag);
}
GPIS_DEV V4 noise3d(const DevModel &M, V3 p, uint32_t seed, float R, const float *A, bool diag)
{
    Mat9 a;
    for (int i = 0; i < 9; ++i) a.m[i] = A[i];
    return noise3d_outlined(&M, p.x, p.y, p.z, seed, R, a, diag);
}
GPIS_DEV V4 noise3d_body(const DevModel &M, V3 p, uint32_t seed, float R, const float *A, bool diag)
#else
GPIS_DEV V4 noise3d(const DevModel &M, V3 p, uint32_t seed, float R, const float *A, bool diag)
#endif
{
    V3 pg = p / R;
    V3 fl = v3(floorf(pg.x), floorf(pg.y), floorf(pg.z));
    V3 frac = pg - fl;
    int i = (int)fl.x, j = (int)fl.y, k = (int)fl.z;
    V4 sum = v4(0.f, 0.f, 0.f, 0.f);
    // the loops stay rolled: 27 inlined copies of cell3d buy nothing and cost registers.  (Skipping
    // neighbour cells that lie wholly beyond the cut-off is exact but was measured at 1.5 % on C3 —
    // lanes rarely agree on which cells to skip — and its extra live values cost the cooperative
    // kernels, which inline this function as their cold fallback, 48 B/lane of scratch: not done.)
#pragma unroll 1
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll 1
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll 1
            for (int dz = -1; dz <= 1; ++dz)
                sum = sum + cell3d(M, (uint32_t)(i + dx), (uint32_t)(j + dy), (uint32_t)(k + dz),
                                   frac - v3((float)dx, (float)dy, (float)dz), seed, R, A, diag);
    return sum;
}
// cell1D / noise1D, SCN.cpp:397-428
template <bool WITH_GRAD = true>
GPIS_DEV void noise1d(const DevModel &M, V3 p_world, float t, uint32_t seed, float R, float &ov, float &og)
{
    float tg = t / R;
    float fl = floorf(tg);
    float frac = tg - fl;
    int i = (int)fl;
    float ls = 1.0f;
    if (GPIS_FLAG_nonstationary(M)) {
        ls = cov_ns_scale(M, p_world);
        ls *= 1.0f;
    }
    // se_splat1d_val / se_splat1d_grad (GPF.cpp:835-845) divide by den = 2 ls^2, which does not change inside this sum.  A
    // correctly rounded quotient by an invariant divisor needs no division: with y = RN(1/den) (one IEEE division here),
    // q = RN(a y), r = a - den q (exact in an fma), q' = RN(q + r y) is RN(a / den) (Markstein's theorem; checked against `/` on
    // 2.8e9 operand pairs in fp32 and fp64, including significands next to all-ones and next to powers of two: 0 differences).
    // 3 instructions instead of the 10 (fp32) / 12 with a quarter-rate v_rcp_f64 (fp64) of the division sequences, per impulse.
    const float den = (float)(2.0 * (double)(ls * ls));
    const float rden = 1.0f / den;
    const double den_d = (double)den, rden_d = 1.0 / den_d;
    float sv = 0.f, sg = 0.f;
#pragma unroll 1
    for (int dx = -1; dx <= 1; ++dx) {
        Pcg32 s;
        s.set_state((uint64_t)(uint32_t)(xxhash32_2((uint32_t)(i + dx), seed) + 1u));
        float tc = frac - (float)dx;
        float cv = 0.f, cg = 0.f;
        for (uint32_t k = 0u; k < M.n_impulses; ++k) {
            float t_i = normalized_uint(s.next_i());
            uint32_t wi = s.next_i();
            float to_point = tc - t_i;
            if (to_point * to_point < 1.0f) {
                float ab = R * tc - R * t_i;
                float w_i = (wi >> 31) ? 1.f : -1.f;
                const float x = ab * ab;
                float q = x * rden;
                q = __builtin_fmaf(__builtin_fmaf(-q, den, x), rden, q);                 // = ab * ab / den
                const float f = expf_glibc(-q);                                          // se_splat1d_val
                cv += w_i * f;
                if (WITH_GRAD) {
                    const double a = -2.0 * (double)ab;
                    double qd = a * rden_d;
                    qd = __builtin_fma(__builtin_fma(-qd, den_d, a), rden_d, qd);        // = -2 ab / den in double
                    cg += w_i * (float)(qd * (double)f);                                 // se_splat1d_grad
                }
            }
        }
        sv += cv; sg += cg;
    }
    ov = sv; og = sg;
}

GPIS_DEV V3 coeff_origin(const gpis_cond_coeff &c) { return v3(c.ray_origin[0], c.ray_origin[1], c.ray_origin[2]); }
GPIS_DEV V3 coeff_gs(const gpis_cond_coeff &c) { return v3(c.gradient_scale[0], c.gradient_scale[1], c.gradient_scale[2]); }

// The evaluators below are split into the part before the lattice sum (the point in grid space, the cell seed,
// the kernel matrix), the sum itself (noise3d / noise1d, 27 rho or 3 rho impulses) and the part after it
// (normalisation, transforms, conditioning splat), so that the persistent march kernels (gpis_persist.inc) can
// run the sums of 64 rays in lockstep while everything else stays per-lane code shared with this file.
struct Job3 {            // one noise3D call (SCN.cpp:362-373) with a diagonal kernel matrix
    V3 frac;             // p / R - floor(p / R)
    int i, j, k;         // floor(p / R)
    uint32_t seed;
    float R, A0, A1, A2;
};
GPIS_DEV Job3 job3_at(V3 p, uint32_t seed, float R, const float *A)
{
    Job3 J;
    V3 pg = p / R;
    V3 fl = v3(floorf(pg.x), floorf(pg.y), floorf(pg.z));
    J.frac = pg - fl;
    J.i = (int)fl.x; J.j = (int)fl.y; J.k = (int)fl.z;
    J.seed = seed; J.R = R;
    J.A0 = A[0]; J.A1 = A[4]; J.A2 = A[8];
    return J;
}
GPIS_DEV Job3 job3_world(const DevModel &M, V3 p, uint32_t seed, int addseed, float R, float kss)
{
    float A[9];
    se_inv_cov_mtx(M, false, false, kss, cov_ns_scale(M, p), A);
    return job3_at(p, seed + (uint32_t)addseed, R, A);
}
GPIS_DEV V4 post3_world(const DevModel &M, const Realization &r, V3 p, V4 noise, float R, float kss, bool conditioning)
{
    noise = noise / cov_norm3d(M, p, M.impulse_density, R, false, kss);
    if (GPIS_FLAG_activate_conditioning(M) && conditioning) {
        float C[9];
        se_inv_cov_mtx(M, true, false, kss, cov_ns_scale(M, p), C);
        V3 ab = p - coeff_origin(r.c);
        if (GPIS_FLAG_other_kernels(M)) {
            // these kernels have no second derivative of their own: the base class returns a zero matrix (GPF.hpp:1518-1521)
            const V4 k = other_splat3d(M, ab);
            const V3 gs = coeff_gs(r.c);
            const V4 vx = v4(k.gx, 0.f, 0.f, 0.f), vy = v4(k.gy, 0.f, 0.f, 0.f), vz = v4(k.gz, 0.f, 0.f, 0.f);
            noise = noise + (k * r.c.value_scale + ((vx * gs.x + vy * gs.y) + vz * gs.z));
        } else {
            noise = noise + (se_splat3d(ab, C) * r.c.value_scale + se_splat3d_grad(ab, C, coeff_gs(r.c)));
        }
    }
    return noise;
}
GPIS_DEV Job3 job3_iso_ray(const DevModel &M, V3 p, V3 rayDir, uint32_t seed, int addseed, float R, float kss)
{
    V3 ray_dir_iso = normalized(cov_pos_w2l(M, rayDir, 1.0f));
    Frame coord = frame_from_normal(ray_dir_iso);
    V3 p_iso_ray = to_local(coord, cov_pos_w2l(M, p, kss));
    float A[9];
    se_inv_cov_mtx(M, false, true, 1.0f, cov_ns_scale(M, p), A);
    return job3_at(p_iso_ray, seed + (uint32_t)addseed, R, A);
}
GPIS_DEV V4 post3_iso_ray(const DevModel &M, const Realization &r, V3 p, V3 rayDir, V4 n, float R, float kss, bool conditioning)
{
    V3 ray_dir_iso = normalized(cov_pos_w2l(M, rayDir, 1.0f));
    Frame coord = frame_from_normal(ray_dir_iso);
    V3 p_iso_ray = to_local(coord, cov_pos_w2l(M, p, kss));
    V3 gw = cov_grad_l2w(M, to_global(coord, v3(n.gx, n.gy, n.gz)), kss);
    V4 nw = v4(n.v, gw.x, gw.y, gw.z) / cov_norm3d(M, p, M.impulse_density, R, true, 1.0f);
    if (GPIS_FLAG_activate_conditioning(M) && conditioning) {
        V3 origin_iso_ray = to_local(coord, cov_pos_w2l(M, coeff_origin(r.c), kss));
        float C[9];
        se_inv_cov_mtx(M, true, true, 1.0f, cov_ns_scale(M, p), C);
        V3 ab = p_iso_ray - origin_iso_ray;
        V4 d = se_splat3d(ab, C) * r.c.value_scale + se_splat3d_grad(ab, C, coeff_gs(r.c));
        V3 gdw = cov_grad_l2w(M, to_global(coord, v3(d.gx, d.gy, d.gz)), kss);
        nw = nw + v4(d.v, gdw.x, gdw.y, gdw.z);
    }
    return nw;
}
// (seed offset, kernel radius, sampling scale) of level 0 / 1 of evaluateNoise3D (SCN.cpp:101-124)
struct LevelParams { int addseed; float R, kss; };
GPIS_DEV LevelParams level_params3(const DevModel &M, const LevelInfo &L, int level)
{
    LevelParams P;
    if (!GPIS_FLAG_multi_res(M)) {
        P.addseed = M.iso3d ? 0 : M.world_addseed;
        P.kss = M.iso3d ? 1.0f : cov_world_sampling_scale(M);
        P.R = M.iso3d ? cov_kernel_radius(M, true, 1.0f) : cov_kernel_radius(M, false, 1.0f);
        return P;
    }
    P.addseed = level ? L.add_hi : L.add_lo;
    P.kss = level ? L.hi : L.lo;
    P.R = M.iso3d ? cov_kernel_radius(M, true, 1.0f) : cov_kernel_radius(M, false, P.kss);
    return P;
}

// evaluateNoise3DNormalized (world space), SCN.cpp:251-260
GPIS_DEV V4 eval_noise3d_world(const DevModel &M, const Realization &r, V3 p, uint32_t seed, int addseed, float R, float kss, bool conditioning)
{
    if (!M.use_aniso_mtx && !GPIS_FLAG_aniso_field(M)) {
        Job3 J = job3_world(M, p, seed, addseed, R, kss);
        const float Ad[9] = {J.A0, 0.f, 0.f, 0.f, J.A1, 0.f, 0.f, 0.f, J.A2};
        return post3_world(M, r, p, noise3d(M, p, J.seed, R, Ad, true), R, kss, conditioning);
    }
    float A[9], Ai[9];
    const bool has = cov_ns_aniso3d_inv(M, p, Ai);
    se_inv_cov_mtx(M, false, false, kss, cov_ns_scale(M, p), A, has ? Ai : nullptr);
    V4 noise = noise3d(M, p, seed + (uint32_t)addseed, R, A, false);
    noise = noise / cov_norm3d(M, p, M.impulse_density, R, false, kss);
    if (GPIS_FLAG_activate_conditioning(M) && conditioning) {
        float C[9];
        se_inv_cov_mtx(M, true, false, kss, cov_ns_scale(M, p), C, has ? Ai : nullptr);
        V3 ab = p - coeff_origin(r.c);
        noise = noise + (se_splat3d(ab, C) * r.c.value_scale + se_splat3d_grad(ab, C, coeff_gs(r.c)));
    }
    return noise;
}
// evaluateNoise3DIsotropicRayNormalized, SCN.cpp:291-320
GPIS_DEV V4 eval_noise3d_iso_ray(const DevModel &M, const Realization &r, V3 p, V3 rayDir, uint32_t seed, int addseed, float R, float kss, bool conditioning)
{
    if (GPIS_FLAG_aniso_field(M)) {
        // full kernel matrix per evaluation (the aniso field's matrix at the query's world position)
        const Frame coord = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, 1.0f)));
        const V3 p_iso_ray = to_local(coord, cov_pos_w2l(M, p, kss));
        float A[9], Ai[9];
        cov_ns_aniso3d_inv(M, p, Ai);
        se_inv_cov_mtx(M, false, true, 1.0f, cov_ns_scale(M, p), A, Ai);
        const V4 n = noise3d(M, p_iso_ray, seed + (uint32_t)addseed, R, A, false);
        const V3 gw = cov_grad_l2w(M, to_global(coord, v3(n.gx, n.gy, n.gz)), kss);
        V4 nw = v4(n.v, gw.x, gw.y, gw.z) / cov_norm3d(M, p, M.impulse_density, R, true, 1.0f);
        if (GPIS_FLAG_activate_conditioning(M) && conditioning) {
            const V3 origin_iso_ray = to_local(coord, cov_pos_w2l(M, coeff_origin(r.c), kss));
            float C[9];
            se_inv_cov_mtx(M, true, true, 1.0f, cov_ns_scale(M, p), C, Ai);
            const V3 ab = p_iso_ray - origin_iso_ray;
            const V4 d = se_splat3d(ab, C) * r.c.value_scale + se_splat3d_grad(ab, C, coeff_gs(r.c));
            const V3 gdw = cov_grad_l2w(M, to_global(coord, v3(d.gx, d.gy, d.gz)), kss);
            nw = nw + v4(d.v, gdw.x, gdw.y, gdw.z);
        }
        return nw;
    }
    // the same arithmetic through the job / post split (one source of truth for the persistent kernels)
    Job3 J = job3_iso_ray(M, p, rayDir, seed, addseed, R, kss);
    const float Ad[9] = {J.A0, 0.f, 0.f, 0.f, J.A1, 0.f, 0.f, 0.f, J.A2};
    V3 pir = to_local(frame_from_normal(normalized(cov_pos_w2l(M, rayDir, 1.0f))), cov_pos_w2l(M, p, kss));
    return post3_iso_ray(M, r, p, rayDir, noise3d(M, pir, J.seed, R, Ad, true), R, kss, conditioning);
}
// evaluateNoise3D, SCN.cpp:101-124
GPIS_DEV V4 eval_noise3d(const DevModel &M, Realization &r, V3 p, V3 rayDir, uint32_t seed, bool conditioning)
{
    r.n_eval++;
    if (!M.iso3d) {
        if (!GPIS_FLAG_multi_res(M)) {
            float kss = cov_world_sampling_scale(M);
            return eval_noise3d_world(M, r, p, seed, M.world_addseed, cov_kernel_radius(M, false, 1.0f), kss, conditioning);
        }
        LevelInfo L = kernel_scale_level_ratio(M, p);
        V4 lo = eval_noise3d_world(M, r, p, seed, L.add_lo, cov_kernel_radius(M, false, L.lo), L.lo, conditioning);
        V4 hi = eval_noise3d_world(M, r, p, seed, L.add_hi, cov_kernel_radius(M, false, L.hi), L.hi, conditioning);
        return L.ratio_lo * lo + L.ratio_hi * hi;
    }
    if (!GPIS_FLAG_multi_res(M))
        return eval_noise3d_iso_ray(M, r, p, rayDir, seed, 0, cov_kernel_radius(M, true, 1.0f), 1.0f, conditioning);
    LevelInfo L = kernel_scale_level_ratio(M, p);
    V4 lo = eval_noise3d_iso_ray(M, r, p, rayDir, seed, L.add_lo, cov_kernel_radius(M, true, 1.0f), L.lo, conditioning);
    V4 hi = eval_noise3d_iso_ray(M, r, p, rayDir, seed, L.add_hi, cov_kernel_radius(M, true, 1.0f), L.hi, conditioning);
    return L.ratio_lo * lo + L.ratio_hi * hi;
}

// evaluateNoise1DNormalized, SCN.cpp:322-360 → (value, gx_cond, gy_cond, gz); split like the 3D evaluators:
// job1_coord = the abscissa handed to noise1D, post1 = everything after the lattice sum
GPIS_DEV float job1_coord(const DevModel &M, V3 p, V3 rayDir, float kss)
{
    V3 ray_dir_iso = normalized(cov_pos_w2l(M, rayDir, 1.0f));
    Frame coord = frame_from_normal(ray_dir_iso);
    V3 p_iso_ray = to_local(coord, cov_pos_w2l(M, p, kss));
    return p_iso_ray.z;
}
GPIS_DEV V4 post1(const DevModel &M, const Realization &r, V3 p, V3 rayDir, float nv, float ng, float R, float kss, bool conditioning, float origin_ratio)
{
    float nf = cov_norm1d(M, p, M.impulse_density, R);
    nv /= nf; ng /= nf;
    float gsx = 0.f, gsy = 0.f;
    if (GPIS_FLAG_activate_conditioning(M) && conditioning) {
        V3 ray_dir_iso = normalized(cov_pos_w2l(M, rayDir, 1.0f));
        Frame coord = frame_from_normal(ray_dir_iso);
        V3 p_iso_ray = to_local(coord, cov_pos_w2l(M, p, kss));
        V3 o = coeff_origin(r.c);
        float osf = GPIS_FLAG_multi_res(M) ? origin_ratio : 1.0f;
        V3 origin_iso_ray = to_local(coord, cov_pos_w2l(M, o, kss));
        float d = p_iso_ray.z - origin_iso_ray.z;
        float cs = GPIS_FLAG_nonstationary(M) ? cov_splat_cov_1d(M, p, o) : 1.0f;
        float kv = se_cov1d_val(d, cs), kg = se_cov1d_grad(d, cs), k2 = se_cov2d_2nd(d, cs);
        float vs_v = r.c.value_scale * kv, vs_g = r.c.value_scale * kg;
        float kz = kss * r.c.gradient_scale[2];
        float gz_v = kz * kg, gz_g = kz * k2;
        nv += osf * (vs_v + gz_v);
        ng += osf * (vs_g + gz_g);
        if (M.correlation_xy) {
            float kn = se_cov2d_2nd_normal(d, cs);
            gsx = osf * kss * r.c.gradient_scale[0] * kn;
            gsy = osf * kss * r.c.gradient_scale[1] * kn;
        }
    }
    return v4(nv, gsx, gsy, ng);
}
GPIS_DEV V4 eval_noise1d_normalized(const DevModel &M, const Realization &r, V3 p, V3 rayDir, uint32_t seed, int addseed, float R, float kss,
                                    bool conditioning, float origin_ratio)
{
    float nv, ng;
    noise1d(M, p, job1_coord(M, p, rayDir, kss), seed + (uint32_t)addseed, R, nv, ng);
    return post1(M, r, p, rayDir, nv, ng, R, kss, conditioning, origin_ratio);
}
// origin_scale_factor of SCN.cpp:338-342 for both levels
GPIS_DEV void origin_ratios(const DevModel &M, const Realization &r, bool conditioning, float &lo, float &hi)
{
    lo = hi = 1.0f;
    if (GPIS_FLAG_multi_res(M) && GPIS_FLAG_activate_conditioning(M) && conditioning) {
        LevelInfo O = kernel_scale_level_ratio(M, coeff_origin(r.c));
        lo = O.ratio_lo; hi = O.ratio_hi;
    }
}
// evaluateValueNoise1D, SCN.cpp:126-135
GPIS_DEV float eval_value_noise1d(const DevModel &M, Realization &r, V3 p, V3 rayDir, uint32_t seed, bool conditioning)
{
    r.n_eval++;
    float R = cov_kernel_radius(M, true, 1.0f);
    if (!GPIS_FLAG_multi_res(M))
        return eval_noise1d_normalized(M, r, p, rayDir, seed, 0, R, 1.0f, conditioning, 1.0f).v;
    LevelInfo L = kernel_scale_level_ratio(M, p);
    float olo, ohi;
    origin_ratios(M, r, conditioning, olo, ohi);
    float lo = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_lo, R, L.lo, conditioning, olo).v;
    float hi = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_hi, R, L.hi, conditioning, ohi).v;
    return L.ratio_lo * lo + L.ratio_hi * hi;
}
GPIS_DEV uint64_t xy_reseed(const RayInfo &info)
{
    return (uint64_t)(uint32_t)(xxhash32_4(info.px, info.py, info.spp, info.seg) + xxhash32_1(info.scene_seed) + 1u);
}
// evaluateGradientNoise1D, SCN.cpp:137-239: `bl` (and `bh` when multi-resolution) are the evaluateNoise1DNormalized
// results of the level(s); everything after them (the xy draws, the frames, the blend) is gradient_noise1d_finish
GPIS_DEV V3 gradient_noise1d_finish(const DevModel &M, V3 p, float tSegment, V3 rayDir, const RayInfo &info, const LevelInfo &L, V4 bl, V4 bh)
{
    float scaleX = cov_splat_cov_1d(M, p, p), scaleY = cov_splat_cov_1d(M, p, p);
    double xs0 = 1.0 / (double)scaleX, xs1 = 1.0 / (double)scaleY;
    const double div = (double)sqrtf(2.f);
    bool plus_xy = (M.ctx == GPIS_CTX_RENEWAL_PLUS && M.correlation_xy);
    Pcg32 s;
    if (!GPIS_FLAG_multi_res(M)) {
        V4 base = bl;
        V3 gbase = v3(base.gx, base.gy, base.gz);
        s.set_state(xy_reseed(info));
        double a, b;
        rand_normal_2(s, a, b);
        double x1 = a / div, y1 = b / div;
        V3 g;
        if (tSegment == 0) {
            g = v3((float)(x1 * xs0), (float)(y1 * xs1), 0.f) + gbase;
        } else if (!plus_xy) {
            double c, d;
            rand_normal_2(s, c, d);
            g = v3((float)(c / div * xs0), (float)(d / div * xs1), 0.f) + gbase;
        } else {
            float factor = (float)(exp_glibc((double)(-tSegment * tSegment) / 4.0) * (0.5 - (double)(tSegment * tSegment) * 0.25));
            double mux = (double)factor * 2.0 * x1, muy = (double)factor * 2.0 * y1;
            float cov = (float)(0.5 - (double)(factor * factor * 2));
            double c, d;
            rand_normal_2(s, c, d);
            double sc = (double)sqrtf(cov);
            g = v3((float)(c * sc + mux), (float)(d * sc + muy), 0.f) + gbase;
        }
        V3 ray_dir_iso = normalized(cov_pos_w2l(M, rayDir, 1.0f));
        Frame coord = frame_from_normal(ray_dir_iso);
        return cov_grad_l2w(M, to_global(coord, g), 1.0f);
    }
    V3 glb = v3(bl.gx, bl.gy, bl.gz), ghb = v3(bh.gx, bh.gy, bh.gz);
    s.set_state(xy_reseed(info));
    double al, bl2, ah, bh2;
    rand_normal_2(s, al, bl2);
    rand_normal_2(s, ah, bh2);
    double x1l = al / div, y1l = bl2 / div, x1h = ah / div, y1h = bh2 / div;
    V3 gl, gh;
    if (tSegment == 0) {
        gl = v3((float)(x1l * xs0), (float)(y1l * xs1), 0.f) + glb;
        gh = v3((float)(x1h * xs0), (float)(y1h * xs1), 0.f) + ghb;
    } else if (!plus_xy) {
        double cl, dl, ch, dh;
        rand_normal_2(s, cl, dl);
        rand_normal_2(s, ch, dh);
        gl = v3((float)(cl / div * xs0), (float)(dl / div * xs1), 0.f) + glb;
        gh = v3((float)(ch / div * xs0), (float)(dh / div * xs1), 0.f) + ghb;
    } else {
        float factor = (float)(exp_glibc((double)(-tSegment * tSegment) / 4.0) * (0.5 - (double)(tSegment * tSegment) * 0.25));
        float cov = (float)(0.5 - (double)(factor * factor * 2));
        double sc = (double)sqrtf(cov);
        double cl, dl, ch, dh;
        rand_normal_2(s, cl, dl);
        rand_normal_2(s, ch, dh);
        gl = v3((float)(cl * sc + (double)factor * 2.0 * x1l), (float)(dl * sc + (double)factor * 2.0 * y1l), 0.f) + glb;
        gh = v3((float)(ch * sc + (double)factor * 2.0 * x1h), (float)(dh * sc + (double)factor * 2.0 * y1h), 0.f) + ghb;
    }
    Frame cl_ = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, L.lo)));
    Frame ch_ = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, L.hi)));
    V3 gwl = cov_grad_l2w(M, to_global(cl_, gl), L.lo);
    V3 gwh = cov_grad_l2w(M, to_global(ch_, gh), L.hi);
    return gwl * L.ratio_lo + gwh * L.ratio_hi;
}
GPIS_DEV V3 eval_gradient_noise1d(const DevModel &M, Realization &r, V3 p, float tSegment, V3 rayDir, const RayInfo &info, bool conditioning)
{
    uint32_t seed = compute_seed(M, info);
    r.n_eval++;
    float R = cov_kernel_radius(M, true, 1.0f);
    LevelInfo L{};
    if (!GPIS_FLAG_multi_res(M)) {
        V4 base = eval_noise1d_normalized(M, r, p, rayDir, seed, 0, R, 1.0f, conditioning, 1.0f);
        return gradient_noise1d_finish(M, p, tSegment, rayDir, info, L, base, base);
    }
    L = kernel_scale_level_ratio(M, p);
    float olo, ohi;
    origin_ratios(M, r, conditioning, olo, ohi);
    V4 bl = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_lo, R, L.lo, conditioning, olo);
    V4 bh = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_hi, R, L.hi, conditioning, ohi);
    return gradient_noise1d_finish(M, p, tSegment, rayDir, info, L, bl, bh);
}

// sparseConvNoiseAmplitude(p): GPF.cpp:611-613, 711 (stationary) / 1235-1237 (getVariance(p) * sigma, GPF.cpp:1638-1641)
GPIS_DEV float cov_amplitude(const DevModel &M, V3 p)
{
    if (GPIS_FLAG_fbm_noise(M) && M.grid.on) {
        const V3d pd = to_d(p);
        return (float)(grid_variance(M.grid, pd.x, pd.y, pd.z) * (double)M.sigma_raw);   // GPF.cpp:1235-1237 over 1393-1403
    }
    if (!GPIS_FLAG_nonstationary(M) || !M.var.enabled)
        return M.sigma;
    return (float)(field_scalar(M.var, to_d(p), GPIS_FLAG_fbm_noise(M)) * (double)M.sigma_raw);
}

// In the all-features instance the three evaluator entries are out-of-line functions too (GPIS_PATH_EVAL: the march reaches them
// from nine sites); the specialised instances inline them.
#ifdef GPIS_PATH_OUTLINE_NOISE3D
#define GPIS_PATH_EVAL static __device__ __attribute__((noinline))
#else
#define GPIS_PATH_EVAL GPIS_DEV
#endif
// evaluateValue, SCN.cpp:73-89
GPIS_PATH_EVAL float evaluate_value(const DevModel &M, Realization &r, V3 p, V3 rayDir, const RayInfo &info, int &gp_id)
{
    uint32_t seed = compute_seed(M, info);
    float noise_val = GPIS_FLAG_sampling_1d(M) ? eval_value_noise1d(M, r, p, rayDir, seed, true) : eval_noise3d(M, r, p, rayDir, seed, true).v;
    double mean;
    int id;
    path_mean_weight_space(M, to_d(p), mean, id);
    gp_id = id;
    if (M.surf_vol_phase_separate) {          // getUnscaledVariance = 1 (GPF.hpp:1185) except in the grid flavour (GPF.cpp:1386-1391)
        float uv = 1.f;
        if (GPIS_FLAG_fbm_noise(M) && M.grid.on) { const V3d pd = to_d(p); uv = grid_unscaled_variance(M.grid, pd.x, pd.y, pd.z); }
        gp_id = (uv < M.surf_vol_phase_amp_thresh) ? 0 : 1;
    }
    return (float)((double)(cov_amplitude(M, p) * noise_val) + mean);
}
// evaluateGradient, SCN.cpp:92-99
GPIS_PATH_EVAL V3 evaluate_gradient(const DevModel &M, Realization &r, V3 p, float t, V3 rayDir, const RayInfo &info)
{
    uint32_t seed = compute_seed(M, info);
    V3 ng;
    if (GPIS_FLAG_sampling_1d(M)) {
        ng = eval_gradient_noise1d(M, r, p, t, rayDir, info, true);
    } else {
        V4 n = eval_noise3d(M, r, p, rayDir, seed, true);
        ng = v3(n.gx, n.gy, n.gz);
    }
    double mean;
    int id;
    path_mean_weight_space(M, to_d(p), mean, id);
    V3 mg = to_f(path_mean_grad(M, id, to_d(p)));
    return cov_amplitude(M, p) * ng + mg;
}

// conditioning, SCN.cpp:431-595, in three parts: conditioning_begin (resets the coefficients; false when no
// evaluation is needed), the unconditioned evaluation(s) at the segment start, and conditioning_finish3d / 1d
// (the coefficients).  The reference re-evaluates the conditioned field after each solve and discards the result
// (SCN.cpp:468-470, 516-519, 560-562, 590-592); those evaluations are COUNTED here (n_eval) but not computed.
GPIS_DEV bool conditioning_begin(const DevModel &M, Realization &r, V3 p)
{
    if (!GPIS_FLAG_activate_conditioning(M))
        return false;
    r.c.value_scale = 0.f;
    r.c.gradient_scale[0] = r.c.gradient_scale[1] = r.c.gradient_scale[2] = 0.f;
    r.c.ray_origin[0] = p.x; r.c.ray_origin[1] = p.y; r.c.ray_origin[2] = p.z;
    return cov_amplitude(M, p) != 0;
}
// c4 = evaluateNoise3D(p, conditioning = false) (value and gradient)
template <bool SDF_MEAN = false> GPIS_DEV void conditioning_finish3d(const DevModel &M, Realization &r, V3 p, V3 rayDir, float targetVal, V3 targetGrad, V4 c4)
{
    LevelInfo K{};
    if (GPIS_FLAG_multi_res(M))
        K = kernel_scale_level_ratio(M, p);
    float amplitude = cov_amplitude(M, p);
    double mean_d;
    int id;
    cond_mean_weight_space<SDF_MEAN>(M, to_d(p), mean_d, id);
    float mean = (float)mean_d;
    const bool plus = M.ctx == GPIS_CTX_RENEWAL_PLUS;
    float cur = c4.v;
    r.c.value_scale = (targetVal - mean) / amplitude - cur;
    if (GPIS_FLAG_multi_res(M))
        r.c.value_scale /= K.ratio_lo + K.ratio_hi;
    r.n_eval++;                       // the discarded re-evaluation
    if (plus) {
        V3 mg = to_f(cond_mean_grad<SDF_MEAN>(M, id, to_d(p)));
        r.n_eval++;                   // the reference evaluates the unconditioned field a second time: same value
        V3 delta = (targetGrad - mg) / amplitude - v3(c4.gx, c4.gy, c4.gz);
        float S[9];
        V3 g;
        if (M.iso3d) {
            Frame coord = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, 1.0f)));
            V3 gi = to_local(coord, cov_grad_w2l(M, delta, 1.0f));
            cov_one_over_second_derivative(M, p, true, S);
            g = eig_matvec(S, gi);
            if (GPIS_FLAG_multi_res(M)) {
                g = g / (K.ratio_lo / K.lo + K.ratio_hi / K.hi);
            } else {
                float q = cov_ns_scale(M, p);
                g = g * (q * q);
            }
        } else {
            cov_one_over_second_derivative(M, p, false, S);
            g = eig_matvec(S, delta);
            if (GPIS_FLAG_multi_res(M)) {
                g = g / (K.ratio_lo / (K.lo * K.lo) + K.ratio_hi / (K.hi * K.hi));
            } else {
                float q = cov_lateral_scale(M, p);
                g = g * (q * q);
            }
        }
        r.c.gradient_scale[0] = g.x; r.c.gradient_scale[1] = g.y; r.c.gradient_scale[2] = g.z;
        r.n_eval++;
    }
}
// bl / bh = evaluateNoise1DNormalized(p, conditioning = false) of the level(s) (bh = bl when not multi-resolution)
template <bool SDF_MEAN = false> GPIS_DEV void conditioning_finish1d(const DevModel &M, Realization &r, V3 p, V3 rayDir, float targetVal, V3 targetGrad, const RayInfo &info, V4 bl, V4 bh)
{
    LevelInfo K{};
    if (GPIS_FLAG_multi_res(M))
        K = kernel_scale_level_ratio(M, p);
    float amplitude = cov_amplitude(M, p);
    double mean_d;
    int id;
    cond_mean_weight_space<SDF_MEAN>(M, to_d(p), mean_d, id);
    float mean = (float)mean_d;
    const bool plus = M.ctx == GPIS_CTX_RENEWAL_PLUS;
    float cur = GPIS_FLAG_multi_res(M) ? K.ratio_lo * bl.v + K.ratio_hi * bh.v : bl.v;
    r.c.value_scale = (targetVal - mean) / amplitude - cur;
    if (GPIS_FLAG_multi_res(M))
        r.c.value_scale /= K.ratio_lo * K.ratio_lo + K.ratio_hi * K.ratio_hi;
    r.n_eval++;
    if (plus) {
        V3 mg = to_f(cond_mean_grad<SDF_MEAN>(M, id, to_d(p)));
        r.n_eval++;
        V3 cgw = gradient_noise1d_finish(M, p, 0.f, rayDir, info, K, bl, bh);
        V3 delta = (targetGrad - mg) / amplitude - cgw;
        Frame coord = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, 1.0f)));
        V3 gi = to_local(coord, cov_grad_w2l(M, delta, 1.0f));
        float sX = cov_splat_cov_1d(M, p, p), sY = sX, sZ = sX;
        V3 g = v3((-2.f * gi.x) * (sX * sX), (-2.f * gi.y) * (sY * sY), (-2.f * gi.z) * (sZ * sZ));
        if (GPIS_FLAG_multi_res(M))
            g = g / (K.ratio_lo * K.ratio_lo + K.ratio_hi * K.ratio_hi);
        if (!M.correlation_xy) { g.x = 0; g.y = 0; }
        r.c.gradient_scale[0] = g.x; r.c.gradient_scale[1] = g.y; r.c.gradient_scale[2] = g.z;
        r.n_eval++;
    }
}
GPIS_PATH_EVAL void conditioning(const DevModel &M, Realization &r, V3 p, V3 rayDir, float targetVal, V3 targetGrad, const RayInfo &info)
{
    if (!conditioning_begin(M, r, p))
        return;
    uint32_t seed = compute_seed(M, info);
    if (GPIS_FLAG_sampling_1d(M)) {
        r.n_eval++;
        float R = cov_kernel_radius(M, true, 1.0f);
        V4 bl, bh;
        if (!GPIS_FLAG_multi_res(M)) {
            bl = bh = eval_noise1d_normalized(M, r, p, rayDir, seed, 0, R, 1.0f, false, 1.0f);
        } else {
            LevelInfo L = kernel_scale_level_ratio(M, p);
            bl = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_lo, R, L.lo, false, 1.0f);
            bh = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_hi, R, L.hi, false, 1.0f);
        }
        conditioning_finish1d<true>(M, r, p, rayDir, targetVal, targetGrad, info, bl, bh);
        return;
    }
    V4 c4 = eval_noise3d(M, r, p, rayDir, seed, false);
    conditioning_finish3d<true>(M, r, p, rayDir, targetVal, targetGrad, c4);
}

// neeShared / neeGrad / neePDF, SCN.cpp:601-743
GPIS_DEV void nee_shared(const DevModel &M, Realization &r, V3 rayDir, V3 normal, V3 p, const RayInfo &info, NeeShared &o)
{
    uint32_t seed = compute_seed(M, info);
    float amplitude = cov_amplitude(M, p);
    double mean_d;
    int id;
    path_mean_weight_space(M, to_d(p), mean_d, id);
    V3 mg = to_f(path_mean_grad(M, id, to_d(p)));
    Frame coord = frame_from_normal(normalized(cov_pos_w2l(M, rayDir, 1.0f)));
    float rc[9] = {coord.tangent.x, coord.bitangent.x, coord.normal.x,
                   coord.tangent.y, coord.bitangent.y, coord.normal.y,
                   coord.tangent.z, coord.bitangent.z, coord.normal.z};
    float scale = 1.f;
    if (GPIS_FLAG_nonstationary(M))
        scale = (float)(GPIS_FLAG_multi_resolution_grid(M) ? 1.0 : (double)M.ls_maxval);
    float sa[9], mtx[9], inv[9];
    for (int i = 0; i < 9; ++i) {
        float w = GPIS_FLAG_nonstationary(M) ? M.w2l_T[i] / scale : M.w2l_T[i];
        sa[i] = amplitude * w;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            GM(mtx, a, b) = sum3e(GM(sa, a, 0) * GM(rc, 0, b), GM(sa, a, 1) * GM(rc, 1, b), GM(sa, a, 2) * GM(rc, 2, b));
    eig_inverse3(mtx, inv);
    r.n_eval++;
    float R = cov_kernel_radius(M, true, 1.0f);
    if (!GPIS_FLAG_multi_res(M)) {
        V4 n = eval_noise1d_normalized(M, r, p, rayDir, seed, 0, R, 1.0f, true, 1.0f);
        o.grad_constraint_3d = v3(n.gx, n.gy, n.gz);
    } else {
        LevelInfo L = kernel_scale_level_ratio(M, p);
        float olo, ohi;
        origin_ratios(M, r, true, olo, ohi);
        V4 lo = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_lo, R, L.lo, true, olo);
        V4 hi = eval_noise1d_normalized(M, r, p, rayDir, seed, L.add_hi, R, L.hi, true, ohi);
        o.grad_constraint_3d = (v3(lo.gx, lo.gy, lo.gz) * L.ratio_lo) / L.lo + (v3(hi.gx, hi.gy, hi.gz) * L.ratio_hi) / L.hi;
    }
    V3 plane_pt = mult3(mtx, v3(0.f, 0.f, o.grad_constraint_3d.z)) + mg;
    V3 cp = cross(mult3(mtx, v3(1.f, 0.f, 0.f)), mult3(mtx, v3(0.f, 1.f, 0.f)));
    o.plane_normal_world = normalized(cp);
    o.plane_stretch_jacobian = length(cp);
    o.isect_dist = dot(plane_pt, o.plane_normal_world) / dot(normal, o.plane_normal_world);
    o.grad_3d_iso_ray = mult3(inv, o.isect_dist * normal - mg);
}
GPIS_DEV V3 nee_grad(const DevModel &M, Realization &r, V3 rayDir, V3 normal, V3 p, const RayInfo &info)
{
    NeeShared s;
    nee_shared(M, r, rayDir, normal, p, info, s);
    return s.isect_dist * normal;
}
GPIS_DEV float nee_pdf(const DevModel &M, Realization &r, V3 rayDir, V3 normal, V3 p, float tSegment, const RayInfo &info)
{
    NeeShared s;
    nee_shared(M, r, rayDir, normal, p, info, s);
    if ((double)s.isect_dist < 0.0)
        return 0.0f;
    float scaleX = cov_splat_cov_1d(M, p, p), scaleY = scaleX;
    float sample_x, sample_y, pdf_area;
    bool plus_xy = (M.ctx == GPIS_CTX_RENEWAL_PLUS && M.correlation_xy);
    const double div = (double)sqrtf(2.f);
    const double kSqrt2 = 1.4142135623730951, kPi = 3.14159265358979323846;
    float dxg = s.grad_3d_iso_ray.x - s.grad_constraint_3d.x, dyg = s.grad_3d_iso_ray.y - s.grad_constraint_3d.y;
    Pcg32 ps;
    if (!GPIS_FLAG_multi_res(M)) {
        if (!plus_xy) {
            sample_x = (float)((double)dxg * kSqrt2 * (double)scaleX);
            sample_y = (float)((double)dyg * kSqrt2 * (double)scaleY);
            pdf_area = (float)(exp_glibc((double)(-sample_x * sample_x) / 2.0) * exp_glibc((double)(-sample_y * sample_y) / 2.0) / (2.0 * kPi) * 2.0 * (double)scaleX * (double)scaleY);
        } else {
            ps.set_state(xy_reseed(info));
            double a, b;
            rand_normal_2(ps, a, b);
            double x1 = a / div, y1 = b / div;
            float factor = (float)(exp_glibc((double)(-tSegment * tSegment) / 4.0) * (0.5 - (double)(tSegment * tSegment) * 0.25));
            double mux = (double)factor * 2.0 * x1, muy = (double)factor * 2.0 * y1;
            float cov = (float)(0.5 - (double)(factor * factor * 2));
            double sc = (double)sqrtf(cov);
            sample_x = (float)(((double)dxg - mux) / sc);
            sample_y = (float)(((double)dyg - muy) / sc);
            pdf_area = (float)(exp_glibc((double)(-sample_x * sample_x) / 2.0) * exp_glibc((double)(-sample_y * sample_y) / 2.0) / (2.0 * kPi) / (double)cov);
        }
    } else {
        LevelInfo L = kernel_scale_level_ratio(M, p);
        float q0 = L.ratio_lo / L.lo, q1 = L.ratio_hi / L.hi;
        float nss = (float)(1.0 / (double)sqrtf(q0 * q0 + q1 * q1));
        scaleX *= nss; scaleY *= nss;
        if (!plus_xy) {
            sample_x = (float)((double)dxg * kSqrt2 * (double)scaleX);
            sample_y = (float)((double)dyg * kSqrt2 * (double)scaleY);
            pdf_area = (float)(exp_glibc((double)(-sample_x * sample_x) / 2.0) * exp_glibc((double)(-sample_y * sample_y) / 2.0) / (2.0 * kPi) * 2.0 * (double)scaleX * (double)scaleY);
        } else {
            ps.set_state(xy_reseed(info));
            double a, b, c, d;
            rand_normal_2(ps, a, b);
            rand_normal_2(ps, c, d);
            double x1 = a / div, y1 = b / div, x2 = c / div, y2 = d / div;
            float factor = (float)(exp_glibc((double)(-tSegment * tSegment) / 4.0) * (0.5 - (double)(tSegment * tSegment) * 0.25));
            double mux = (double)factor * 2.0 * (x1 * (double)L.ratio_lo / (double)L.lo + x2 * (double)L.ratio_hi / (double)L.hi);
            double muy = (double)factor * 2.0 * (y1 * (double)L.ratio_lo / (double)L.lo + y2 * (double)L.ratio_hi / (double)L.hi);
            float cov = (float)(0.5 - (double)(factor * factor * 2));
            double sc = (double)sqrtf(cov);
            sample_x = (float)(((double)dxg - mux) / sc * (double)nss);
            sample_y = (float)(((double)dyg - muy) / sc * (double)nss);
            pdf_area = (float)(exp_glibc((double)(-sample_x * sample_x) / 2.0) * exp_glibc((double)(-sample_y * sample_y) / 2.0) / (2.0 * kPi * (double)cov) * (double)(nss * nss));
        }
    }
    float cosl = fabsf(dot(normal, s.plane_normal_world));
    float pdf_normal = pdf_area * (s.isect_dist * s.isect_dist) / cosl / s.plane_stretch_jacobian;
    return (float)((double)pdf_normal / (4.0 * (double)dot(normal, v3(-rayDir.x, -rayDir.y, -rayDir.z))));
}

// ---- medium level (SCNM.cpp:102-183, GPM.cpp:221-393) -------------------------------------

// intersectGP, SCNM.cpp:102-183
GPIS_DEV bool intersect_gp(const DevModel &M, Realization &noise, V3 pos, V3 dir, float nearT, float farT, float u, MediumState &st, double &t_out)
{
    V3d rd = to_d(dir), p = to_d(pos);
    float step_size = (farT - nearT) / (float)M.min_step;
    if (M.step_size < step_size)
        step_size = M.step_size;
    int gp = 0;
    double t = (double)nearT;
    if (!st.first_scatter)
        conditioning(M, noise, to_f(p), dir, (float)(double)st.last_val, to_f(st.last_aniso), st.info);
    double f0 = (double)evaluate_value(M, noise, to_f(ray_at(p, rd, t)), dir, st.info, gp);
    int sign0 = f0 < 0 ? -1 : 1;
    double pf = f0;
    t = (double)(nearT + step_size * u);
    int step = 0;
    while (t < (double)farT) {
        step++;
        double f_c = (double)evaluate_value(M, noise, to_f(ray_at(p, rd, t)), dir, st.info, gp);
        int signc = f_c < 0 ? -1 : 1;
        if (!st.first_scatter && step == 1) {
            sign0 = signc;
        } else if (signc != sign0) {
            double intp = pf / (pf - f_c);
            double a = t - (double)step_size;
            double t_test, t_prev = lerp_d(a, t, intp);
            for (;;) {
                t_test = lerp_d(a, t, intp);
                double f_test = (double)evaluate_value(M, noise, to_f(ray_at(p, rd, t_test)), dir, st.info, gp);
                int sign_test = f_test < 0 ? -1 : 1;
                if (sign_test == sign0)
                    break;
                intp *= 0.9;
                if (intp <= 0.01) {
                    t_prev = t_test = 0;
                    break;
                }
                t_prev = t_test;
            }
            t = t_prev;
            st.last_gp_id = gp;
            st.scheme = cov_amplitude(M, to_f(ray_at(p, rd, t))) < 1e-6f ? GPIS_UNI : M.scheme_1d_eff;   // samplingScheme(p + t*rd), SCN.cpp:51-58, SCNM.cpp:164
            st.last_val = 0.0f;
            t_out = t;
            return true;
        }
        pf = f_c;
        t += (double)step_size;
    }
    t = (double)farT;
    st.scheme = GPIS_UNI;
    st.last_val = evaluate_value(M, noise, to_f(ray_at(p, rd, t)), dir, st.info, gp);
    t_out = t;
    return false;
}

// GaussianProcessMedium::transmittance, GPM.cpp:343-393
GPIS_DEV bool transmittance_one(const DevModel &M, Realization &noise, const gpis_ray_in &ray, MediumState &st)
{
    V3 pos = v3(ray.pos[0], ray.pos[1], ray.pos[2]), dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
    double startT = (double)ray.near_t;
    float farT = ray.far_t;
    if (!__builtin_isfinite(farT))
        farT = (float)(startT + 2000);
    float maxT = farT;
    double t = (double)maxT;
    V3d ro = to_d(pos), rd = to_d(dir);
    { double inv = 1.0 / length_d(rd); rd.x *= inv; rd.y *= inv; rd.z *= inv; }
    bool exited;
    do {
        exited = !intersect_gp(M, noise, pos, dir, (float)startT, farT, ray.u_jitter, st, t);
        if (t < (double)maxT) {
            V3 g = evaluate_gradient(M, noise, to_f(ray_at(ro, rd, t)), (float)t, dir, st.info);
            st.last_aniso = to_d(g);
            st.first_scatter = false;
            double avg = ((double)g.x + (double)g.y + (double)g.z) / 3.0;
            if (!__builtin_isfinite(avg))
                return false;
        }
        startT = t;
    } while (t < (double)maxT && exited);
    return exited;
}

// GaussianProcessMedium::sampleDistance, GPM.cpp:221-341
GPIS_DEV void sample_distance_one(const DevModel &M, Realization &noise, const gpis_ray_in &ray, gpis_seg_out &out)
{
    MediumState st;
    state_from_ray(ray, st);
    V3 pos = v3(ray.pos[0], ray.pos[1], ray.pos[2]), dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
    double startT = (double)ray.near_t;
    float farT = ray.far_t;
    if (!__builtin_isfinite(farT))
        farT = (float)(startT + 2000);
    float maxT = farT;
    out.t = 0.;
    out.sample_t = 0.f; out.continued_t = 0.f;
    for (int c = 0; c < 3; ++c) { out.weight[c] = 0.f; out.continued_weight[c] = 0.f; out.p[c] = 0.f; }
    out.exited = 0; out.ok = 0; out.scheme = GPIS_UNI;
    out.gp_id = st.last_gp_id;
    out.last_val = st.last_val;
    out.aniso[0] = st.last_aniso.x; out.aniso[1] = st.last_aniso.y; out.aniso[2] = st.last_aniso.z;
    if (st.bounce >= M.max_bounces)
        return;
    if (maxT == 0.f) {
        out.weight[0] = out.weight[1] = out.weight[2] = 1.f;
        out.exited = 1;
        V3 pp = pos + dir * out.sample_t;
        out.p[0] = pp.x; out.p[1] = pp.y; out.p[2] = pp.z;
        out.ok = 1;
        return;
    }
    V3d aniso = st.last_aniso;
    if (M.absorption_only) {
        if (maxT == __builtin_huge_valf())
            return;
        out.sample_t = maxT;
        bool vis = transmittance_one(M, noise, ray, st);
        out.weight[0] = out.weight[1] = out.weight[2] = vis ? 1.f : 0.f;
        out.exited = 1;
        aniso = st.last_aniso;
    } else {
        double t = (double)maxT;
        V3d ro = to_d(pos), rd = to_d(dir);
        { double inv = 1.0 / length_d(rd); rd.x *= inv; rd.y *= inv; rd.z *= inv; }
        bool exited;
        do {
            exited = !intersect_gp(M, noise, pos, dir, (float)startT, farT, ray.u_jitter, st, t);
            if (t < (double)maxT) {
                V3 g = evaluate_gradient(M, noise, to_f(ray_at(ro, rd, t)), (float)t, dir, st.info);
                aniso = to_d(g);
                st.last_aniso = aniso;
                st.first_scatter = false;
                double avg = (aniso.x + aniso.y + aniso.z) / 3.0;
                if (!__builtin_isfinite(avg)) {
                    out.aniso[0] = 1.; out.aniso[1] = 0.; out.aniso[2] = 0.;
                    out.t = t; out.exited = exited ? 1 : 0;
                    out.last_val = st.last_val; out.gp_id = st.last_gp_id;
                    return;
                }
            }
            startT = t;
        } while (t < (double)maxT && exited);
        out.t = t;
        out.exited = exited ? 1 : 0;
        if (!exited) {
            double d = aniso.x * (double)dir.x; d += aniso.y * (double)dir.y; d += aniso.z * (double)dir.z;
            double l2 = 0.; l2 += aniso.x * aniso.x; l2 += aniso.y * aniso.y; l2 += aniso.z * aniso.z;
            bool wrong_side = d > 0;
            bool zero_grad = !wrong_side && l2 < (double)0.0000001f;
            if (wrong_side || zero_grad) {
                if (zero_grad) aniso = V3d{1., 0., 0.};
                out.aniso[0] = aniso.x; out.aniso[1] = aniso.y; out.aniso[2] = aniso.z;
                out.last_val = st.last_val; out.gp_id = st.last_gp_id;
                return;
            }
        } else {
            aniso = to_d(evaluate_gradient(M, noise, to_f(ray_at(ro, rd, t)), (float)t, dir, st.info));
        }
        float ft = (float)t;
        out.sample_t = ft < maxT ? ft : maxT;
        out.continued_t = ft;
        double col[3] = {1., 1., 1.};
        if (!exited && M.color.enabled) field_vec(M.color, path_color_point(M, ray_at(ro, rd, t)), GPIS_FLAG_fbm_noise(M), col);   // color(ro + rd*t), GPM.cpp:316
        for (int c = 0; c < 3; ++c) {
            out.weight[c] = (float)col[c] * M.sigma_s_over_t[c];
            out.continued_weight[c] = (float)col[c] * M.sigma_s_over_t[c];
        }
        st.last_aniso = aniso;
        out.scheme = st.scheme;
    }
    V3 pp = pos + dir * out.sample_t;
    out.p[0] = pp.x; out.p[1] = pp.y; out.p[2] = pp.z;
    out.aniso[0] = aniso.x; out.aniso[1] = aniso.y; out.aniso[2] = aniso.z;
    out.gp_id = st.last_gp_id;
    out.last_val = st.last_val;
    out.ok = 1;
}


// entry points of this instance for the march kernels
struct Path {
    static GPIS_DEV void sample_distance(const DevModel &M, Realization &noise, const gpis_ray_in &ray, gpis_seg_out &out)
    {
        sample_distance_one(M, noise, ray, out);
    }
    static GPIS_DEV bool transmittance(const DevModel &M, Realization &noise, const gpis_ray_in &ray, MediumState &st)
    {
        return transmittance_one(M, noise, ray, st);
    }
    static GPIS_DEV float nee_pdf_of(const DevModel &M, Realization &r, V3 rayDir, V3 normal, V3 p, float tSegment, const RayInfo &info)
    {
        return nee_pdf(M, r, rayDir, normal, p, tSegment, info);
    }
    static GPIS_DEV V3 nee_grad_of(const DevModel &M, Realization &r, V3 rayDir, V3 normal, V3 p, const RayInfo &info)
    {
        return nee_grad(M, r, rayDir, normal, p, info);
    }
};

}   // namespace GPIS_PATH_NS
}   // namespace gpis

#include "gpis_persist.inc"

#undef GPIS_PATH_NS
#undef GPIS_FLAG_fbm_noise
#undef GPIS_FLAG_sdf_mean
#undef GPIS_PATH_OUTLINE_NOISE3D
#undef GPIS_PATH_EVAL
#undef GPIS_FLAG_other_kernels
#undef GPIS_FLAG_aniso_field
#undef GPIS_FLAG_sampling_1d
#undef GPIS_FLAG_multi_res
#undef GPIS_FLAG_nonstationary
#undef GPIS_FLAG_multi_resolution_grid
#undef GPIS_FLAG_activate_conditioning
