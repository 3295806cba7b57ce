// gpis_hip.hip — C ABI (include/gpis.h) of the MI355X sparse-convolution GPIS path: the model build, the handle, the batch and
// *_host entries, the guide and profiling entries.  The staged scene-S frame drivers are tu_scene.hip; both share gpis_host.hpp.
// Errors, owning buffers and the round trip of a *_host entry: gpis_host_base.hpp (shared with the weight-space units).
// Build (see __graft_entry__.build): every .hip of this directory for gfx950, -O3 -ffp-contract=off, linked into libgpis_hip.so.
//
// Layout in HBM: rays and results are arrays of the 128-/96-byte PODs of gpis.h (a wave reads
// 64 consecutive records = 8 KiB / 6 KiB contiguous); the medium's constants live in one
// DevModel block read through scalar loads; counters are two 64-bit words updated once per wave.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "gpis.h"
#include "gpis_host.hpp"      // gpis_medium, ProfScope; HIP_TRY, CHECK_ARGS, DevBuf (gpis_host_base.hpp); gpis_tables.hpp (FastTable, fast_supported, fast_table_free,
                              // GuideField, kBrickFloats, guide_free) — none of the fast or guided device code is seen here
#include "gpis_launch.hpp"    // the march kernels live in the tu_*.hip translation units
#include "gpis_nn_mean.hpp"   // the exact evaluator of a neural SDF mean: k_mean over a network (this unit only)

#pragma clang fp contract(off)

using namespace gpis;
using gpis::launch::grid_of;

// ======================================================================================
// errors: the one definition of the text both handle families report through (gpis_host_base.hpp)
// ======================================================================================
static thread_local char g_err[512] = "";

int gpis::set_err(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *gpis_last_error(void) { return g_err; }

// ---- shared with the weight-space medium's translation unit (tu_ws.hip) ----
namespace gpis {
int ws_destroy(gpis_medium *m);
// a weight-space handle starts with kWsHandleTag where a gpis_medium holds params.abi_version (GPIS_ABI_VERSION)
bool ws_is_handle(const void *m)
{
    uint32_t w = 0;
    if (m) memcpy(&w, m, sizeof w);
    return w == 0x57534D31u;
}
}   // namespace gpis
bool gpis::std_handle(const gpis_medium *m) { return m && !gpis::ws_is_handle(m); }

int gpis::ensure_stage(gpis_medium *m, int slot, size_t bytes, bool exact)
{
    std::lock_guard<std::mutex> lock(m->stage_mu[slot]);
    HIP_TRY(m->stage[slot].grow(bytes, !exact));     // exact: whole-frame workspaces (tens of GB; allocation time is per byte)
    return GPIS_OK;
}
size_t gpis::stage_size(gpis_medium *m, int slot)
{
    std::lock_guard<std::mutex> lock(m->stage_mu[slot]);
    return m->stage[slot].bytes;
}
// the *_host round trip (gpis_host_base.hpp) on this handle's lock and staging slots 0..2
template <typename Call>
static int host_trip(gpis_medium *m, std::initializer_list<HostArray> arrays, Call call)
{
    return host_round_trip(m->mu, m->device, m->stage, [m](int slot, size_t bytes) { return ensure_stage(m, slot, bytes); }, arrays, call);
}

// ======================================================================================
// host-side "fromJson": precompute the constants the reference computes once
// (GPF.cpp:654-679, 696-709, 741-760; SCN.cpp:8-37; GPM.cpp:152-158)
// ======================================================================================
static inline float hsum3e(float a, float b, float c) { return a + (b + c); }
#define HM(m, r, c) ((m)[3 * (r) + (c)])
static float hcof(const float *m, int i, int j)
{
    int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return HM(m, i1, j1) * HM(m, i2, j2) - HM(m, i1, j2) * HM(m, i2, j1);
}
static void hinverse3(const float *m, float *r)
{
    float c0 = hcof(m, 0, 0), c1 = hcof(m, 1, 0), c2 = hcof(m, 2, 0);
    float det = hsum3e(c0 * HM(m, 0, 0), c1 * HM(m, 1, 0), c2 * HM(m, 2, 0));
    float invdet = 1.0f / det;
    HM(r, 1, 0) = hcof(m, 0, 1) * invdet; HM(r, 1, 1) = hcof(m, 1, 1) * invdet; HM(r, 2, 0) = hcof(m, 0, 2) * invdet;
    HM(r, 1, 2) = hcof(m, 2, 1) * invdet; HM(r, 2, 1) = hcof(m, 1, 2) * invdet; HM(r, 2, 2) = hcof(m, 2, 2) * invdet;
    HM(r, 0, 0) = c0 * invdet; HM(r, 0, 1) = c1 * invdet; HM(r, 0, 2) = c2 * invdet;
}
static float hdet3(const float *m)
{
    auto h = [&](int a, int b, int c) { return HM(m, 0, a) * (HM(m, 1, b) * HM(m, 2, c) - HM(m, 1, c) * HM(m, 2, b)); };
    return h(0, 1, 2) - h(1, 0, 2) + h(2, 0, 1);
}

static int build_model(const gpis_params &P, DevModel &M, gpis_derived &D)
{
    memset(&M, 0, sizeof M);
    memset(&D, 0, sizeof D);
    M.single_realization = P.single_realization != 0;
    M.iso3d = P.isotropic_3d_sampling != 0;
    M.sampling_1d = P.sampling_1d != 0;
    M.correlation_xy = P.correlation_xy != 0;
    M.ctx = P.correlation_context;
    M.activate_conditioning = !M.single_realization && (M.ctx == GPIS_CTX_RENEWAL || M.ctx == GPIS_CTX_RENEWAL_PLUS);
    M.scheme_1d_eff = (!M.single_realization && M.sampling_1d) ? P.scheme_1d : GPIS_UNI;
    M.nonstationary = P.nonstationary != 0;
    M.multi_resolution_grid = P.multi_resolution_grid != 0;
    M.multi_res = M.nonstationary && M.multi_resolution_grid;
    M.use_aniso_mtx = P.use_aniso_mtx != 0;
    M.surf_vol_phase_separate = P.surf_vol_phase_separate != 0;
    M.surf_vol_phase_amp_thresh = P.surf_vol_phase_amp_thresh;
    M.has_mean_additional = P.has_mean_additional != 0;
    M.max_bounces = P.max_bounces;
    M.seed = P.seed;
    M.n_impulses = (uint32_t)P.impulse_density;
    M.min_step = P.min_step;
    M.step_size = P.step_size;
    M.impulse_density = P.impulse_density;
    M.sigma = M.nonstationary ? (float)(1.0 * (double)P.sigma) : P.sigma;
    M.sigma_raw = P.sigma;

    // SquaredExponentialCovariance::fromJson
    float l_conv = P.length_scale * sqrtf(2.f) / 2;
    float l2w[9] = {0}, w2l[9] = {0};
    float l_aniso[3] = {0, 0, 0};
    if (!M.use_aniso_mtx) {
        for (int i = 0; i < 3; ++i) {
            l_aniso[i] = l_conv * P.aniso[i];
            float inv = 1.0f / l_aniso[i];
            if (std::isinf(inv) || std::isnan(inv)) inv = 0;
            HM(l2w, i, i) = l_aniso[i];
            HM(w2l, i, i) = inv;
            HM(M.invcov_world, i, i) = inv * inv;
        }
        M.cov_det_sqrt_world = (double)(l_aniso[0] * l_aniso[1] * l_aniso[2]);
        float a = l_aniso[0] > l_aniso[1] ? l_aniso[0] : l_aniso[1];
        M.mtx_factor = a > l_aniso[2] ? a : l_aniso[2];
    } else {
        for (int i = 0; i < 9; ++i) l2w[i] = l_conv * P.aniso_mtx[i];
        hinverse3(l2w, w2l);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                HM(M.invcov_world, r, c) = hsum3e(HM(w2l, 0, r) * HM(w2l, 0, c), HM(w2l, 1, r) * HM(w2l, 1, c), HM(w2l, 2, r) * HM(w2l, 2, c));
        float det = hdet3(M.invcov_world);
        M.cov_det_sqrt_world = 1.0 / (double)sqrtf(det);
        float e0 = (HM(l2w, 0, 0) + HM(l2w, 0, 1)) + HM(l2w, 0, 2);
        float e1 = (HM(l2w, 1, 0) + HM(l2w, 1, 1)) + HM(l2w, 1, 2);
        float e2 = (HM(l2w, 2, 0) + HM(l2w, 2, 1)) + HM(l2w, 2, 2);
        float a = e0 > e1 ? e0 : e1;
        M.mtx_factor = a > e2 ? a : e2;
    }
    memcpy(M.w2l, w2l, sizeof w2l);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            HM(M.w2l_T, r, c) = HM(w2l, c, r);
            HM(M.l2w_T, r, c) = HM(l2w, c, r);
        }
    M.kernel_scale = P.local_scale;
    M.pi_pow_1_5 = pow(M_PI, 1.5);
    M.sqrt_pi = sqrt(M_PI);

    // ramp + multi-resolution tables (host libm so that they equal the reference's values)
    M.ls_ramp_type = P.ls_ramp_type;
    M.ls_min = P.ls_min; M.ls_max = P.ls_max;
    M.ls_scale = 1.0 / (P.ls_end - P.ls_start);
    M.ls_offset = -P.ls_start * M.ls_scale;
    { double mn = P.ls_min + 1., mx = P.ls_max + 1.; M.ls_log_min2 = log(mn * mn); M.ls_log_max2 = log(mx * mx); }
    M.ls_maxval = (float)(P.ls_max > P.ls_min ? P.ls_max : P.ls_min);
    // the procedural fields in their general form (host libm for the logs, as the reference computes them per call)
    auto make_ramp = [](int enabled, int type, double mn, double mx, double st, double en, double mn2, double mx2, double st2, double en2) {
        DevRamp R;
        memset(&R, 0, sizeof R);
        R.enabled = enabled; R.type = type;
        R.scale = 1.0 / (en - st); R.offset = -st * R.scale;
        R.scale2 = 1.0 / (en2 - st2); R.offset2 = -st2 * R.scale2;
        const double a = mn + 1., b = mx + 1., a2 = mn2 + 1., b2 = mx2 + 1.;
        R.log_min2 = log(a * a); R.log_max2 = log(b * b);
        R.log2_min2 = log(a2 * a2); R.log2_max2 = log(b2 * b2);
        R.vmin = mn; R.vmax = mx;
        return R;
    };
    M.ls = make_ramp(M.nonstationary, P.ls_ramp_type, P.ls_min, P.ls_max, P.ls_start, P.ls_end, P.ls_min2, P.ls_max2, P.ls_start2, P.ls_end2);
    M.var = make_ramp(P.var.enabled != 0, P.var.type, P.var.min, P.var.max, P.var.start, P.var.end, P.var.min2, P.var.max2, P.var.start2, P.var.end2);
    M.aniso = make_ramp(P.aniso_field.enabled != 0, P.aniso_field.type, P.aniso_field.min, P.aniso_field.max, P.aniso_field.start, P.aniso_field.end,
                        P.aniso_field.min2, P.aniso_field.max2, P.aniso_field.start2, P.aniso_field.end2);
    M.color = make_ramp(P.mean_color.enabled != 0, P.mean_color.type, P.mean_color.min, P.mean_color.max, P.mean_color.start, P.mean_color.end,
                        P.mean_color.min2, P.mean_color.max2, P.mean_color.start2, P.mean_color.end2);
    M.emission = make_ramp(P.mean_emission.enabled != 0, P.mean_emission.type, P.mean_emission.min, P.mean_emission.max, P.mean_emission.start, P.mean_emission.end,
                           P.mean_emission.min2, P.mean_emission.max2, P.mean_emission.start2, P.mean_emission.end2);
    if (P.ls_ramp_type == GPIS_RAMP_BOTTOM_TOP_LEFT_RIGHT)      // ProceduralNoiseVec::maxVal, GPF.cpp:124-138
        M.ls_maxval = (float)((P.ls_max > P.ls_min ? P.ls_max : P.ls_min) * (P.ls_max2 > P.ls_min2 ? P.ls_max2 : P.ls_min2));
    if (P.ls_ramp_type == GPIS_NOISE_SANDSTONE || P.ls_ramp_type == GPIS_NOISE_RUST)
        M.ls_maxval = 1.f;
    {   // sandstone / rust anywhere: the launcher routes the medium to the all-features path instance (gpis_device.hpp: GPIS_FLAG_fbm_noise)
        const DevRamp *fields[5] = {&M.ls, &M.var, &M.aniso, &M.color, &M.emission};
        M.fbm_noise = 0;
        for (const DevRamp *f : fields)
            if (f->enabled && f->type >= GPIS_NOISE_SANDSTONE) M.fbm_noise = 1;
    }
    {   // GridNonstationaryCovariance (GPF.cpp:1326-1427): variance and kernel scale from a voxel grid (gpis_set_variance_grid)
        memset(&M.grid, 0, sizeof M.grid);
        M.grid.on = P.grid_nonstationary != 0;
        M.grid.offset = P.grid_offset; M.grid.scale = P.grid_scale;
        M.grid.separate = P.grid_surf_vol_amp_separate != 0;
        M.grid.thresh = P.grid_surf_vol_amp_thresh;
        M.grid.surf_amp = P.grid_surf_amp_scale; M.grid.vol_amp = P.grid_vol_amp_scale;
        M.grid.surf_ls = P.grid_surf_ls_scale; M.grid.vol_ls = P.grid_vol_ls_scale;
        if (M.grid.on) {
            M.fbm_noise = 1;                                     // all-features path instance
            M.ls.enabled = 0;
            // sparseConvNoiseMaxLateralScale, GPF.cpp:1422-1427
            M.ls_maxval = M.grid.separate ? (P.grid_surf_ls_scale < P.grid_vol_ls_scale ? P.grid_vol_ls_scale : P.grid_surf_ls_scale) : 1.f;
        }
    }
    const float base = 2.5f;
    M.log_base = logf(base);
    for (int l = kLevelMin; l <= kLevelMax; ++l) {
        float sc = powf(base, (float)l);
        M.level_scale[l - kLevelMin] = sc;
        M.level_addseed[l - kLevelMin] = (int)floorf(logf(sc) / logf(base));
    }
    float wss = M.nonstationary ? M.ls_maxval : 1.f;
    M.world_addseed = (int)floorf(logf(wss) / logf(base));

    // stationary constants
    auto variance3d = [&](float dens, float R, bool isIdentity, float globalScale, float localScale) {
        double idua = dens / (R * R * R);
        double cds = 1.0;
        if (!isIdentity) {
            cds = M.cov_det_sqrt_world;
            cds *= pow(globalScale, 3);
        }
        cds *= pow(localScale, 3);
        return (float)(idua * (M.pi_pow_1_5 * cds));
    };
    M.radius_iso = M.kernel_scale;
    M.radius_world = M.kernel_scale * 1.0f * M.mtx_factor;
    M.norm3d_world = sqrtf(variance3d(P.impulse_density, M.radius_world, false, 1.0f, 1.0f));
    {   // bound on ab^T A ab inside the unit ball, for the grid space the cooperative kernels use (A as in coop_eval_noise3d)
        const float amax = M.iso3d ? 0.5f : 0.5f * fmaxf(M.invcov_world[0], fmaxf(M.invcov_world[4], M.invcov_world[8]));
        const float R = M.iso3d ? M.kernel_scale : M.radius_world;
        const float v = amax * R * R * 1.01f;
        M.exp_arg_max = (v == v && v >= 0.f) ? v : 3.4e38f;
    }
    M.norm3d_iso = sqrtf(variance3d(P.impulse_density, M.radius_iso, true, 1.0f, 1.0f));
    // Matérn / Gabor kernels: their own radius and variance (GPF.cpp:1020-1046, 1127-1138, 1192-1203); host libm as the reference
    M.kernel_type = P.kernel_type;
    M.matern_v = P.matern_v;
    M.k_l = P.length_scale;
    M.fs_n = P.fs_sample_points;
    M.fs_step = P.fs_step_size;
    for (int i = 0; i < 3; ++i) M.fs_aniso[i] = P.aniso[i];
    M.gabor_a = (float)(1.0 / P.gabor_a_inv);
    M.gabor_f = (float)(1.0 / P.gabor_f_inv);
    {
        float l2 = 0.f; l2 += P.gabor_omega[0] * P.gabor_omega[0]; l2 += P.gabor_omega[1] * P.gabor_omega[1]; l2 += P.gabor_omega[2] * P.gabor_omega[2];
        const float inv = 1.0f / sqrtf(l2);
        for (int i = 0; i < 3; ++i) M.gabor_omega[i] = P.gabor_omega[i] * inv;
    }
    if (P.kernel_type != GPIS_KERNEL_SQUARED_EXPONENTIAL) {
        const float l = P.length_scale, a = M.gabor_a, f = M.gabor_f;
        double iks;
        if (P.kernel_type == GPIS_KERNEL_MATERN) {
            float la[3];
            for (int i = 0; i < 3; ++i) {
                la[i] = l / sqrtf(P.aniso[i]);
                if (std::isinf(la[i]) || std::isnan(la[i])) la[i] = 0;
            }
            float mx = la[0] > la[1] ? la[0] : la[1];
            mx = mx > la[2] ? mx : la[2];
            M.radius_world = (float)(M.kernel_scale * 1.0f * sqrt(2) / 2 * mx);
            iks = P.matern_v == 0.5 ? 2.0 * M_PI * l : (P.matern_v == 1.5 ? pow(M_PI * l, 3) / (24 * sqrt(3)) : M_PI * pow(l, 3) / (5 * sqrt(5)));      // GPF.cpp:1029-1046
        } else if (P.kernel_type == GPIS_KERNEL_GABOR_ANISO) {
            M.radius_world = (float)(M.kernel_scale * sqrt(2) / 2 * 1.0 / a);
            const float q = f / a;
            iks = pow(1.0 / a, 3) * (1 + exp(-2.0 * M_PI * (q * q))) / (4 * sqrt(2));
        } else {
            M.radius_world = (float)(M.kernel_scale * sqrt(2) / 4 * 1.0 / a);
            iks = 2 * sqrt(2) * M_PI * (f * f) / a * (1 - exp(-2 * M_PI * f / (a * a)));
        }
        const float R = M.radius_world;
        const double idua = P.impulse_density / (R * R * R);
        M.norm3d_world = sqrtf((float)(idua * iks));
        M.radius_iso = M.kernel_scale;      // splattingKernelRadius(true, .) of these kernels; unused (world space only)
    }
    {
        double idua = P.impulse_density / M.radius_iso;
        M.norm1d = sqrtf((float)(idua * (M.sqrt_pi * 1.0f)));
    }
    // prepareForRender
    bool all_zero = true;
    for (int c = 0; c < 3; ++c) {
        float sa = P.sigma_a[c] * P.density, ss = P.sigma_s[c] * P.density;
        float st = sa + ss;
        M.sigma_s_over_t[c] = ss / st;
        if (ss != 0.0f) all_zero = false;
    }
    M.absorption_only = all_zero;
    M.mean[0] = P.mean;
    M.mean[1] = P.mean_additional;
    for (int w = 0; w < 2; ++w) {
        const gpis_mean &mu = M.mean[w];
        double l2 = 0.; l2 += mu.dir[0] * mu.dir[0]; l2 += mu.dir[1] * mu.dir[1]; l2 += mu.dir[2] * mu.dir[2];
        double len = sqrt(l2);
        double inv = len > 0 ? 1.0 / len : 0.0;
        for (int k = 0; k < 3; ++k) M.lin_dir[w][k] = mu.dir[k] * inv;
    }
    {   // procedural SDF means (gpis_sdf.hpp): the three Mat4f::rotAxis((1,0,0), angle) of SdfFunctions.cpp, Mat4f.cpp:132-148 with the host libm
        auto out_of_line = [](const gpis_mean &mu) { return mu.type == GPIS_MEAN_PROCEDURAL || mu.type == GPIS_MEAN_TABULATED; };
        M.sdf_mean = out_of_line(M.mean[0]) || (M.has_mean_additional && out_of_line(M.mean[1]));
        const float angles[3] = {-90.f, 90.f, -45.f};
        for (int r = 0; r < 3; ++r) {
            const float angle = angles[r] * (3.1415926536f / 180.0f);      // Angle::degToRad
            const float s = std::sin(angle), c = std::cos(angle), c1 = 1.0f - c;
            const float x = 1.f, y = 0.f, z = 0.f;
            const float R[9] = {c + x * x * c1, x * y * c1 - z * s, x * z * c1 + y * s,
                                y * x * c1 + z * s, c + y * y * c1, y * z * c1 - x * s,
                                z * x * c1 - y * s, z * y * c1 + x * s, c + z * z * c1};
            memcpy(M.sdf_rot[r], R, sizeof R);
        }
        for (int w = 0; w < 2; ++w)
            for (int i = 0; i < 12; ++i) M.sdf_inv[w][i] = (i % 5 == 0) ? 1.f : 0.f;       // Mat4f(): the identity
    }
    {   // tabulated means (gpis_grid_mean.hpp): no grid yet (gpis_set_mean_grid); "volume" travels in gpis_mean.func
        for (int w = 0; w < 2; ++w)
            M.mean_volume[w] = M.mean[w].type == GPIS_MEAN_TABULATED && M.mean[w].func != 0;
        // TabulatedMean::emission (GPF.cpp:174-177) is the grid's, 0 without an emission grid, and GaussianProcess::emission asks the
        // primary mean (GaussianProcess.hpp:258-260): such a medium emits nothing whatever its "emission" field says
        if (M.mean[0].type == GPIS_MEAN_TABULATED) M.emission.enabled = 0;
    }

    memcpy(D.world_to_local, w2l, sizeof w2l);
    memcpy(D.local_to_world, l2w, sizeof l2w);
    if (!M.nonstationary) {
        D.kernel_radius_world = M.radius_world;
        D.kernel_radius_iso = M.radius_iso;
        D.norm3d_world = M.norm3d_world;
        D.norm3d_iso = M.norm3d_iso;
        D.norm1d = M.norm1d;
    } else {
        float ls = (float)((double)1.0f * (M.multi_resolution_grid ? 1.0 : (double)M.ls_maxval));
        ls *= M.aniso.enabled ? 1.5f : 1.f;          // sparseConvNoiseMaxAnisotropyScale(), GPF.cpp:1743-1747
        D.kernel_radius_world = M.kernel_scale * ls * M.mtx_factor;
        D.kernel_radius_iso = M.kernel_scale;
        D.norm3d_world = 0.f; D.norm3d_iso = 0.f; D.norm1d = 0.f;   // position dependent: not constants of the medium
    }
    D.impulses_per_cell = M.n_impulses;
    D.activate_conditioning = M.activate_conditioning;
    D.effective_scheme_1d = M.scheme_1d_eff;
    D.multi_resolution = M.multi_res;
    return GPIS_OK;
}
// the model part a weight-space medium shares (means, colour, medium coefficients; tu_ws.hip)
namespace gpis {
int host_build_model(const gpis_params &P, DevModel &M)
{
    gpis_derived D;
    return build_model(P, M, D);
}
}   // namespace gpis

// MeanFunction::color / emission at double-precision points (GPF.hpp:849-857; ramp noises: three equal components)
__global__ void __launch_bounds__(256) k_mean_color_emission(const DevModel *__restrict__ Mp, size_t n, const double *__restrict__ p3,
                                                             float *__restrict__ color3, float *__restrict__ emission3)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevModel &M = *Mp;
    const V3d p{p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]};
    if (color3) {
        double c[3] = {1., 1., 1.};
        if (M.color.enabled) field_vec(M.color, sdf::color_point(M, p), true, c);      // ProceduralMean::color: at T^-1 . Vec3f(p)
        for (int k = 0; k < 3; ++k) color3[3 * i + k] = (float)c[k];
    }
    if (emission3) {
        double e[3] = {0., 0., 0.};
        if (M.emission.enabled) field_vec(M.emission, p, true, e);
        for (int k = 0; k < 3; ++k) emission3[3 * i + k] = (float)e[k];
    }
}
// GaussianProcess::mean_weight_space at double-precision points: value, chosen slot, dmean_da of that slot (any mean type)
__global__ void __launch_bounds__(256) k_mean(const DevModel *__restrict__ Mp, size_t n, const double *__restrict__ p3, double *__restrict__ value,
                                              int32_t *__restrict__ id, double *__restrict__ grad3)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const sdf::MeanId r = sdf::mean_weight_space(Mp, p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]);
    if (value) value[i] = r.mean;
    if (id) id[i] = r.id;
    if (grad3) {
        const V3d g = sdf::mean_grad(Mp, r.id, p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]);
        grad3[3 * i] = g.x; grad3[3 * i + 1] = g.y; grad3[3 * i + 2] = g.z;
    }
}
__global__ void k_xxhash32(size_t n, int arity, const uint32_t *__restrict__ w, uint32_t *__restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *p = w + i * (size_t)arity;
    out[i] = arity == 1 ? xxhash32_1(p[0]) : arity == 2 ? xxhash32_2(p[0], p[1]) : arity == 3 ? xxhash32_3(p[0], p[1], p[2]) : xxhash32_4(p[0], p[1], p[2], p[3]);
}
__global__ void k_pcg32_stream(size_t n, const uint64_t *__restrict__ state, uint32_t count, uint32_t *__restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pcg32 s;
    s.set_state(state[i]);
    for (uint32_t k = 0; k < count; ++k)
        out[i * (size_t)count + k] = s.next_i();
}

// ======================================================================================
// C ABI
// ======================================================================================

extern "C" const char *gpis_abi_sizes(void)
{
    static char buf[768];
    snprintf(buf, sizeof buf,
             "gpis_params=%zu,gpis_mean=%zu,gpis_ray_in=%zu,gpis_seg_out=%zu,gpis_cond_coeff=%zu,gpis_query=%zu,"
             "gpis_nee_query=%zu,gpis_derived=%zu,gpis_scene_s=%zu,gpis_surface_s=%zu,gpis_ramp=%zu,gpis_fs_state=%zu,gpis_guide_info=%zu,"
             "gpis_ws_params=%zu,gpis_ws_query=%zu,gpis_adaptive_s=%zu,gpis_adaptive_record=%zu,gpis_adaptive_info=%zu,gpis_mean_network=%zu,"
             "gpis_surface_rgb_s=%zu,gpis_material_rgb=%zu,gpis_materials_s=%zu",
             sizeof(gpis_params), sizeof(gpis_mean), sizeof(gpis_ray_in), sizeof(gpis_seg_out), sizeof(gpis_cond_coeff),
             sizeof(gpis_query), sizeof(gpis_nee_query), sizeof(gpis_derived), sizeof(gpis_scene_s), sizeof(gpis_surface_s), sizeof(gpis_ramp), sizeof(gpis_fs_state), sizeof(gpis_guide_info),
             sizeof(gpis_ws_params), sizeof(gpis_ws_query), sizeof(gpis_adaptive_s), sizeof(gpis_adaptive_record), sizeof(gpis_adaptive_info), sizeof(gpis_mean_network),
             sizeof(gpis_surface_rgb_s), sizeof(gpis_material_rgb), sizeof(gpis_materials_s));
    return buf;
}

extern "C" void gpis_default_params(gpis_params *p)
{
    memset(p, 0, sizeof *p);
    p->abi_version = GPIS_ABI_VERSION;
    p->step_size = 0.01f; p->min_step = 8; p->seed = 0; p->impulse_density = 3.0f;
    p->scheme_1d = GPIS_UNI;
    p->correlation_context = GPIS_CTX_RENEWAL_PLUS;
    p->max_bounces = 1024;
    p->density = 1.f;
    p->sigma = 1.f; p->length_scale = 1.f;
    p->aniso[0] = p->aniso[1] = p->aniso[2] = 1.f;
    p->aniso_mtx[0] = p->aniso_mtx[4] = p->aniso_mtx[8] = 1.f;
    p->local_scale = 3.0f;
    p->ls_min = 1.; p->ls_max = 500.; p->ls_start = 0.; p->ls_end = 1.;
    p->ls_min2 = 1.; p->ls_max2 = 500.; p->ls_start2 = 0.; p->ls_end2 = 1.;          // GPF.hpp:694-699
    p->matern_v = 0.5f; p->gabor_a_inv = 1.f; p->gabor_f_inv = 1.f; p->gabor_omega[0] = 1.f;   // GPF.hpp:1964, 2041, 2079
    p->fs_sample_points = 32; p->fs_step_size = 0.;                                  // FunctionSpace...cpp:24-26
    p->grid_scale = 1.f; p->grid_surf_vol_amp_thresh = 1.f;                          // GPF.hpp:2327-2335
    p->grid_surf_amp_scale = p->grid_vol_amp_scale = p->grid_surf_ls_scale = p->grid_vol_ls_scale = 1.f;
    gpis_ramp *ramps[4] = {&p->var, &p->mean_color, &p->mean_emission, &p->aniso_field};
    for (gpis_ramp *r : ramps) { r->min = 1.; r->max = 500.; r->start = 0.; r->end = 1.; r->min2 = 1.; r->max2 = 500.; r->start2 = 0.; r->end2 = 1.; }
    p->mean.type = GPIS_MEAN_SPHERICAL; p->mean.radius = 1.f;
    p->mean.scale = 1.f; p->mean.min = -FLT_MAX; p->mean.dir[0] = 1.;
    p->mean_additional = p->mean;
}

extern "C" int gpis_create(const gpis_params *params, int device, gpis_medium **out)
{
    if (!params || !out) return set_err(GPIS_ERR_INVALID_ARG, "gpis_create: null argument");
    if (params->abi_version != GPIS_ABI_VERSION) return set_err(GPIS_ERR_INVALID_ARG, "gpis_create: abi_version %u != %d", params->abi_version, GPIS_ABI_VERSION);
    // same failure points as the reference's JSON parsing (GPM.cpp:40, SCNM.cpp:44)
    if (params->correlation_context < 0 || params->correlation_context > 3) return set_err(GPIS_ERR_INVALID_ARG, "Invalid correlation context: '%d'", params->correlation_context);
    if (params->scheme_1d < 0 || params->scheme_1d > 2) return set_err(GPIS_ERR_INVALID_ARG, "Invalid sparse conv sampling scheme: '%d'", params->scheme_1d);
    if (!(params->impulse_density >= 0.f) || params->impulse_density > 4096.f) return set_err(GPIS_ERR_INVALID_ARG, "impulse_density out of range");
    if (params->mean.type < 0 || params->mean.type > GPIS_MEAN_TABULATED ||
        (params->has_mean_additional && (params->mean_additional.type < 0 || params->mean_additional.type > GPIS_MEAN_TABULATED)))
        return set_err(GPIS_ERR_INVALID_ARG, "invalid mean type");
    for (int w = 0; w < (params->has_mean_additional ? 2 : 1); ++w) {
        const gpis_mean &mu = w ? params->mean_additional : params->mean;
        if (mu.type == GPIS_MEAN_PROCEDURAL && (mu.func < GPIS_SDF_KNOB || mu.func > GPIS_SDF_PLANE))
            return set_err(GPIS_ERR_INVALID_ARG, "Invalid sdf function: '%d' (procedural mean, slot %d)", mu.func, w);
    }
    if (params->nonstationary && (params->ls_ramp_type < 0 || params->ls_ramp_type > GPIS_NOISE_RUST)) return set_err(GPIS_ERR_INVALID_ARG, "invalid ls noise type");
    {
        const gpis_ramp *ramps[3] = {&params->var, &params->mean_color, &params->mean_emission};
        for (const gpis_ramp *r : ramps)
            if (r->enabled && (r->type < 0 || r->type > GPIS_NOISE_RUST)) return set_err(GPIS_ERR_INVALID_ARG, "invalid procedural noise type");
        if (params->var.enabled && !params->nonstationary) return set_err(GPIS_ERR_INVALID_ARG, "a \"var\" field needs the proc_nonstationary wrapper");
        if (params->aniso_field.enabled) {
            if (params->aniso_field.type < 0 || params->aniso_field.type > GPIS_NOISE_RUST) return set_err(GPIS_ERR_INVALID_ARG, "invalid procedural noise type");
            if (!params->nonstationary) return set_err(GPIS_ERR_INVALID_ARG, "an \"aniso\" field needs the proc_nonstationary wrapper");
            if (params->sampling_1d) return set_err(GPIS_ERR_INVALID_ARG, "an \"aniso\" field is built for 3D sampling only (GPF.cpp:1691-1727 are outside the built scope)");
        }
    }
    if (params->grid_nonstationary && (!params->nonstationary || params->var.enabled || params->aniso_field.enabled))
        return set_err(GPIS_ERR_INVALID_ARG, "the grid flavour of the non-stationary wrapper needs nonstationary = 1 and carries no var / aniso field");
    if (params->kernel_type < 0 || params->kernel_type > 3) return set_err(GPIS_ERR_INVALID_ARG, "invalid kernel type");
    if (params->kernel_type != GPIS_KERNEL_SQUARED_EXPONENTIAL) {
        if (params->kernel_type == GPIS_KERNEL_MATERN && params->matern_v != 0.5f && params->matern_v != 1.5f && params->matern_v != 2.5f)
            return set_err(GPIS_ERR_UNSUPPORTED, "Matern kernel only implemented for v = 0.5, 1.5, 2.5! (GPF.cpp:1000)");
        if (params->isotropic_3d_sampling || params->sampling_1d || params->nonstationary || params->correlation_context == GPIS_CTX_RENEWAL_PLUS)
            return set_err(GPIS_ERR_UNSUPPORTED, "Matern / Gabor kernels: world-space 3D sampling with correlation context none / global / renewal only "
                                                 "(they define no isotropic transform, 1D kernel or second derivative, GPF.hpp:2002-2110)");
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_err(GPIS_ERR_NO_DEVICE, "gpis_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= count) return set_err(GPIS_ERR_INVALID_ARG, "gpis_create: device %d out of range (%d devices)", device, count);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return set_err(GPIS_ERR_NO_DEVICE, "gpis_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
    gpis_medium *m = new (std::nothrow) gpis_medium();
    if (!m) return set_err(GPIS_ERR_DEVICE, "out of host memory");
    m->params = *params;       // every other member starts from its initialiser (gpis_host.hpp)
    m->device = device;
    m->n_cus = prop.multiProcessorCount;
    {   // diagnostic overrides, read here and nowhere else (include/gpis.h: gpis_set_option)
        m->opt[GPIS_OPT_MARCH_FORM] = GPIS_MARCH_FORM_AUTO;
        if (const char *e = getenv("GPIS_MARCH")) {
            if (strcmp(e, "resident") == 0) m->opt[GPIS_OPT_MARCH_FORM] = GPIS_MARCH_FORM_RESIDENT;
            else if (strcmp(e, "wave") == 0) m->opt[GPIS_OPT_MARCH_FORM] = GPIS_MARCH_FORM_WAVE;
        }
        m->opt[GPIS_OPT_WAVE_TAIL] = 262144;
        if (const char *e = getenv("GPIS_WAVE_TAIL")) m->opt[GPIS_OPT_WAVE_TAIL] = atoll(e) < 0 ? 0 : atoll(e);
        const char *e1 = getenv("GPIS_PATHS_SORT"), *e2 = getenv("GPIS_PATHS_PRESORT");
        m->opt[GPIS_OPT_PATHS_SORT] = !(e1 && e1[0] == '0');
        m->opt[GPIS_OPT_PATHS_PRESORT] = !(e2 && e2[0] == '0');
        m->opt[GPIS_OPT_PERSISTENT] = 1;
        if (const char *e = getenv("GPIS_PERSIST")) m->opt[GPIS_OPT_PERSISTENT] = e[0] != '0';
        m->opt[GPIS_OPT_RANGE_LEN] = 0;       // measured on C1: refill breaks the depth coherence the cooperative evaluator lives on
        if (const char *e = getenv("GPIS_RANGE_LEN")) { long long v = atoll(e); m->opt[GPIS_OPT_RANGE_LEN] = v <= 0 ? 0 : ((v + 63) / 64) * 64; }
        m->opt[GPIS_OPT_DEFER_GRAD] = 0;
        if (const char *e = getenv("GPIS_DEFER_GRAD")) m->opt[GPIS_OPT_DEFER_GRAD] = e[0] != '0';
        m->opt[GPIS_OPT_SOLO_MAX] = -1;
        if (const char *e = getenv("GPIS_SOLO_MAX")) m->opt[GPIS_OPT_SOLO_MAX] = atoll(e);
        m->opt[GPIS_OPT_SCENE_EXIT_STATE] = 0;
        if (const char *e = getenv("GPIS_SCENE_EXIT_STATE")) m->opt[GPIS_OPT_SCENE_EXIT_STATE] = e[0] != '0';
        m->opt[GPIS_OPT_SCENE_COMPACT] = 1;
        if (const char *e = getenv("GPIS_SCENE_COMPACT")) m->opt[GPIS_OPT_SCENE_COMPACT] = e[0] != '0';
        m->opt[GPIS_OPT_SHADOW_LEAN] = 1;
        if (const char *e = getenv("GPIS_SHADOW_LEAN")) m->opt[GPIS_OPT_SHADOW_LEAN] = e[0] != '0';
        m->opt[GPIS_OPT_CHUNK_LOG2] = 0;
        if (const char *e = getenv("GPIS_CHUNK_LOG2")) { int l = atoi(e); m->opt[GPIS_OPT_CHUNK_LOG2] = l < 16 ? 16 : (l > 28 ? 28 : l); }
    }
    int st = build_model(*params, m->host_model, m->derived);
    if (st != GPIS_OK) { delete m; return st; }
    hipError_t e = m->d_model.grow(sizeof(DevModel));
    if (e == hipSuccess) e = m->d_counters.grow(2 * sizeof(Counters));
    if (e == hipSuccess) e = m->d_guide_cnt.grow(8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(m->d_guide_cnt.p, 0, 8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = m->d_guide.grow(sizeof(GuideField));
    if (e == hipSuccess) e = hipMemset(m->d_guide.p, 0, sizeof(GuideField));
    if (e == hipSuccess) e = m->d_next.grow(kPersistSlots * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemcpy(m->d_model.p, &m->host_model, sizeof(DevModel), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(m->d_counters.p, 0, 2 * sizeof(Counters));
    if (e != hipSuccess) {
        set_err(GPIS_ERR_DEVICE, "gpis_create: %s", hipGetErrorString(e));
        delete m;
        return GPIS_ERR_DEVICE;
    }
    st = launch::fast_table_build(m->host_model, &m->fast);
    if (st != GPIS_OK) {
        set_err(st, "gpis_create: building the cell table failed");
        delete m;
        return st;
    }
    m->derived.fast_path = m->fast.enabled;
    *out = m;
    return GPIS_OK;
}

extern "C" int gpis_destroy(gpis_medium *m)
{
    if (!m) return GPIS_OK;
    if (gpis::ws_is_handle(m)) return gpis::ws_destroy(m);
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    delete m;
    return GPIS_OK;
}

extern "C" int gpis_get_derived(const gpis_medium *m, gpis_derived *out)
{
    if (!std_handle(m) || !out) return set_err(GPIS_ERR_INVALID_ARG, "null argument or not a sparse-convolution handle");
    *out = m->derived;
    return GPIS_OK;
}

int gpis::launch_check(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return set_err(GPIS_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
    return GPIS_OK;
}

// The guided march as a wavefront (gpis_wave.hpp): step → sort → eval until no ray requests a value,
// then (sampleDistance) one sorted gradient pass.  Synchronises the stream once per iteration to read the
// request count.  GPIS_MARCH=resident selects the one-kernel state machine instead.
// Which form runs: the caller's hint decides (MarchHint, gpis_host.hpp); GPIS_MARCH=wave|resident overrides it.
bool gpis::wave_march_selected(const gpis_medium *m, int hint)
{
    if (m->opt[GPIS_OPT_MARCH_FORM] == GPIS_MARCH_FORM_RESIDENT) return false;
    if (m->opt[GPIS_OPT_MARCH_FORM] == GPIS_MARCH_FORM_WAVE) return true;
    return hint == MARCH_SCATTERED;
}
// shared-workspace hand-over between callers on different streams (slot 0: stage[3], slot 1: stage[4])
int gpis::ws_acquire(gpis_medium *m, int slot, hipStream_t s)
{
    if (m->ws_event_set[slot])
        HIP_TRY(hipStreamWaitEvent(s, m->ws_event[slot], 0));
    return GPIS_OK;
}
int gpis::ws_release(gpis_medium *m, int slot, hipStream_t s)
{
    if (!m->ws_event[slot])
        HIP_TRY(hipEventCreateWithFlags(&m->ws_event[slot], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(m->ws_event[slot], s));
    m->ws_event_set[slot] = true;
    return GPIS_OK;
}
static int wave_march(gpis_medium *m, size_t n, const gpis_ray_in *rays, const uint8_t *mask, bool want_sample, gpis_seg_out *out,
                      gpis_cond_coeff *coeff, uint8_t *visible, hipStream_t s)
{
    if (n > 0x7FFFFFF0ull) return set_err(GPIS_ERR_INVALID_ARG, "wave march: batch too large (the radix sort takes an int count)");
    size_t temp_bytes = 0;
    if (sort_pairs_u32(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, n, s) != hipSuccess)
        return set_err(GPIS_ERR_DEVICE, "radix sort scratch query failed");
    size_t off = 0;
    const size_t o_cnt = ws_carve(off, 64), o_state = ws_carve(off, n * launch::wave_state_bytes()), o_k0 = ws_carve(off, n * 4),
                 o_v0 = ws_carve(off, n * 4), o_k1 = ws_carve(off, n * 4), o_v1 = ws_carve(off, n * 4), o_temp = ws_carve(off, temp_bytes);
    int rc = ensure_stage(m, 4, off);
    if (rc) return rc;
    if ((rc = ws_acquire(m, 1, s))) return rc;
    char *ws = (char *)m->stage[4].p;
    unsigned long long *d_req = (unsigned long long *)(ws + o_cnt);
    uint32_t *k0 = (uint32_t *)(ws + o_k0), *v0 = (uint32_t *)(ws + o_v0), *k1 = (uint32_t *)(ws + o_k1), *v1 = (uint32_t *)(ws + o_v1);
    const launch::WaveBufs wb{ws + o_state, k0, v0, k1, v1, d_req};
    const bool small_arg = m->host_model.exp_arg_max < 100.f;
    Counters *cnt = m->d_counters.p + (want_sample ? 0 : 1);
    auto read_requests = [&](size_t &n_req) -> int {
        unsigned long long h = 0;
        HIP_TRY(hipMemcpyAsync(&h, d_req, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemsetAsync(d_req, 0, sizeof h, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_req = (size_t)h;
        return GPIS_OK;
    };
    HIP_TRY(hipMemsetAsync(d_req, 0, sizeof(unsigned long long), s));
    const size_t tail_limit = (size_t)m->opt[GPIS_OPT_WAVE_TAIL];      // default 262144; measured on the multi-bounce driver: 16 Ki 55.9, 64 Ki 61.5, 256 Ki 65.0, 1 Mi 64.5 M paths/s
    size_t n_active = n;
    const uint32_t *active = nullptr;
    int init = 1;
    for (;;) {
        launch::wave_step(want_sample, m->d_model.p, m->guide, n_active, active, init, rays, mask, wb, m->d_guide_cnt.p, s);
        if ((rc = launch_check("k_wave_step"))) return rc;
        size_t n_req = 0;
        if ((rc = read_requests(n_req))) return rc;
        if (n_req == 0)
            break;
        size_t tb = temp_bytes;
        if (sort_pairs_u32(ws + o_temp, tb, k0, k1, v0, v1, n_active, s) != hipSuccess)
            return set_err(GPIS_ERR_DEVICE, "radix sort failed");
        launch::wave_eval(small_arg, m->d_model.p, m->fast, m->guide, n_req, v1, rays, wb, cnt, s);
        if ((rc = launch_check("k_wave_eval"))) return rc;
        active = v1;            // the sorted requesters are the rays still marching
        n_active = n_req;
        init = 0;
        if (n_active <= tail_limit) {
            // few rays left: one wave per ray runs them to the end of their value requests
            launch::wave_tail(want_sample, m->d_model.p, m->fast, m->guide, n_active, active, rays, wb, cnt, m->d_guide_cnt.p, s);
            if ((rc = launch_check("k_wave_tail"))) return rc;
            break;
        }
    }
    if (want_sample) {
        launch::wave_grad_keys(m->d_model.p, m->guide, n, rays, wb, s);
        if ((rc = launch_check("k_wave_grad_keys"))) return rc;
        size_t n_grad = 0;
        if ((rc = read_requests(n_grad))) return rc;
        if (n_grad) {
            size_t tb = temp_bytes;
            if (sort_pairs_u32(ws + o_temp, tb, k0, k1, v0, v1, n, s) != hipSuccess)
                return set_err(GPIS_ERR_DEVICE, "radix sort failed");
            launch::wave_grad(small_arg, m->d_model.p, m->fast, m->guide, n_grad, v1, rays, wb, cnt, s);
            if ((rc = launch_check("k_wave_grad"))) return rc;
        }
        launch::wave_finish_sd(m->d_model.p, n, rays, mask, wb, out, coeff, cnt, s);
        if ((rc = launch_check("k_wave_finish_sd"))) return rc;
        return ws_release(m, 1, s);
    }
    launch::wave_finish_tr(n, mask, wb, visible, cnt, s);
    if ((rc = launch_check("k_wave_finish_tr"))) return rc;
    return ws_release(m, 1, s);
}

// ---- persistent march launch (per-path media) ---------------------------------------------------------------
// the lattice sums of gpis_persist.inc have a diagonal kernel matrix: every medium except world-space 3D with a full anisoMtx
// (a procedural or tabulated mean is evaluated by the lane-per-ray all-features instance only: gpis_persist.inc states the analytic means inline)
static bool persist_supported(const DevModel &H) { return !H.aniso.enabled && !H.fbm_noise && !H.sdf_mean && (H.sampling_1d || H.iso3d || !H.use_aniso_mtx); }
// sideways (lane = impulse) evaluation pays while at most this many lanes of a wave have a job: lockstep costs
// 27 n g instructions per round whatever the number of jobs, one sideways job ~20.6 cells x (c0 + c1 n)
// (g = 61 generator, c0 = 135, c1 = 0.31: counted on the gfx950 ISA of these loops)
static int persist_solo_max(const gpis_medium *m)
{
    const DevModel &H = m->host_model;
    if (H.sampling_1d || H.n_impulses > 64u || H.n_impulses == 0u) return 0;     // the sideways form holds one cell's impulses in one wave
    if (m->opt[GPIS_OPT_SOLO_MAX] >= 0) return (int)m->opt[GPIS_OPT_SOLO_MAX];
    const double lock = 27.0 * H.n_impulses * 61.0, side = 20.6 * (135.0 + 0.31 * H.n_impulses);
    int t = (int)(lock / side);
    return t < 0 ? 0 : (t > 48 ? 48 : t);
}
template <bool WANT_SAMPLE>
static int launch_persist(gpis_medium *m, PersistArgs a, hipStream_t s)
{
    const DevModel &H = m->host_model;
    if (a.n >= 0xFFFF0000ull) return set_err(GPIS_ERR_INVALID_ARG, "persistent march: batch too large for the 32-bit ray counter");
    a.solo_max = persist_solo_max(m);
    int inst = launch::INST_GENERIC;
    if (H.fbm_noise) inst = launch::INST_GENERIC;          // sandstone / rust fields: all-features instance only
    else if (H.sampling_1d) inst = launch::INST_1D;
    else if (H.kernel_type != GPIS_KERNEL_SQUARED_EXPONENTIAL) inst = launch::INST_GENERIC;
    else if (!H.nonstationary && !H.multi_res && !H.multi_resolution_grid) inst = launch::INST_3D;
    else if (H.nonstationary && H.multi_res && H.multi_resolution_grid) inst = launch::INST_3D_MULTIRES;
    const int slot_id = (WANT_SAMPLE ? 0 : 4) + inst;
    if (m->persist_waves[slot_id] == 0) {
        int nb = launch::persist_blocks_per_cu(inst, WANT_SAMPLE);
        if (nb <= 0) nb = 8;
        m->persist_waves[slot_id] = nb * m->n_cus;
        if (getenv("GPIS_DEBUG")) fprintf(stderr, "gpis: persistent march instance %d (%s): %d resident waves per CU x %d CUs\n", inst, WANT_SAMPLE ? "sampleDistance" : "transmittance", nb, m->n_cus);
    }
    const size_t waves_needed = (a.n + kBlock - 1) / kBlock;
    const unsigned grid = (unsigned)(waves_needed < (size_t)m->persist_waves[slot_id] ? waves_needed : (size_t)m->persist_waves[slot_id]);
    a.next = m->d_next.p + (m->next_slot++ % kPersistSlots);
    HIP_TRY(hipMemsetAsync(a.next, 0, sizeof(unsigned int), s));
    launch::persist_march(inst, WANT_SAMPLE, grid, m->d_model.p, a, s);
    return launch_check("k_persist_march");
}
// neePDF / neeGrad: the 1D-sampling instance for the media the NEE estimators are built for, else the all-features one
int gpis::nee_instance(const DevModel &H) { return (H.sampling_1d && !H.fbm_noise && !H.sdf_mean) ? launch::INST_1D : launch::INST_GENERIC; }
// the lane-per-ray instance whose compile-time flags equal the medium's
static int lane_instance(const DevModel &H)
{
    if (H.fbm_noise || H.sdf_mean) return launch::INST_GENERIC;           // sandstone / rust fields, procedural / tabulated means: all-features instance only
    if (H.sampling_1d) return launch::INST_1D;
    if (!H.nonstationary && !H.multi_res && !H.multi_resolution_grid && H.kernel_type == GPIS_KERNEL_SQUARED_EXPONENTIAL) return launch::INST_3D;
    if (H.nonstationary && H.multi_res && H.multi_resolution_grid && !H.aniso.enabled) return launch::INST_3D_MULTIRES;
    return launch::INST_GENERIC;
}

int gpis::sample_distance_impl(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, gpis_cond_coeff *coeff,
                               const uint8_t *mask, hipStream_t s, int hint, bool exit_state)
{
    // exit_state = false (gpis_render_scene_s only): the caller reads nothing but ok / exited of a segment that left through farT, so the
    // resident guided march may skip lastVal and the gradient there (guided_march, EXIT_STATE); every other form evaluates them as ever
    if (n == 0) return GPIS_OK;
    ProfScope prof(m, 0, s);
    if (m->guide.enabled && wave_march_selected(m, hint))
        return wave_march(m, n, rays, mask, true, out, coeff, nullptr, s);
    if (m->guide.enabled && m->opt[GPIS_OPT_RANGE_LEN] > 0) {
        // guided march with in-wave refill (gpis_guide_range.hpp) + one coherent gradient pass
        launch::range_sample_distance(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->guide, n, rays, out, coeff, mask, m->d_counters.p, m->d_guide_cnt.p,
                                      (uint32_t)m->opt[GPIS_OPT_RANGE_LEN], s);
        return launch_check("k_guided_range_sd / k_guided_range_grad");
    }
    if (m->guide.enabled) {
        if (m->opt[GPIS_OPT_DEFER_GRAD]) {
            launch::guided_sample_distance_nograd(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->d_guide.p, n, rays, out, coeff, mask, m->d_counters.p, m->d_guide_cnt.p, s);
            int rc = launch_check("k_guided_sample_distance_nograd");
            if (rc) return rc;
            launch::range_grad(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->guide, n, rays, out, coeff, mask, m->d_counters.p, s);
            return launch_check("k_guided_range_grad");
        }
        if (!exit_state) {
            launch::guided_sample_distance_noexit(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->d_guide.p, n, rays, out, coeff, mask, m->d_counters.p, m->d_guide_cnt.p, s);
            return launch_check("k_guided_sample_distance_noexit");
        }
        launch::guided_sample_distance(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->d_guide.p, n, rays, out, coeff, mask, m->d_counters.p, m->d_guide_cnt.p, s);
        return launch_check("k_guided_sample_distance");
    }
    if (m->fast.enabled) {
        launch::fast_sample_distance(m->d_model.p, m->fast, n, rays, out, coeff, mask, m->d_counters.p, s);
        return launch_check("k_fast_sample_distance");
    }
    // pick the instance whose compile-time flags equal the medium's
    const DevModel &H = m->host_model;
    if (m->opt[GPIS_OPT_PERSISTENT] && persist_supported(H)) {
        PersistArgs a{};
        a.n = n; a.rays = rays; a.out = out; a.coeff = coeff; a.visible = nullptr; a.mask = mask; a.cnt = m->d_counters.p;
        return launch_persist<true>(m, a, s);
    }
    launch::lane_sample_distance(lane_instance(H), m->d_model.p, n, rays, out, coeff, mask, m->d_counters.p, s);
    return launch_check("k_sample_distance");
}
int gpis::transmittance_impl(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible, const uint8_t *mask, hipStream_t s,
                             int hint)
{
    if (n == 0) return GPIS_OK;
    ProfScope prof(m, 1, s);
    if (m->guide.enabled && wave_march_selected(m, hint))
        return wave_march(m, n, rays, mask, false, nullptr, nullptr, visible, s);
    if (m->guide.enabled && m->opt[GPIS_OPT_RANGE_LEN] > 0) {
        launch::range_transmittance(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->guide, n, rays, visible, mask, m->d_counters.p + 1, m->d_guide_cnt.p,
                                    (uint32_t)m->opt[GPIS_OPT_RANGE_LEN], s);
        return launch_check("k_guided_range_tr");
    }
    if (m->guide.enabled) {
        launch::guided_transmittance(m->host_model.exp_arg_max < 100.f, m->opt[GPIS_OPT_SHADOW_LEAN] != 0, m->d_model.p, m->fast, m->d_guide.p, n, rays, visible, mask, m->d_counters.p + 1, m->d_guide_cnt.p, s);
        return launch_check(m->opt[GPIS_OPT_SHADOW_LEAN] ? "k_shadow_lean" : "k_guided_transmittance");
    }
    if (m->fast.enabled) {
        launch::fast_transmittance(m->d_model.p, m->fast, n, rays, visible, mask, m->d_counters.p + 1, s);
        return launch_check("k_fast_transmittance");
    }
    const DevModel &H = m->host_model;
    if (m->opt[GPIS_OPT_PERSISTENT] && persist_supported(H)) {
        PersistArgs a{};
        a.n = n; a.rays = rays; a.out = nullptr; a.coeff = nullptr; a.visible = visible; a.mask = mask; a.cnt = m->d_counters.p + 1;
        return launch_persist<false>(m, a, s);
    }
    launch::lane_transmittance(lane_instance(H), m->d_model.p, n, rays, visible, mask, m->d_counters.p + 1, s);
    return launch_check("k_transmittance");
}

// The Lambert frame driver's compact body (gpis_scene.hpp: 32-byte records): the marches k_guided_sample_distance_noexit and
// k_guided_transmittance run, on the same counters and profile slots, reading the camera position / the light direction from the
// launch.  lambert_compact() is true exactly when sample_distance_impl(exit_state = false) and transmittance_impl would launch those
// two kernels for a coherent batch; every other selection keeps the full-record body.  `guided` is m->guide.enabled for a render call
// (under the handle's lock); gpis_reserve_scene_workspace, which runs beside gpis_build_guide without the lock, passes what it
// expects instead and does not read the field the build is writing.
bool gpis::lambert_compact(const gpis_medium *m, bool guided)
{
    return m->opt[GPIS_OPT_SCENE_COMPACT] && guided && !wave_march_selected(m, MARCH_COHERENT) && m->opt[GPIS_OPT_RANGE_LEN] == 0 &&
           !m->opt[GPIS_OPT_DEFER_GRAD] && !m->opt[GPIS_OPT_SCENE_EXIT_STATE];
}
int gpis::scene_sample_distance_compact(gpis_medium *m, size_t n, const SceneRay *rays, SceneHit *out, const float origin[3], hipStream_t s)
{
    if (n == 0) return GPIS_OK;
    ProfScope prof(m, 0, s);
    launch::guided_sample_distance_scene(m->host_model.exp_arg_max < 100.f, m->d_model.p, m->fast, m->d_guide.p, n, rays, out, origin, m->d_counters.p, m->d_guide_cnt.p, s);
    return launch_check("k_guided_sample_distance_scene");
}
int gpis::scene_transmittance_compact(gpis_medium *m, size_t n, const SceneRay *rays, const float light[3], uint8_t *visible, hipStream_t s)
{
    if (n == 0) return GPIS_OK;
    ProfScope prof(m, 1, s);
    launch::guided_transmittance_scene(m->host_model.exp_arg_max < 100.f, m->opt[GPIS_OPT_SHADOW_LEAN] != 0, m->d_model.p, m->fast, m->d_guide.p, n, rays, light, visible, m->d_counters.p + 1, m->d_guide_cnt.p, s);
    return launch_check(m->opt[GPIS_OPT_SHADOW_LEAN] ? "k_shadow_lean_scene" : "k_guided_transmittance_scene");
}

extern "C" int gpis_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, gpis_cond_coeff *coeff, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && out)));
    std::lock_guard<std::mutex> lock(m->mu);      // the handle's event lists / wavefront workspace are shared; held while ENQUEUEING only
    HIP_TRY(hipSetDevice(m->device));
    return sample_distance_impl(m, n, rays, out, coeff, nullptr, (hipStream_t)stream, m->batch_hint);
}
extern "C" int gpis_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && visible)));
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    return transmittance_impl(m, n, rays, visible, nullptr, (hipStream_t)stream, m->batch_hint);
}
extern "C" int gpis_set_batch_order(gpis_medium *m, int order)
{
    CHECK_ARGS(std_handle(m) && (order == GPIS_ORDER_COHERENT || order == GPIS_ORDER_SCATTERED));
    std::lock_guard<std::mutex> lock(m->mu);
    m->batch_hint = order;
    return GPIS_OK;
}
extern "C" int gpis_set_option(gpis_medium *m, int option, long long value)
{
    CHECK_ARGS(std_handle(m) && option >= 0 && option < GPIS_OPT_COUNT_);
    switch (option) {
    case GPIS_OPT_MARCH_FORM: CHECK_ARGS(value >= GPIS_MARCH_FORM_AUTO && value <= GPIS_MARCH_FORM_WAVE); break;
    case GPIS_OPT_WAVE_TAIL: CHECK_ARGS(value >= 0); break;
    case GPIS_OPT_PATHS_SORT: case GPIS_OPT_PATHS_PRESORT: case GPIS_OPT_PERSISTENT: case GPIS_OPT_DEFER_GRAD: case GPIS_OPT_SCENE_EXIT_STATE: case GPIS_OPT_SCENE_COMPACT: case GPIS_OPT_SHADOW_LEAN: CHECK_ARGS(value == 0 || value == 1); break;
    case GPIS_OPT_CHUNK_LOG2: CHECK_ARGS(value == 0 || (value >= 8 && value <= 28)); break;    // below 16: chunks smaller than a record of a pass
    case GPIS_OPT_SOLO_MAX: CHECK_ARGS(value >= -1 && value <= 64); break;
    case GPIS_OPT_RANGE_LEN: CHECK_ARGS(value >= 0 && value <= (1 << 24) && value % 64 == 0); break;
    default: break;
    }
    std::lock_guard<std::mutex> lock(m->mu);
    m->opt[option] = value;
    return GPIS_OK;
}
extern "C" int gpis_get_option(gpis_medium *m, int option, long long *value)
{
    CHECK_ARGS(std_handle(m) && value && option >= 0 && option < GPIS_OPT_COUNT_);
    std::lock_guard<std::mutex> lock(m->mu);
    *value = m->opt[option];
    return GPIS_OK;
}
extern "C" int gpis_eval_value_batch(gpis_medium *m, size_t n, const gpis_query *q, float *value, int32_t *gp_id, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && value)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    launch::eval_value(m->d_model.p, n, q, value, gp_id, m->d_counters.p, (hipStream_t)stream);
    return launch_check("k_eval_value");
}
extern "C" int gpis_eval_gradient_batch(gpis_medium *m, size_t n, const gpis_query *q, float *grad3, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && grad3)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    launch::eval_gradient(m->d_model.p, n, q, grad3, m->d_counters.p, (hipStream_t)stream);
    return launch_check("k_eval_gradient");
}
extern "C" int gpis_conditioning_batch(gpis_medium *m, size_t n, const gpis_query *q, const float *target_val, const float *target_grad3,
                                       gpis_cond_coeff *coeff_out, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && target_val && target_grad3 && coeff_out)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    launch::conditioning(m->d_model.p, n, q, target_val, target_grad3, coeff_out, m->d_counters.p, (hipStream_t)stream);
    return launch_check("k_conditioning");
}
extern "C" int gpis_nee_pdf_batch(gpis_medium *m, size_t n, const gpis_nee_query *q, float *pdf, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && pdf)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    launch::nee(nee_instance(m->host_model), m->d_model.p, n, q, pdf, nullptr, m->d_counters.p, nullptr, (hipStream_t)stream);
    return launch_check("k_nee");
}
extern "C" int gpis_nee_grad_batch(gpis_medium *m, size_t n, const gpis_nee_query *q, float *grad3, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && grad3)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    launch::nee(nee_instance(m->host_model), m->d_model.p, n, q, nullptr, grad3, m->d_counters.p, nullptr, (hipStream_t)stream);
    return launch_check("k_nee");
}
extern "C" int gpis_mean_color_emission_batch(gpis_medium *m, size_t n, const double *p3, float *color3, float *emission3, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || p3));
    if (n == 0 || (!color3 && !emission3)) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    k_mean_color_emission<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(m->d_model.p, n, p3, color3, emission3);
    return launch_check("k_mean_color_emission");
}
extern "C" int gpis_mean_batch(gpis_medium *m, size_t n, const double *p3, double *value, int32_t *id, double *grad3, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || p3));
    if (n == 0 || (!value && !id && !grad3)) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    k_mean<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(m->d_model.p, n, p3, value, id, grad3);
    return launch_check("k_mean");
}
// function-space comparison path: gpis_fs.hpp
int gpis::fs_check(gpis_medium *m)
{
    const DevModel &H = m->host_model;
    if (H.sdf_mean)
        return set_err(GPIS_ERR_UNSUPPORTED, "function-space path: a procedural (SDF) or tabulated (voxel grid) mean is outside its built scope");
    if (H.fs_n < 2 || H.fs_n > GPIS_FS_MAX_POINTS || !(H.fs_step >= 0) || H.kernel_type != GPIS_KERNEL_SQUARED_EXPONENTIAL || H.nonstationary ||
        H.use_aniso_mtx || H.has_mean_additional || (H.color.enabled && H.color.type >= GPIS_NOISE_SANDSTONE))
        return set_err(GPIS_ERR_INVALID_ARG, "function-space path: squared-exponential covariance, analytic mean (ramp colour), 2..64 sample points");
    return GPIS_OK;
}
// 37 KB of LDS per workgroup: four one-wave workgroups (one per SIMD) are resident per CU and walk the batch; each owns one
// slice of the L2-resident workspace and, behind the slices, two state slots (2.4 KB each): bank 0 holds the frame drivers' path
// states, bank 1 the path driver's shadow copies (k_fs_scene uses bank 0 alone).  scene_rec_bytes: the frame drivers' record array
// and work counter, grown here under the same lock.
int gpis::fs_workspace(gpis_medium *m, unsigned &cap, size_t scene_rec_bytes)
{
    cap = (unsigned)(m->n_cus > 0 ? m->n_cus : 256) * 4u;
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->fs_ws_blocks < cap) {
        if (m->fs_ws.p) HIP_TRY(hipDeviceSynchronize());
        m->fs_slots = nullptr; m->fs_ws_blocks = 0;
        const size_t slices = (size_t)cap * launch::fs_workspace_bytes_per_block();
        if (m->fs_ws.grow(slices + 2 * (size_t)cap * sizeof(gpis_fs_state)) != hipSuccess) { (void)hipGetLastError(); return set_err(GPIS_ERR_DEVICE, "function-space workspace allocation failed"); }
        m->fs_slots = (gpis_fs_state *)((char *)m->fs_ws.p + slices);
        m->fs_ws_blocks = cap;
    }
    if (scene_rec_bytes && m->fs_scene_next.grow(sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(GPIS_ERR_DEVICE, "function-space frame counter allocation failed");
    }
    if (m->fs_scene_recs.bytes < scene_rec_bytes) {
        if (m->fs_scene_recs.p) HIP_TRY(hipDeviceSynchronize());
        if (m->fs_scene_recs.grow(scene_rec_bytes) != hipSuccess) { (void)hipGetLastError(); return set_err(GPIS_ERR_DEVICE, "function-space frame records: no memory for %zu bytes", scene_rec_bytes); }
    }
    return GPIS_OK;
}
static int fs_launch(bool want_sample, gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, gpis_seg_out *out, uint8_t *visible, hipStream_t s)
{
    HIP_TRY(hipSetDevice(m->device));
    unsigned cap = 0;
    if (int st = fs_workspace(m, cap)) return st;
    const unsigned grid = (unsigned)(n < cap ? n : cap);
    launch::fs_march(want_sample, grid, m->d_model.p, n, rays, states, out, visible, m->fs_ws.p, s);
    return launch_check("k_fs_march");
}
#ifdef GPIS_FS_PROF
extern "C" int gpis_fs_prof_read(unsigned long long *out16, int reset) { return launch::fs_prof_read(out16, reset); }
#endif
extern "C" int gpis_fs_linalg_batch(gpis_medium *m, int op, int n, size_t count, const double *in, double *out, double *evals, void *stream)
{
    CHECK_ARGS(std_handle(m) && op >= GPIS_FS_OP_EIGH && op <= GPIS_FS_OP_PINV && n >= 1 && n <= GPIS_FS_MAX_CTX && (count == 0 || (in && out)));
    if (count == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    unsigned cap = 0;
    if (int st = fs_workspace(m, cap)) return st;
    launch::fs_linalg((unsigned)(count < cap ? count : cap), op, n, count, in, out, evals, m->fs_ws.p, (hipStream_t)stream);
    return launch_check("k_fs_linalg");
}
extern "C" int gpis_sort_pairs_u32(size_t n, const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out, void *stream)
{
    CHECK_ARGS(n == 0 || (keys_in && vals_in && keys_out && vals_out));
    size_t tb = 0;
    if (sort_pairs_u32(nullptr, tb, nullptr, nullptr, nullptr, nullptr, n, (hipStream_t)stream) != hipSuccess)
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_sort_pairs_u32: batch too large");
    if (n == 0) return GPIS_OK;
    DevBuf<> temp;
    HIP_TRY(temp.grow(tb));
    hipError_t e = sort_pairs_u32(temp.p, tb, keys_in, keys_out, vals_in, vals_out, n, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return set_err(GPIS_ERR_DEVICE, "gpis_sort_pairs_u32: %s", hipGetErrorString(e));
    return GPIS_OK;
}
extern "C" int gpis_libm_batch(int fn, size_t n, const double *x, const double *y, double *out, double *out2, void *stream)
{
    CHECK_ARGS(fn >= GPIS_LIBM_EXP && fn <= GPIS_LIBM_SINCOSF && (n == 0 || (x && out)) && (fn != GPIS_LIBM_POW || n == 0 || y) && ((fn != GPIS_LIBM_SINCOS && fn != GPIS_LIBM_SINCOSF) || n == 0 || out2));
    if (n == 0) return GPIS_OK;
    launch::libm_eval(fn, n, x, y, out, out2, (hipStream_t)stream);
    return launch_check("k_libm");
}
extern "C" int gpis_fs_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, gpis_seg_out *out, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && states && out)));
    if (int st = fs_check(m)) return st;
    if (n == 0) return GPIS_OK;
    return fs_launch(true, m, n, rays, states, out, nullptr, (hipStream_t)stream);
}
extern "C" int gpis_fs_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, uint8_t *visible, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && states && visible)));
    if (int st = fs_check(m)) return st;
    if (n == 0) return GPIS_OK;
    return fs_launch(false, m, n, rays, states, nullptr, visible, (hipStream_t)stream);
}
// host-pointer forms of the two function-space entries: one staging round trip per call (stage[0..2] are shared by the
// host conveniences of this handle, so the whole call holds the handle's host mutex; the workspace has its own lock)
static int fs_host(gpis_medium *m, bool want_sample, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, void *out)
{
    if (int st = fs_check(m)) return st;
    if (n == 0) return GPIS_OK;
    DevBuf<> *d = m->fs_stage;
    return host_round_trip(m->fs_host_mu, m->device, d, GrowStage{d},
                           {{rays, nullptr, n * sizeof(gpis_ray_in), 0}, {states, states, n * sizeof(gpis_fs_state), 1}, {nullptr, out, n * (want_sample ? sizeof(gpis_seg_out) : 1), 2}},
                           [&] { return fs_launch(want_sample, m, n, (const gpis_ray_in *)d[0].p, (gpis_fs_state *)d[1].p, want_sample ? (gpis_seg_out *)d[2].p : nullptr,
                                                  want_sample ? nullptr : (uint8_t *)d[2].p, nullptr); });
}
extern "C" int gpis_fs_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, gpis_seg_out *out)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && states && out)));
    return fs_host(m, true, n, rays, states, out);
}
extern "C" int gpis_fs_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, uint8_t *visible)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && states && visible)));
    return fs_host(m, false, n, rays, states, visible);
}
extern "C" int gpis_mean_color_emission_host(gpis_medium *m, size_t n, const double *p3, float *color3, float *emission3)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || p3));
    if (n == 0 || (!color3 && !emission3)) return GPIS_OK;
    return host_trip(m, {{p3, nullptr, 3 * n * sizeof(double), 0}, {nullptr, color3, 3 * n * sizeof(float), 1}, {nullptr, emission3, 3 * n * sizeof(float), 2}},
                     [&] { return gpis_mean_color_emission_batch(m, n, (const double *)m->stage[0].p, color3 ? (float *)m->stage[1].p : nullptr, emission3 ? (float *)m->stage[2].p : nullptr, nullptr); });
}
extern "C" int gpis_mean_host(gpis_medium *m, size_t n, const double *p3, double *value, int32_t *id, double *grad3)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || p3));
    if (n == 0 || (!value && !id && !grad3)) return GPIS_OK;
    // stage[1]: n values, then 3 n gradient components; stage[2]: n ids
    return host_trip(m, {{p3, nullptr, 3 * n * sizeof(double), 0}, {nullptr, value, n * sizeof(double), 1}, {nullptr, id, n * sizeof(int32_t), 2}, {nullptr, grad3, 3 * n * sizeof(double), 1, n * sizeof(double)}},
                     [&] { double *d_val = (double *)m->stage[1].p;
                           return gpis_mean_batch(m, n, (const double *)m->stage[0].p, value ? d_val : nullptr, id ? (int32_t *)m->stage[2].p : nullptr, grad3 ? d_val + n : nullptr, nullptr); });
}
extern "C" int gpis_xxhash32_batch(gpis_medium *m, size_t n, int arity, const uint32_t *words, uint32_t *out, void *stream)
{
    CHECK_ARGS(std_handle(m) && arity >= 1 && arity <= 4 && (n == 0 || (words && out)));
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    k_xxhash32<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(n, arity, words, out);
    return launch_check("k_xxhash32");
}
extern "C" int gpis_pcg32_stream_batch(gpis_medium *m, size_t n, const uint64_t *state, uint32_t count, uint32_t *out, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (state && out)));
    if (n == 0 || count == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(m->device));
    k_pcg32_stream<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(n, state, count, out);
    return launch_check("k_pcg32_stream");
}

// ---- host-pointer conveniences -----------------------------------------------------------
// ---- pipelined host path ------------------------------------------------------------------------------------
// Records move in chunks through two slots (streams): H2D of chunk k, the march kernel of chunk k-1 and D2H of chunk k-2
// overlap.  Caller memory that is pinned (gpis_alloc_host, hipHostMalloc, hipHostRegister) is DMA'd directly; pageable
// memory is staged through the slot's own pinned buffers (one memcpy each way).  A batch of one costs one small H2D,
// one launch, one D2H and one stream synchronise.
// records per chunk: 32 MiB of rays in, 24 MiB of results out.  Measured on C1 (guided march, pinned caller memory, 1 Mi rays):
// 64 Ki-record chunks 74 M segments/s — each chunk's kernel is too small to fill the chip (61 M segments/s for a lone 64 Ki batch
// against 361 M for 1 Mi) — so chunks are as large as the overlap of three stages allows
constexpr size_t kHostChunk = 262144;
constexpr size_t kInRec = sizeof(gpis_ray_in), kOutRecMax = sizeof(gpis_seg_out), kAuxRec = sizeof(gpis_cond_coeff);

static bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}
static int host_slot_ensure(gpis_medium *m, int k, size_t cap)
{
    gpis_medium::HostSlot &S = m->hs[k];
    if (!S.stream) HIP_TRY(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    if (!S.done) HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    if (S.cap >= cap) return GPIS_OK;
    HIP_TRY(hipStreamSynchronize(S.stream));
    S.pin_in.reset(); S.pin_out.reset(); S.pin_aux.reset(); S.dev_in.reset(); S.dev_out.reset(); S.dev_aux.reset(); S.cap = 0;      // all six go before the first comes back
    HIP_TRY(S.pin_in.grow(cap * kInRec));
    HIP_TRY(S.pin_out.grow(cap * kOutRecMax));
    HIP_TRY(S.pin_aux.grow(cap * kAuxRec));
    HIP_TRY(S.dev_in.grow(cap * kInRec));
    HIP_TRY(S.dev_out.grow(cap * kOutRecMax));
    HIP_TRY(S.dev_aux.grow(cap * kAuxRec));
    S.cap = cap;
    return GPIS_OK;
}
// sample == true: sampleDistance (out = gpis_seg_out, aux = gpis_cond_coeff or null); false: transmittance (out = uint8_t)
static int host_march(gpis_medium *m, bool sample, size_t n, const gpis_ray_in *rays, void *out, gpis_cond_coeff *aux)
{
    const size_t out_rec = sample ? sizeof(gpis_seg_out) : 1;
    const size_t chunk = n < kHostChunk ? n : kHostChunk;
    const size_t cap = chunk <= 256 ? 256 : (chunk <= 16384 ? 16384 : kHostChunk);   // small batches keep a small slot
    int st;
    if ((st = host_slot_ensure(m, 0, cap)) || (n > chunk && (st = host_slot_ensure(m, 1, cap))))
        return st;
    // whether the caller's buffers are pinned decides between DMA from them and a copy through the slot's pinned staging; small
    // batches (the Medium adapter's batch of one) go through the staging without asking — three pointer queries cost more than
    // the copies they would save
    const bool ask = n >= 4096;
    const bool in_pinned = ask && is_pinned_host(rays), out_pinned = ask && is_pinned_host(out), aux_pinned = ask && aux && is_pinned_host(aux);
    const size_t n_chunks = (n + chunk - 1) / chunk;
    struct Pending { size_t first, count; bool live; } pend[2] = {{0, 0, false}, {0, 0, false}};
    auto retire = [&](int k) -> int {      // chunk in slot k has finished: hand its results to the caller
        gpis_medium::HostSlot &S = m->hs[k];
        if (!pend[k].live) return GPIS_OK;
        HIP_TRY(hipEventSynchronize(S.done));
        if (!out_pinned) memcpy((char *)out + pend[k].first * out_rec, S.pin_out.p, pend[k].count * out_rec);
        if (aux && !aux_pinned) memcpy(aux + pend[k].first, S.pin_aux.p, pend[k].count * kAuxRec);
        pend[k].live = false;
        return GPIS_OK;
    };
    for (size_t c = 0; c < n_chunks; ++c) {
        const int k = (int)(c & 1);
        gpis_medium::HostSlot &S = m->hs[k];
        if ((st = retire(k))) return st;
        const size_t first = c * chunk, count = n - first < chunk ? n - first : chunk;
        const void *src = rays + first;
        if (!in_pinned) { memcpy(S.pin_in.p, src, count * kInRec); src = S.pin_in.p; }
        HIP_TRY(hipMemcpyAsync(S.dev_in.p, src, count * kInRec, hipMemcpyHostToDevice, S.stream));
        if (sample)
            st = sample_distance_impl(m, count, (const gpis_ray_in *)S.dev_in.p, (gpis_seg_out *)S.dev_out.p, aux ? (gpis_cond_coeff *)S.dev_aux.p : nullptr, nullptr, S.stream);
        else
            st = transmittance_impl(m, count, (const gpis_ray_in *)S.dev_in.p, (uint8_t *)S.dev_out.p, nullptr, S.stream);
        if (st) return st;
        HIP_TRY(hipMemcpyAsync(out_pinned ? (char *)out + first * out_rec : S.pin_out.p, S.dev_out.p, count * out_rec, hipMemcpyDeviceToHost, S.stream));
        if (aux) HIP_TRY(hipMemcpyAsync(aux_pinned ? (char *)(aux + first) : S.pin_aux.p, S.dev_aux.p, count * kAuxRec, hipMemcpyDeviceToHost, S.stream));
        HIP_TRY(hipEventRecord(S.done, S.stream));
        pend[k] = {first, count, true};
    }
    if ((st = retire((int)(n_chunks & 1)))) return st;       // the older chunk first
    return retire((int)((n_chunks + 1) & 1));
}
extern "C" int gpis_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, gpis_cond_coeff *coeff)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && out)));
    if (n == 0) return GPIS_OK;
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    return host_march(m, true, n, rays, out, coeff);
}
extern "C" int gpis_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (rays && visible)));
    if (n == 0) return GPIS_OK;
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    return host_march(m, false, n, rays, visible, nullptr);
}
extern "C" void *gpis_alloc_host(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void gpis_free_host(void *p)
{
    if (p) (void)hipHostFree(p);
}
extern "C" int gpis_eval_value_host(gpis_medium *m, size_t n, const gpis_query *q, float *value, int32_t *gp_id)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && value)));
    if (n == 0) return GPIS_OK;
    return host_trip(m, {{q, nullptr, n * sizeof(gpis_query), 0}, {nullptr, value, n * sizeof(float), 1}, {nullptr, gp_id, n * sizeof(int32_t), 2}},
                     [&] { return gpis_eval_value_batch(m, n, (const gpis_query *)m->stage[0].p, (float *)m->stage[1].p, (int32_t *)m->stage[2].p, nullptr); });
}
extern "C" int gpis_eval_gradient_host(gpis_medium *m, size_t n, const gpis_query *q, float *grad3)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && grad3)));
    if (n == 0) return GPIS_OK;
    return host_trip(m, {{q, nullptr, n * sizeof(gpis_query), 0}, {nullptr, grad3, 3 * n * sizeof(float), 1}},
                     [&] { return gpis_eval_gradient_batch(m, n, (const gpis_query *)m->stage[0].p, (float *)m->stage[1].p, nullptr); });
}

extern "C" int gpis_conditioning_host(gpis_medium *m, size_t n, const gpis_query *q, const float *target_val, const float *target_grad3,
                                      gpis_cond_coeff *coeff_out)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && target_val && target_grad3 && coeff_out)));
    if (n == 0) return GPIS_OK;
    // stage[1]: n target values, then 3 n target gradient components
    return host_trip(m, {{q, nullptr, n * sizeof(gpis_query), 0}, {target_val, nullptr, n * sizeof(float), 1}, {target_grad3, nullptr, 3 * n * sizeof(float), 1, n * sizeof(float)},
                         {nullptr, coeff_out, n * sizeof(gpis_cond_coeff), 2}},
                     [&] { float *d_tv = (float *)m->stage[1].p;
                           return gpis_conditioning_batch(m, n, (const gpis_query *)m->stage[0].p, d_tv, d_tv + n, (gpis_cond_coeff *)m->stage[2].p, nullptr); });
}
static int nee_host(gpis_medium *m, size_t n, const gpis_nee_query *q, float *pdf, float *grad3)
{
    // stage[1] has room for the gradients whichever of the two is asked for
    return host_trip(m, {{q, nullptr, n * sizeof(gpis_nee_query), 0}, {nullptr, nullptr, 3 * n * sizeof(float), 1}, {nullptr, pdf ? pdf : grad3, (pdf ? 1 : 3) * n * sizeof(float), 1}},
                     [&] { return pdf ? gpis_nee_pdf_batch(m, n, (const gpis_nee_query *)m->stage[0].p, (float *)m->stage[1].p, nullptr)
                                      : gpis_nee_grad_batch(m, n, (const gpis_nee_query *)m->stage[0].p, (float *)m->stage[1].p, nullptr); });
}
extern "C" int gpis_nee_pdf_host(gpis_medium *m, size_t n, const gpis_nee_query *q, float *pdf)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && pdf)));
    return n ? nee_host(m, n, q, pdf, nullptr) : GPIS_OK;
}
extern "C" int gpis_nee_grad_host(gpis_medium *m, size_t n, const gpis_nee_query *q, float *grad3)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || (q && grad3)));
    return n ? nee_host(m, n, q, nullptr, grad3) : GPIS_OK;
}

// ---- measurement -------------------------------------------------------------------------
extern "C" int gpis_get_counters(gpis_medium *m, uint64_t *n_eval, uint64_t *n_seg)
{
    CHECK_ARGS(std_handle(m));
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    Counters c[2];
    HIP_TRY(hipMemcpy(c, m->d_counters.p, sizeof c, hipMemcpyDeviceToHost));
    if (n_eval) *n_eval = c[0].n_eval + c[1].n_eval;
    if (n_seg) *n_seg = c[0].n_seg + c[1].n_seg;
    return GPIS_OK;
}
extern "C" int gpis_reset_counters(gpis_medium *m)
{
    CHECK_ARGS(std_handle(m));
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(m->d_counters.p, 0, 2 * sizeof(Counters)));
    HIP_TRY(hipMemset(m->d_guide_cnt.p, 0, 8 * sizeof(unsigned long long)));
    for (int k = 0; k < 3; ++k) { m->events_used[k] = 0; m->prof_ms[k] = 0.; m->prof_launches[k] = 0; }
    return GPIS_OK;
}

// ---- guide field ---------------------------------------------------------------------------
extern "C" int gpis_build_guide(gpis_medium *m, int half_extent_cells, int points_per_cell)
{
    CHECK_ARGS(std_handle(m));
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    if (m->host_model.sdf_mean)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_build_guide: a procedural (SDF) or tabulated (voxel grid) mean has no guide field (no per-brick bound of such a mean is built)");
    if (!m->fast.enabled)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_build_guide: the medium is not covered by the wave-cooperative path (single_realization, 3D, stationary SE, diagonal anisotropy)");
    int st = launch::guide_build(m->host_model, m->d_model.p, m->fast, half_extent_cells, points_per_cell, &m->guide, getenv("GPIS_GUIDE_DENSE") == nullptr);
    if (st != GPIS_OK)
        return set_err(st, "gpis_build_guide(half=%d, ppc=%d) failed: %s", half_extent_cells, points_per_cell,
                       st == GPIS_ERR_UNSUPPORTED ? "unsupported arguments" : hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipMemcpy(m->d_guide.p, &m->guide, sizeof(GuideField), hipMemcpyHostToDevice));
    return GPIS_OK;
}
extern "C" int gpis_drop_guide(gpis_medium *m)
{
    CHECK_ARGS(std_handle(m));
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    guide_free(&m->guide);
    HIP_TRY(hipMemcpy(m->d_guide.p, &m->guide, sizeof(GuideField), hipMemcpyHostToDevice));
    return GPIS_OK;
}
extern "C" int gpis_get_guide_steps(gpis_medium *m, uint64_t *n_guide)
{
    CHECK_ARGS(std_handle(m) && n_guide);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, m->d_guide_cnt.p, sizeof v, hipMemcpyDeviceToHost));
    *n_guide = v;
    return GPIS_OK;
}
extern "C" int gpis_guide_selfcheck(gpis_medium *m, size_t n, const float *points3, uint64_t *checked, uint64_t *violations,
                                    float *max_ratio, float *mean_bound, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || points3));
    if (!m->guide.enabled) return set_err(GPIS_ERR_UNSUPPORTED, "gpis_guide_selfcheck: no guide field built");
    HIP_TRY(hipSetDevice(m->device));
    // scratch: [0] = points inside the field, [1] = violations, word 2 = {max ratio bits, sum of bounds}, [3] = points in tabulated bricks
    unsigned long long *st = m->d_guide_cnt.p + 1;
    HIP_TRY(hipMemsetAsync(st, 0, 4 * sizeof(unsigned long long), (hipStream_t)stream));
    if (n)
        launch::guide_selfcheck(m->d_model.p, m->fast, m->guide, n, points3, st, (float *)(st + 2), (float *)(st + 2) + 1, (hipStream_t)stream);
    int rc = launch_check("k_guide_selfcheck");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long h[4];
    HIP_TRY(hipMemcpy(h, st, sizeof h, hipMemcpyDeviceToHost));
    float fr[2];
    memcpy(fr, &h[2], sizeof fr);
    if (checked) *checked = h[0];
    if (violations) *violations = h[1];
    if (max_ratio) *max_ratio = fr[0];
    if (mean_bound) *mean_bound = h[3] ? fr[1] / (float)h[3] : 0.f;
    m->selfcheck_tabulated = h[3];
    return GPIS_OK;
}
extern "C" int gpis_get_guide_info(gpis_medium *m, gpis_guide_info *out)
{
    CHECK_ARGS(std_handle(m) && out);
    memset(out, 0, sizeof *out);
    if (!m->guide.enabled) return GPIS_OK;
    const GuideField &F = m->guide;
    const uint64_t nblk = (uint64_t)(F.side / 4) * (F.side / 4) * (F.side / 4);
    out->half_extent_cells = F.half; out->points_per_cell = F.ppc;
    out->bricks_total = nblk / 64; out->bricks_allocated = F.n_alloc; out->bricks_usable = F.n_usable;
    out->bytes_samples = (uint64_t)(F.n_alloc ? F.n_alloc : 1u) * kBrickFloats * 4;
    out->bytes_bounds = nblk * 8;
    out->bytes_dense = (uint64_t)F.side * F.side * F.side * 4;
    out->selfcheck_points_tabulated = m->selfcheck_tabulated;
    return GPIS_OK;
}

extern "C" int gpis_guide_raycheck(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint32_t steps, uint64_t *certified,
                                   uint64_t *violations, void *stream)
{
    CHECK_ARGS(std_handle(m) && (n == 0 || rays));
    if (!m->guide.enabled) return set_err(GPIS_ERR_UNSUPPORTED, "gpis_guide_raycheck: no guide field built");
    HIP_TRY(hipSetDevice(m->device));
    unsigned long long *st = m->d_guide_cnt.p + 1;
    HIP_TRY(hipMemsetAsync(st, 0, 3 * sizeof(unsigned long long), (hipStream_t)stream));
    if (n)
        launch::guide_raycheck(m->d_model.p, m->fast, m->guide, n, rays, steps, st, (hipStream_t)stream);
    int rc = launch_check("k_guide_raycheck");
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long h[2];
    HIP_TRY(hipMemcpy(h, st, sizeof h, hipMemcpyDeviceToHost));
    if (certified) *certified = h[0];
    if (violations) *violations = h[1];
    return GPIS_OK;
}

extern "C" int gpis_set_profiling(gpis_medium *m, int enable)
{
    CHECK_ARGS(std_handle(m));
    m->profiling = enable != 0;
    return GPIS_OK;
}
extern "C" int gpis_get_kernel_profile(gpis_medium *m, int which, double *total_ms, uint64_t *launches, uint64_t *n_eval, uint64_t *n_seg)
{
    CHECK_ARGS(std_handle(m) && which >= 0 && which <= 2);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    for (size_t i = 0; i < m->events_used[which]; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, m->events[which][i].first, m->events[which][i].second));
        m->prof_ms[which] += (double)ms;
        m->prof_launches[which]++;
    }
    m->events_used[which] = 0;
    Counters c[2];
    HIP_TRY(hipMemcpy(c, m->d_counters.p, sizeof c, hipMemcpyDeviceToHost));
    if (total_ms) *total_ms = m->prof_ms[which];
    if (launches) *launches = m->prof_launches[which];
    if (n_eval) *n_eval = which < 2 ? c[which].n_eval : 0;      // the NEE queries count into the sampleDistance pair
    if (n_seg) *n_seg = which < 2 ? c[which].n_seg : 0;
    return GPIS_OK;
}

#ifdef GPIS_FAST_STATS
// diagnostic build only: read and clear the cooperative loop's work counters (of the guided sampleDistance kernel's TU)
extern "C" int gpis_debug_fast_stats(uint64_t *out32)
{
    unsigned long long h[32];
    int st = launch::fast_stats_read(h);
    if (st != GPIS_OK) return st;
    for (int i = 0; i < 32; ++i) out32[i] = h[i];
    return GPIS_OK;
}
// ... and of the guided transmittance kernels' TU
extern "C" int gpis_debug_fast_stats_tr(uint64_t *out32)
{
    unsigned long long h[32];
    int st = launch::fast_stats_read_tr(h);
    if (st != GPIS_OK) return st;
    for (int i = 0; i < 32; ++i) out32[i] = h[i];
    return GPIS_OK;
}
#endif

extern "C" int gpis_set_variance_grid(gpis_medium *m, const gpis_variance_grid *g, const float *voxels)
{
    CHECK_ARGS(std_handle(m) && g && voxels);
    CHECK_ARGS(g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1 && (g->interpolate == 0 || g->interpolate == 1));
    if (!m->host_model.grid.on) return set_err(GPIS_ERR_INVALID_ARG, "gpis_set_variance_grid: the medium was not created with grid_nonstationary = 1");
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)g->dims[0] * (size_t)g->dims[1] * (size_t)g->dims[2];
    DevBuf<float> d;
    HIP_TRY(d.grow(n * sizeof(float)));
    if (hipMemcpy(d.p, voxels, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return set_err(GPIS_ERR_DEVICE, "gpis_set_variance_grid: copy failed");
    m->d_grid_vox.adopt(d.release(), n * sizeof(float));      // frees the earlier array
    DevGrid &G = m->host_model.grid;
    G.vox = m->d_grid_vox.p;
    G.interpolate = g->interpolate;
    for (int c = 0; c < 3; ++c) { G.dims[c] = g->dims[c]; G.origin[c] = g->origin[c]; G.lo[c] = g->bounds_min[c] + 2; G.hi[c] = g->bounds_max[c] - 3; }
    for (int i = 0; i < 12; ++i) G.T[i] = g->inv_natural_transform[i];
    HIP_TRY(hipMemcpy(m->d_model.p, &m->host_model, sizeof(DevModel), hipMemcpyHostToDevice));
    return GPIS_OK;
}

// the slot's device array `d` becomes its grid: descriptor into the host model, model refresh, the earlier array freed behind it.
// The caller holds the handle's lock and has waited for the device.
static int install_mean_grid(gpis_medium *m, int which, const gpis_variance_grid *g, size_t n, float *d)
{
    float *old = m->d_mean_vox[which].release();
    m->d_mean_vox[which].adopt(d, n * sizeof(float));
    DevGrid &G = m->host_model.mean_grid[which];
    G.vox = d;
    G.interpolate = g->interpolate;
    for (int c = 0; c < 3; ++c) { G.dims[c] = g->dims[c]; G.origin[c] = g->origin[c]; G.lo[c] = g->bounds_min[c] + 2; G.hi[c] = g->bounds_max[c] - 3; }
    for (int i = 0; i < 12; ++i) G.T[i] = g->inv_natural_transform[i];
    HIP_TRY(hipMemcpy(m->d_model.p, &m->host_model, sizeof(DevModel), hipMemcpyHostToDevice));
    if (old) HIP_TRY(hipFree(old));          // behind the model refresh: the device model never names a freed array
    return GPIS_OK;
}
// TabulatedMean's grid: the descriptor and the discipline of gpis_set_variance_grid, one device copy per slot
extern "C" int gpis_set_mean_grid(gpis_medium *m, int which, const gpis_variance_grid *g, const float *voxels)
{
    CHECK_ARGS(std_handle(m) && g && voxels && (which == 0 || which == 1));
    CHECK_ARGS(g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1 && (g->interpolate == 0 || g->interpolate == 1));
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->host_model.mean[which].type != GPIS_MEAN_TABULATED || (which == 1 && !m->host_model.has_mean_additional))
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_set_mean_grid: slot %d holds no tabulated mean", which);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)g->dims[0] * (size_t)g->dims[1] * (size_t)g->dims[2];
    DevBuf<float> d;
    HIP_TRY(d.grow(n * sizeof(float)));
    if (hipMemcpy(d.p, voxels, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return set_err(GPIS_ERR_DEVICE, "gpis_set_mean_grid: copy failed");
    return install_mean_grid(m, which, g, n, d.release());
}

// Mat4f::invert (Mat4f.hpp:75-101): the adjugate over the determinant, in float.  inv[4 i + j] is the cofactor of (row j, column i):
// with r0 < r1 < r2 the rows other than j and c0 < c1 < c2 the columns other than i, six triple products (a*b)*c summed left to
// right in the order and with the signs below (all flipped when i + j is odd) — the order the reference's expanded lines have.
// det = a[0] inv[0] + a[1] inv[4] + a[2] inv[8] + a[3] inv[12]; det == 0 gives the identity.
static void mat4_invert_ref(const float *a, float *out)
{
    static const int pick[6][3] = {{0, 1, 2}, {0, 1, 2}, {1, 0, 2}, {1, 0, 2}, {2, 0, 1}, {2, 0, 1}};     // rows of the three factors
    static const int cols[6][3] = {{0, 1, 2}, {0, 2, 1}, {0, 1, 2}, {0, 2, 1}, {0, 1, 2}, {0, 2, 1}};     // their columns
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
extern "C" int gpis_set_mean_transform(gpis_medium *m, int which, const float transform[16])
{
    CHECK_ARGS(std_handle(m) && transform && (which == 0 || which == 1));
    if (m->host_model.mean[which].type != GPIS_MEAN_PROCEDURAL || (which == 1 && !m->host_model.has_mean_additional))
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_set_mean_transform: slot %d holds no procedural mean", which);
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    float inv[16];
    mat4_invert_ref(transform, inv);
    memcpy(m->host_model.sdf_inv[which], inv, 12 * sizeof(float));
    HIP_TRY(hipMemcpy(m->d_model.p, &m->host_model, sizeof(DevModel), hipMemcpyHostToDevice));
    return GPIS_OK;
}

// ======================================================================================
// neural SDF means (gpis_nn_mean.hpp): the exact evaluator at points and on a lattice, and the bake into a tabulated slot
// ======================================================================================
constexpr size_t kNnChunkPoints = (size_t)1 << 18;          // points of one launch
constexpr size_t kNnWorkspaceBytes = (size_t)64 << 20;      // activation workspace of one launch (networks wider than 64)

static int nn_describe(const char *who, const gpis_mean_network *net, nn::Net &N, size_t &n_weights)
{
    if (net->n_layers < 2 || net->n_layers > GPIS_NN_MAX_LAYERS)
        return set_err(GPIS_ERR_INVALID_ARG, "%s: n_layers = %d, outside 2 .. %d", who, net->n_layers, GPIS_NN_MAX_LAYERS);
    memset(&N, 0, sizeof N);
    N.n_layers = net->n_layers;
    N.max_width = 3;
    size_t off = 0;
    for (int k = 0; k < net->n_layers; ++k) {
        const int in = net->dims[k][0], out = net->dims[k][1];
        if (in < 1 || out < 1 || in > GPIS_NN_MAX_WIDTH || out > GPIS_NN_MAX_WIDTH)
            return set_err(GPIS_ERR_INVALID_ARG, "%s: layer %d is %d -> %d; a width is 1 .. %d", who, k, in, out, GPIS_NN_MAX_WIDTH);
        if (k == 0 && in != 3) return set_err(GPIS_ERR_INVALID_ARG, "%s: the first layer takes %d inputs, not the 3 of a point", who, in);
        if (k > 0 && in != net->dims[k - 1][1])
            return set_err(GPIS_ERR_INVALID_ARG, "%s: layer %d takes %d inputs but layer %d gives %d", who, k, in, k - 1, net->dims[k - 1][1]);
        if (k == net->n_layers - 1 && out != 1)
            return set_err(GPIS_ERR_INVALID_ARG, "%s: the last layer gives %d outputs; only 1 is built (more rows sum in another order)", who, out);
        N.dims[k][0] = in;
        N.dims[k][1] = out;
        N.w_off[k] = (uint32_t)off;
        off += (size_t)out * (size_t)(in + 1);
        if (out > N.max_width) N.max_width = out;
    }
    n_weights = off;
    for (int c = 0; c < 3; ++c) { N.bmin[c] = net->bounds_min[c]; N.bmax[c] = net->bounds_max[c]; }
    N.offset = net->offset;
    N.scale = net->scale;
    float inv[16];
    mat4_invert_ref(net->transform, inv);
    memcpy(N.inv, inv, sizeof N.inv);
    return GPIS_OK;
}
// points of one launch, and the bytes of its workspace: two buffers of max_width doubles per lane of the launch
static size_t nn_chunk(const nn::Net &N, size_t &ws_bytes)
{
    const size_t per_lane = 2 * (size_t)N.max_width * sizeof(double);
    if (N.max_width <= 64) { ws_bytes = 0; return kNnChunkPoints; }
    size_t c = kNnWorkspaceBytes / per_lane;
    c -= c % nn::kLanes;
    if (c > kNnChunkPoints) c = kNnChunkPoints;
    ws_bytes = c * per_lane;
    return c;
}
// lat == nullptr: value / grad3 at the n points p3; otherwise voxels [0, n) of the lattice
static int nn_launch(const nn::Net &N, const double *W, size_t n, const double *p3, double *value, double *grad3, const nn::Lattice *lat, float *voxels,
                     double *ws, hipStream_t s)
{
    size_t ws_bytes;
    const size_t chunk = nn_chunk(N, ws_bytes);
    for (size_t a = 0; a < n; a += chunk) {
        const size_t c = n - a < chunk ? n - a : chunk;
        const unsigned blocks = (unsigned)grid_of(c, nn::kLanes);
        if (lat) {
            if (N.max_width <= 32) k_mean<32><<<blocks, nn::kLanes, 0, s>>>(N, W, *lat, a, c, voxels, nullptr);
            else if (N.max_width <= 64) k_mean<64><<<blocks, nn::kLanes, 0, s>>>(N, W, *lat, a, c, voxels, nullptr);
            else k_mean<0><<<blocks, nn::kLanes, 0, s>>>(N, W, *lat, a, c, voxels, ws);
        } else {
            double *v = value ? value + a : nullptr, *g = grad3 ? grad3 + 3 * a : nullptr;
            if (N.max_width <= 32) k_mean<32><<<blocks, nn::kLanes, 0, s>>>(N, W, c, p3 + 3 * a, v, g, nullptr);
            else if (N.max_width <= 64) k_mean<64><<<blocks, nn::kLanes, 0, s>>>(N, W, c, p3 + 3 * a, v, g, nullptr);
            else k_mean<0><<<blocks, nn::kLanes, 0, s>>>(N, W, c, p3 + 3 * a, v, g, ws);
        }
        if (int st = launch_check("k_mean (network)")) return st;
    }
    return GPIS_OK;
}
extern "C" int gpis_network_mean_batch(const gpis_mean_network *net, const double *weights, size_t n, const double *p3, double *value, double *grad3,
                                       void *stream)
{
    CHECK_ARGS(net && weights && (n == 0 || p3));
    nn::Net N;
    size_t n_weights;
    if (int st = nn_describe(__func__, net, N, n_weights)) return st;
    if (n == 0 || (!value && !grad3)) return GPIS_OK;
    size_t ws_bytes;
    (void)nn_chunk(N, ws_bytes);
    DevBuf<double> ws;       // freed on every way out
    HIP_TRY(ws.grow(ws_bytes));
    if (int st = nn_launch(N, weights, n, p3, value, grad3, nullptr, nullptr, ws.p, (hipStream_t)stream)) return st;
    if (ws_bytes) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));        // the workspace is this call's: its kernels end before it goes
    return GPIS_OK;
}
extern "C" int gpis_network_mean_host(const gpis_mean_network *net, const double *weights, size_t n, const double *p3, double *value, double *grad3)
{
    CHECK_ARGS(net && weights && (n == 0 || p3));
    nn::Net N;
    size_t n_weights;
    if (int st = nn_describe(__func__, net, N, n_weights)) return st;
    if (n == 0 || (!value && !grad3)) return GPIS_OK;
    DevBuf<double> dW, dP, dV, dG;
    HIP_TRY(dW.grow(n_weights * sizeof(double)));
    HIP_TRY(dP.grow(3 * n * sizeof(double)));
    if (value) HIP_TRY(dV.grow(n * sizeof(double)));
    if (grad3) HIP_TRY(dG.grow(3 * n * sizeof(double)));
    HIP_TRY(hipMemcpy(dW.p, weights, n_weights * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dP.p, p3, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    if (int st = gpis_network_mean_batch(net, dW.p, n, dP.p, dV.p, dG.p, nullptr)) return st;
    HIP_TRY(hipDeviceSynchronize());
    if (value) HIP_TRY(hipMemcpy(value, dV.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (grad3) HIP_TRY(hipMemcpy(grad3, dG.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    return GPIS_OK;
}
extern "C" int gpis_bake_mean_network(gpis_medium *m, int which, const gpis_mean_network *net, const double *weights, const gpis_variance_grid *g,
                                      const float index_to_world[12], float *voxels_out)
{
    CHECK_ARGS(std_handle(m) && net && weights && g && index_to_world && (which == 0 || which == 1));
    CHECK_ARGS(g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1 && (g->interpolate == 0 || g->interpolate == 1));
    nn::Net N;
    size_t n_weights;
    if (int st = nn_describe(__func__, net, N, n_weights)) return st;
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->host_model.mean[which].type != GPIS_MEAN_TABULATED || (which == 1 && !m->host_model.has_mean_additional))
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_bake_mean_network: slot %d holds no tabulated mean", which);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)g->dims[0] * (size_t)g->dims[1] * (size_t)g->dims[2];
    nn::Lattice lat;
    for (int c = 0; c < 3; ++c) { lat.dims[c] = g->dims[c]; lat.origin[c] = g->origin[c]; }
    memcpy(lat.A, index_to_world, sizeof lat.A);
    size_t ws_bytes;
    (void)nn_chunk(N, ws_bytes);
    DevBuf<double> dW, ws;
    DevBuf<float> vox;
    HIP_TRY(dW.grow(n_weights * sizeof(double)));
    HIP_TRY(ws.grow(ws_bytes));
    HIP_TRY(vox.grow(n * sizeof(float)));
    HIP_TRY(hipMemcpy(dW.p, weights, n_weights * sizeof(double), hipMemcpyHostToDevice));
    if (int st = nn_launch(N, dW.p, n, nullptr, nullptr, nullptr, &lat, vox.p, ws.p, nullptr)) return st;
    HIP_TRY(hipDeviceSynchronize());
    if (voxels_out) HIP_TRY(hipMemcpy(voxels_out, vox.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return install_mean_grid(m, which, g, n, vox.release());
}
