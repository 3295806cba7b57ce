// tu_ws.hip — the weight-space GP medium (gpis_ws.hpp): its kernels and its gpis_ws_* entry points (include/gpis.h).
//
// The handle (WsHandle) and the helpers every gpis_ws_* translation unit shares are in gpis_ws_host.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>

#include "gpis.h"
#include "gpis_ws.hpp"
#include "gpis_ws_host.hpp"

#pragma clang fp contract(off)

using namespace gpis;

namespace {

// the refusals of the built scope (include/gpis.h); no device needed
int ws_validate(const gpis_params &P, const gpis_ws_params &S)
{
    if (P.abi_version != GPIS_ABI_VERSION) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: abi_version %u != %d", P.abi_version, GPIS_ABI_VERSION);
    if (S.version != GPIS_WS_PARAMS_VERSION) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: gpis_ws_params.version %u != %d", S.version, GPIS_WS_PARAMS_VERSION);
    if (P.correlation_context < GPIS_CTX_GLOBAL || P.correlation_context > GPIS_CTX_NONE)
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: correlation_context %d", P.correlation_context);
    if (S.basis_functions < 0 || S.basis_functions > GPIS_WS_MAX_BASIS)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: basis_functions %d outside 0..%d", S.basis_functions, GPIS_WS_MAX_BASIS);
    if (!(P.step_size > 0.f))
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: step_size %g: only the ray march (step_size > 0) is built, not the affine-arithmetic "
                                            "sphere trace of step_size == 0 (WSM:186-235)", (double)P.step_size);
    if (P.kernel_type != GPIS_KERNEL_SQUARED_EXPONENTIAL || P.nonstationary || P.grid_nonstationary)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: only the stationary squared-exponential covariance is built: the spectral samplers of "
                                            "the other kernels and of the non-stationary wrappers draw from std::mt19937 / std::gamma_distribution");
    if (S.normal_method == GPIS_NORMAL_BECKMANN || S.normal_method == GPIS_NORMAL_GGX)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: normal_method beckmann / ggx is outside the built scope");
    if (S.normal_method != GPIS_NORMAL_CONDITIONED_GAUSSIAN && S.normal_method != GPIS_NORMAL_FINITE_DIFFERENCES)
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: normal_method %d", S.normal_method);
    if (S.intersect_method == GPIS_INTERSECT_MEAN)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: intersect_method mean is outside the built scope");
    if (S.intersect_method != GPIS_INTERSECT_GP_DISCRETE)
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: intersect_method %d", S.intersect_method);
    if (P.mean_color.enabled && P.mean_color.type >= GPIS_NOISE_SANDSTONE)
        return set_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_create: a sandstone / rust mean colour is outside the built scope (ramp colours only)");
    for (int w = 0; w < 1 + (P.has_mean_additional ? 1 : 0); ++w) {
        const int t = w ? P.mean_additional.type : P.mean.type;
        if (t == GPIS_MEAN_TABULATED) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: a tabulated (voxel grid) mean is outside the built scope of the weight-space medium");
        if (t == GPIS_MEAN_PROCEDURAL) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: a procedural (SDF) mean is outside the built scope of the weight-space medium");
        if (t < GPIS_MEAN_HOMOGENEOUS || t > GPIS_MEAN_LINEAR) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: mean type %d", t);
    }
    return GPIS_OK;
}

int march(WsHandle *h, bool want_sample, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, uint8_t *visible, hipStream_t s)
{
    if (n == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(h->device));
    const unsigned grid = (unsigned)(n < h->grid_cap ? n : h->grid_cap);
    if (int st = ws_ensure_work(h, grid)) return st;
    if (want_sample)
        k_ws_march<true><<<grid, 64, 0, s>>>(h->d_model.p, n, rays, out, nullptr, h->d_work.p, h->d_counters.p);
    else
        k_ws_march<false><<<grid, 64, 0, s>>>(h->d_model.p, n, rays, nullptr, visible, h->d_work.p, h->d_counters.p);
    if (int st = launch_check("k_ws_march")) return st;
    return ws_check_overflow(h, s);
}

// the host-pointer form: results are copied back also when the march refused them as GPIS_ERR_UNSUPPORTED (ws_check_overflow)
int march_host(WsHandle *h, bool want_sample, size_t n, const gpis_ray_in *rays, void *out)
{
    if (n == 0) return GPIS_OK;
    return host_round_trip(h->mu, h->device, h->stage, GrowStage{h->stage}, {{rays, nullptr, n * sizeof(gpis_ray_in), 0}, {nullptr, out, n * (want_sample ? sizeof(gpis_seg_out) : 1), 1}},
                           [&] { return march(h, want_sample, n, (const gpis_ray_in *)h->stage[0].p, want_sample ? (gpis_seg_out *)h->stage[1].p : nullptr,
                                              want_sample ? nullptr : (uint8_t *)h->stage[1].p, nullptr); },
                           kTripNoSync | kTripKeepUnsupported);
}

}   // namespace

namespace gpis {
int ws_destroy(gpis_medium *m)
{
    WsHandle *h = as_ws(m);
    if (!h) return GPIS_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    h->tag = 0;
    delete h;
    return GPIS_OK;
}
}   // namespace gpis

extern "C" void gpis_ws_default_params(gpis_ws_params *p)
{
    memset(p, 0, sizeof *p);
    p->version = GPIS_WS_PARAMS_VERSION;
    p->basis_functions = 300;                                  // WSM:26
    p->normal_method = GPIS_NORMAL_CONDITIONED_GAUSSIAN;       // GPM.cpp:93
    p->intersect_method = GPIS_INTERSECT_GP_DISCRETE;          // GPM.cpp:92
}

extern "C" int gpis_ws_create(const gpis_params *params, const gpis_ws_params *ws, int device, gpis_medium **out)
{
    if (!params || !ws || !out) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: null argument");
    *out = nullptr;
    if (int st = ws_validate(*params, *ws)) return st;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return set_err(GPIS_ERR_NO_DEVICE, "gpis_ws_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= count) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_create: device %d of %d", device, count);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return set_err(GPIS_ERR_NO_DEVICE, "gpis_ws_create: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);

    WsHandle *h = new (std::nothrow) WsHandle();
    if (!h) return set_err(GPIS_ERR_DEVICE, "out of host memory");
    h->device = device;
    h->params = *params;
    h->wsp = *ws;
    WsModel &W = h->host;
    if (int st = host_build_model(*params, W.base)) { delete h; return st; }
    W.n = ws->basis_functions;
    W.normal_method = ws->normal_method;
    W.single = params->single_realization != 0;
    W.ctx = params->correlation_context;
    W.seed = params->seed;
    W.min_step = params->min_step;
    W.step_size = params->step_size;
    W.l = params->length_scale;
    for (int c = 0; c < 3; ++c) W.sqrt_aniso[c] = std::sqrt(params->aniso[c]);     // float overload
    W.sqrt2n = W.n > 0 ? std::sqrt(2. / W.n) : 0.;
    W.basis = nullptr;
    int st = GPIS_OK;
    // after the error text is set.  Nothing of this handle can still run on the device: its one launch (k_ws_basis) either failed
    // to launch or was waited for by the hipDeviceSynchronize whose failure brings us here, and hipFree waits in any case
    auto fail = [&](int code) { delete h; return code; };
    if (h->d_model.grow(sizeof(WsModel)) != hipSuccess || h->d_counters.grow(sizeof(WsCounters)) != hipSuccess ||
        hipMemset(h->d_counters.p, 0, sizeof(WsCounters)) != hipSuccess)
        return fail(set_err(GPIS_ERR_DEVICE, "gpis_ws_create: device allocation failed"));
    if (W.single && W.n > 0) {
        if (h->d_basis.grow(6 * (size_t)W.n * sizeof(double)) != hipSuccess)
            return fail(set_err(GPIS_ERR_DEVICE, "gpis_ws_create: device allocation failed"));
        W.basis = h->d_basis.p;
    }
    if (hipMemcpy(h->d_model.p, &W, sizeof W, hipMemcpyHostToDevice) != hipSuccess)
        return fail(set_err(GPIS_ERR_DEVICE, "gpis_ws_create: upload failed"));
    if (W.single && W.n > 0) {
        k_ws_basis<0><<<(W.n + 255) / 256, 256>>>(h->d_model.p, 1, nullptr, h->d_basis.p, 0);     // pss (0,0,0,0)
        if ((st = launch_check("k_ws_basis"))) return fail(st);
        if (hipDeviceSynchronize() != hipSuccess) return fail(set_err(GPIS_ERR_DEVICE, "gpis_ws_create: basis build failed"));
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ws_march<true>, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
    h->grid_cap = (unsigned)(per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1));
    *out = reinterpret_cast<gpis_medium *>(h);
    return GPIS_OK;
}

extern "C" int gpis_ws_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, void *stream)
{
    WS_HANDLE(m);
    if (n && (!rays || !out)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_sample_distance_batch: null pointer");
    std::lock_guard<std::mutex> lock(h->mu);
    return march(h, true, n, rays, out, nullptr, (hipStream_t)stream);
}
extern "C" int gpis_ws_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible, void *stream)
{
    WS_HANDLE(m);
    if (n && (!rays || !visible)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_transmittance_batch: null pointer");
    std::lock_guard<std::mutex> lock(h->mu);
    return march(h, false, n, rays, nullptr, visible, (hipStream_t)stream);
}
extern "C" int gpis_ws_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out)
{
    WS_HANDLE(m);
    if (n && (!rays || !out)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_sample_distance_host: null pointer");
    return march_host(h, true, n, rays, out);
}
extern "C" int gpis_ws_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible)
{
    WS_HANDLE(m);
    if (n && (!rays || !visible)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_transmittance_host: null pointer");
    return march_host(h, false, n, rays, visible);
}
extern "C" int gpis_ws_eval_batch(gpis_medium *m, size_t n, const gpis_ws_query *q, double *value, double *grad3, int32_t *gp_id, void *stream)
{
    WS_HANDLE(m);
    if (n && !q) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_eval_batch: null pointer");
    if (n == 0) return GPIS_OK;
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    const unsigned grid = (unsigned)(n < h->grid_cap ? n : h->grid_cap);
    if (int st = ws_ensure_work(h, grid)) return st;
    k_ws_eval<0><<<grid, 64, 0, (hipStream_t)stream>>>(h->d_model.p, n, q, value, grad3, gp_id, h->d_work.p, h->d_counters.p);
    if (int st = launch_check("k_ws_eval")) return st;
    return ws_check_overflow(h, (hipStream_t)stream);
}
extern "C" int gpis_ws_basis_batch(gpis_medium *m, size_t n, const uint32_t *pss4, double *out, void *stream)
{
    WS_HANDLE(m);
    if (n && (!pss4 || !out)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_basis_batch: null pointer");
    const size_t total = n * (size_t)h->host.n;
    if (total == 0) return GPIS_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t blocks = (total + 255) / 256;
    k_ws_basis<0><<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, (hipStream_t)stream>>>(h->d_model.p, n, pss4, out, 1);
    return launch_check("k_ws_basis");
}
extern "C" int gpis_ws_get_counters(gpis_medium *m, uint64_t *n_eval, uint64_t *n_spec, uint64_t *n_seg)
{
    WS_HANDLE(m);
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    WsCounters c;
    HIP_TRY(hipMemcpy(&c, h->d_counters.p, sizeof c, hipMemcpyDeviceToHost));
    if (n_eval) *n_eval = c.n_eval;
    if (n_spec) *n_spec = c.n_spec;
    if (n_seg) *n_seg = c.n_seg;
    return GPIS_OK;
}
extern "C" int gpis_ws_reset_counters(gpis_medium *m)
{
    WS_HANDLE(m);
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(h->d_counters.p, 0, sizeof(WsCounters)));
    return GPIS_OK;
}
