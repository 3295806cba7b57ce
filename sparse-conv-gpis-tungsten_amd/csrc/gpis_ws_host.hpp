// gpis_ws_host.hpp — host side of a weight-space handle, shared by the translation units that implement gpis_ws_* entries
// (tu_ws.hip: handle, batch entries; tu_ws_scene.hip: the scene-S frame driver; tu_ws_paths.hip: the multi-bounce path driver).
//
// A weight-space handle is its own object (WsHandle) behind the opaque gpis_medium pointer; its first word is kWsHandleTag,
// where a sparse-convolution handle holds gpis_params::abi_version, so either family of entries can refuse the other's handles.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "gpis.h"
#include "gpis_scene.hpp"
#include "gpis_ws.hpp"

namespace gpis {
// gpis_hip.hip
int host_build_model(const gpis_params &P, DevModel &M);
int host_set_err(int code, const char *msg);
bool ws_is_handle(const void *m);
int ws_destroy(gpis_medium *m);

struct WsHandle {
    uint32_t tag = kWsHandleTag;          // must stay the first member
    int device = 0;
    gpis_params params{};
    gpis_ws_params wsp{};
    WsModel host{};
    WsModel *d_model = nullptr;
    WsCounters *d_counters = nullptr;
    double *d_basis = nullptr;            // single realization: [6][N]
    double *d_work = nullptr;             // per-path realizations: one [6][N] slice per resident workgroup
    unsigned work_blocks = 0;
    unsigned grid_cap = 0;                // resident one-wave workgroups of k_ws_march on this device
    unsigned scene_grid_cap = 0;          // ... of k_ws_scene (tu_ws_scene.hip; 0 until the first frame)
    unsigned paths_grid_cap = 0;          // ... of k_ws_paths (tu_ws_paths.hip; 0 until the first frame)
    unsigned *d_scene_next = nullptr;     // the frame drivers' work counter (k_ws_scene, k_ws_paths): the next sample of the chunk
    std::mutex mu;                        // serialises the entries of one handle (workspace, staging, counters)
    void *stage[3] = {nullptr, nullptr, nullptr};     // 0, 1: the *_host entries' rays / results; 2: the frame drivers' sample records
    size_t stage_bytes[3] = {0, 0, 0};
};

inline int ws_err(int code, const char *fmt, ...)
{
    char buf[480];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return host_set_err(code, buf);
}

#define WS_HIP_TRY(expr)                                                                                              \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return ws_err(GPIS_ERR_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline WsHandle *as_ws(gpis_medium *m) { return ws_is_handle(m) ? reinterpret_cast<WsHandle *>(m) : nullptr; }

#define WS_HANDLE(m)                                                                                            \
    WsHandle *h = as_ws(m);                                                                                     \
    if (!h) return ws_err(GPIS_ERR_INVALID_ARG, "%s: not a weight-space handle (gpis_ws_create)", __func__)

inline int ws_launch_check(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ws_err(GPIS_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
    return GPIS_OK;
}

// the per-path workspace: one realization slice per resident workgroup
inline int ws_ensure_work(WsHandle *h, unsigned blocks)
{
    if (h->host.single || h->host.n == 0 || h->work_blocks >= blocks) return GPIS_OK;
    if (h->d_work) { WS_HIP_TRY(hipDeviceSynchronize()); WS_HIP_TRY(hipFree(h->d_work)); h->d_work = nullptr; h->work_blocks = 0; }
    WS_HIP_TRY(hipMalloc(&h->d_work, (size_t)blocks * 6 * (size_t)h->host.n * sizeof(double)));
    h->work_blocks = blocks;
    return GPIS_OK;
}

// the arguments of cos / sin stayed inside the restated range (include/gpis.h): read after the stream drained
inline int ws_check_overflow(WsHandle *h, hipStream_t s)
{
    unsigned long long ov = 0;
    WS_HIP_TRY(hipMemcpyAsync(&ov, &h->d_counters->arg_overflow, sizeof ov, hipMemcpyDeviceToHost, s));
    WS_HIP_TRY(hipStreamSynchronize(s));
    if (ov) {
        WS_HIP_TRY(hipMemsetAsync(&h->d_counters->arg_overflow, 0, sizeof ov, s));
        WS_HIP_TRY(hipStreamSynchronize(s));
        return ws_err(GPIS_ERR_UNSUPPORTED, "weight-space medium: a cos / sin argument reached |x| >= 105414350, where glibc's large-argument "
                                            "reduction (not restated on the device) applies; the results of this call are not valid");
    }
    return GPIS_OK;
}

inline int ws_stage(WsHandle *h, int k, size_t bytes)
{
    if (h->stage_bytes[k] >= bytes) return GPIS_OK;
    if (h->stage[k]) { WS_HIP_TRY(hipFree(h->stage[k])); h->stage[k] = nullptr; h->stage_bytes[k] = 0; }
    const size_t cap = bytes + bytes / 4 + 4096;
    WS_HIP_TRY(hipMalloc(&h->stage[k], cap));
    h->stage_bytes[k] = cap;
    return GPIS_OK;
}

// The frame loop of the weight-space scene-S drivers (tu_ws_scene.hip, tu_ws_paths.hip), under the handle's lock: per chunk of
// samples one fused launch (`march`: grid, first pixel, samples, records) and the per-pixel sum of its records (`sum`: first
// pixel, pixels, records); each launches and returns its ws_launch_check.  The record array is 8 B per sample at most (32 MB a
// chunk), and a chunk fills the grid of resident waves (2048) two thousand times over; frames of this medium are about 10^6
// samples (about 1 M segments/s), so most frames are one chunk.  grid_cap: the handle's count of resident one-wave workgroups
// of `kernel`, queried on the first frame.  `entry` names the caller in messages.
template <typename Kernel, typename March, typename Sum>
inline int ws_frame(WsHandle *h, const gpis_scene_s *s, size_t rec_bytes, const char *entry, Kernel kernel, unsigned &grid_cap, hipStream_t st, March march, Sum sum)
{
    constexpr size_t kFrameChunk = (size_t)1 << 22;      // samples per chunk
    const size_t total_pixels = scene_rows(*s) * s->width;
    if (total_pixels == 0) return GPIS_OK;
    if (!grid_cap) {
        hipDeviceProp_t prop;
        WS_HIP_TRY(hipGetDeviceProperties(&prop, h->device));
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
        grid_cap = (unsigned)(per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1));
    }
    if (!h->d_scene_next) WS_HIP_TRY(hipMalloc(&h->d_scene_next, sizeof(uint32_t)));
    size_t chunk_pixels = kFrameChunk / s->spp_count;
    if (chunk_pixels < 1) chunk_pixels = 1;
    if (chunk_pixels > total_pixels) chunk_pixels = total_pixels;
    const size_t ns_max = chunk_pixels * s->spp_count;
    if (ns_max + grid_cap >= ((size_t)1 << 32)) return ws_err(GPIS_ERR_UNSUPPORTED, "%s: spp_count %u", entry, s->spp_count);
    if (int rc = ws_stage(h, 2, ns_max * rec_bytes)) return rc;
    void *recs = h->stage[2];
    const unsigned grid = (unsigned)(ns_max < grid_cap ? ns_max : grid_cap);
    if (int rc = ws_ensure_work(h, grid)) return rc;
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        WS_HIP_TRY(hipMemsetAsync(h->d_scene_next, 0, sizeof(uint32_t), st));
        if (int rc = march((unsigned)(ns < grid ? ns : grid), p0, (uint32_t)ns, recs)) return rc;
        if (int rc = sum(p0, np, recs)) return rc;
    }
    return ws_check_overflow(h, st);
}

}   // namespace gpis
