// gpis_ws_host.hpp — host side of a weight-space handle, shared by the translation units that implement gpis_ws_* entries
// (tu_ws.hip: handle, batch entries; tu_ws_scene.hip: the scene-S frame driver; tu_ws_paths.hip: the multi-bounce path driver;
// tu_ws_adaptive.hip: both under the adaptive sample schedule).
//
// A weight-space handle is its own object (WsHandle) behind the opaque gpis_medium pointer; its first word is kWsHandleTag,
// where a sparse-convolution handle holds gpis_params::abi_version, so either family of entries can refuse the other's handles.
// Errors, buffers and the *_host round trip are the common ones of gpis_host_base.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "gpis.h"
#include "gpis_host_base.hpp"     // set_err, HIP_TRY, launch_check; DevBuf; host_round_trip
#include "gpis_scene.hpp"
#include "gpis_ws.hpp"

namespace gpis {
// gpis_hip.hip
int host_build_model(const gpis_params &P, DevModel &M);
bool ws_is_handle(const void *m);
int ws_destroy(gpis_medium *m);

struct WsHandle {                         // owns its buffers: deleting it frees them (ws_destroy, the failure paths of gpis_ws_create)
    uint32_t tag = kWsHandleTag;          // must stay the first member
    int device = 0;
    gpis_params params{};
    gpis_ws_params wsp{};
    WsModel host{};
    DevBuf<WsModel> d_model;
    DevBuf<WsCounters> d_counters;
    DevBuf<double> d_basis;               // single realization: [6][N]
    DevBuf<double> d_work;                // per-path realizations: one [6][N] slice per resident workgroup
    unsigned grid_cap = 0;                // resident one-wave workgroups of k_ws_march on this device
    unsigned scene_grid_cap = 0;          // ... of k_ws_scene (tu_ws_scene.hip; 0 until the first frame)
    unsigned paths_grid_cap = 0;          // ... of k_ws_paths (tu_ws_paths.hip; 0 until the first frame)
    unsigned scene_adaptive_grid_cap = 0, paths_adaptive_grid_cap = 0;     // ... of k_ws_scene_adaptive, k_ws_paths_adaptive (tu_ws_adaptive.hip)
    DevBuf<unsigned> d_scene_next;        // the frame drivers' work counter (k_ws_scene, k_ws_paths): the next sample of the chunk
    std::mutex mu;                        // serialises the entries of one handle (workspace, staging, counters)
    DevBuf<> stage[3];                    // 0, 1: the *_host entries' rays / results; 2: the frame drivers' sample records
};

inline WsHandle *as_ws(gpis_medium *m) { return ws_is_handle(m) ? reinterpret_cast<WsHandle *>(m) : nullptr; }

#define WS_HANDLE(m)                                                                                            \
    WsHandle *h = as_ws(m);                                                                                     \
    if (!h) return set_err(GPIS_ERR_INVALID_ARG, "%s: not a weight-space handle (gpis_ws_create)", __func__)

// the per-path workspace: one realization slice per resident workgroup
inline int ws_ensure_work(WsHandle *h, unsigned blocks)
{
    const size_t bytes = (size_t)blocks * 6 * (size_t)h->host.n * sizeof(double);
    if (h->host.single || h->host.n == 0 || h->d_work.bytes >= bytes) return GPIS_OK;
    if (h->d_work.p) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(h->d_work.grow(bytes));
    return GPIS_OK;
}

// the arguments of cos / sin stayed inside the restated range (include/gpis.h): read after the stream drained (ws_check_overflow);
// in two steps for a caller with a synchronisation of its own (the adaptive pass loop): the read, enqueued ahead of it, and the verdict
inline int ws_read_overflow(WsHandle *h, unsigned long long *ov, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(ov, &h->d_counters.p->arg_overflow, sizeof *ov, hipMemcpyDeviceToHost, s));
    return GPIS_OK;
}
inline int ws_overflow_verdict(WsHandle *h, unsigned long long ov, hipStream_t s)
{
    if (ov) {
        HIP_TRY(hipMemsetAsync(&h->d_counters.p->arg_overflow, 0, sizeof ov, s));
        HIP_TRY(hipStreamSynchronize(s));
        return set_err(GPIS_ERR_UNSUPPORTED, "weight-space medium: a cos / sin argument reached |x| >= 105414350, where glibc's large-argument "
                                            "reduction (not restated on the device) applies; the results of this call are not valid");
    }
    return GPIS_OK;
}
inline int ws_check_overflow(WsHandle *h, hipStream_t s)
{
    unsigned long long ov = 0;
    if (int rc = ws_read_overflow(h, &ov, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return ws_overflow_verdict(h, ov, s);
}

// grid_cap: the handle's count of resident one-wave workgroups of a fused frame kernel, queried on the kernel's first frame
template <typename Kernel>
inline int ws_grid_cap(WsHandle *h, Kernel kernel, unsigned &grid_cap)
{
    if (!grid_cap) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, h->device));
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
        grid_cap = (unsigned)(per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1));
    }
    return GPIS_OK;
}

// The frame loop of the weight-space scene-S drivers (tu_ws_scene.hip, tu_ws_paths.hip), under the handle's lock: per chunk of
// samples one fused launch (`march`: grid, first pixel, samples, records) and the per-pixel sum of its records (`sum`: first
// pixel, pixels, records); each launches and returns its launch_check.  The record array is 8 B per sample at most (32 MB a
// chunk), and a chunk fills the grid of resident waves (2048) two thousand times over; frames of this medium are about 10^6
// samples (about 1 M segments/s), so most frames are one chunk.  grid_cap: the handle's count of resident one-wave workgroups
// of `kernel` (ws_grid_cap).  `entry` names the caller in messages.
template <typename Kernel, typename March, typename Sum>
inline int ws_frame(WsHandle *h, const gpis_scene_s *s, size_t rec_bytes, const char *entry, Kernel kernel, unsigned &grid_cap, hipStream_t st, March march, Sum sum)
{
    constexpr size_t kFrameChunk = (size_t)1 << 22;      // samples per chunk
    const size_t total_pixels = scene_rows(*s) * s->width;
    if (total_pixels == 0) return GPIS_OK;
    if (int rc = ws_grid_cap(h, kernel, grid_cap)) return rc;
    HIP_TRY(h->d_scene_next.grow(sizeof(uint32_t)));
    size_t chunk_pixels = kFrameChunk / s->spp_count;
    if (chunk_pixels < 1) chunk_pixels = 1;
    if (chunk_pixels > total_pixels) chunk_pixels = total_pixels;
    const size_t ns_max = chunk_pixels * s->spp_count;
    if (ns_max + grid_cap >= ((size_t)1 << 32)) return set_err(GPIS_ERR_UNSUPPORTED, "%s: spp_count %u", entry, s->spp_count);
    if (int rc = GrowStage{h->stage}(2, ns_max * rec_bytes)) return rc;
    void *recs = h->stage[2].p;
    const unsigned grid = (unsigned)(ns_max < grid_cap ? ns_max : grid_cap);
    if (int rc = ws_ensure_work(h, grid)) return rc;
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        HIP_TRY(hipMemsetAsync(h->d_scene_next.p, 0, sizeof(uint32_t), st));
        if (int rc = march((unsigned)(ns < grid ? ns : grid), p0, (uint32_t)ns, recs)) return rc;
        if (int rc = sum(p0, np, recs)) return rc;
    }
    return ws_check_overflow(h, st);
}

}   // namespace gpis
