// gpis_adaptive_host.hpp — the pass loop of the adaptive frame drivers, stated once for both families of handles
// (include/gpis.h at gpis_render_scene_s_adaptive; gpis_adaptive.hpp: the sample layout; tu_adaptive.hip: the plan step).
// tu_scene.hip runs it on a sparse-convolution handle (gpis_render_scene_s_adaptive, gpis_render_scene_s_paths_rgb_adaptive),
// tu_ws_adaptive.hip on a weight-space one (gpis_ws_render_scene_s_adaptive, gpis_ws_render_scene_s_paths_adaptive).
// tu_fs_adaptive.hip runs it on the function-space side of a gpis_create handle (gpis_fs_render_scene_s_adaptive,
// gpis_fs_render_scene_s_paths_adaptive).
//
// Per pass: the plan step on the host, its (offset, sample_index, count) table to the device, then chunks of whole records through
// the driver's own stages, which end with its tile statistics into the device records; the records come back for the next plan
// step, which is the pass's one synchronisation.  What belongs to the handle comes in as `host`:
//   host.mu(), host.device():   the handle's lock, held for the whole call, and its device;
//   host.chunk_log2():          samples per chunk, as a power of two;
//   host.acquire(st), host.release(st): around the passes (the workspace of a sparse-convolution handle);
//   host.before_sync(st):       enqueued behind a pass's last chunk, ahead of the pass's synchronisation;
//   host.after_sync(st):        what that synchronisation brought back; a non-zero status ends the call with it.
// The driver passes
//   size(n, fits): lay out (and, if it wants, allocate) its workspace for chunks of up to n samples; fits = the device holds it;
//   bind():        called once per pass after the table's upload: allocate what `size` planned and take the pointers;
//   render(ch, ns, d_records): the stages of the chunk `ch` of ns samples.
// Chunks hold 2^host.chunk_log2() samples (at most the pass), halved until the device holds the workspace; a record larger than that
// is a chunk of its own.  The entry has checked the arguments of its own; `entry` names it in messages.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "gpis.h"
#include "gpis_adaptive.hpp"
#include "gpis_host_base.hpp"     // set_err, HIP_TRY

namespace gpis {

struct DeviceArray {                   // hipMalloc for the length of one call
    void *p = nullptr;
    ~DeviceArray() { if (p) (void)hipFree(p); }
};

template <typename Host, typename Size, typename Bind, typename Render>
inline int adaptive_passes(Host host, const gpis_scene_s *s, const gpis_adaptive_s *a, const char *entry, hipStream_t st, gpis_adaptive_record *records,
                           gpis_adaptive_info *info, Size size, Bind bind, Render render)
{
    const uint32_t vw = (s->width + kVarianceTile - 1) / kVarianceTile, vh = (s->height + kVarianceTile - 1) / kVarianceTile;
    const size_t n_rec = (size_t)vw * vh;
#define ADAPTIVE_ARGS(cond)                                                                                        \
    do {                                                                                                           \
        if (!(cond)) return set_err(GPIS_ERR_INVALID_ARG, "%s: invalid argument (%s)", entry, #cond);              \
    } while (0)
    ADAPTIVE_ARGS(s->y_begin == 0 && s->y_count == s->height && s->shard_count <= 1u);
    ADAPTIVE_ARGS(a->spp_step > 0 && a->threshold >= 2);
    ADAPTIVE_ARGS(n_rec < 0xFFFFFFFFull);
#undef ADAPTIVE_ARGS
    std::lock_guard<std::mutex> lock(host.mu());
    HIP_TRY(hipSetDevice(host.device()));
    std::vector<gpis_adaptive_record> rec(n_rec, gpis_adaptive_record{0, 0, 0, 0.f, 0.f, 0.f}), rec_dev(n_rec);
    std::vector<AdaptivePlanRec> plan(n_rec + 1);
    DeviceArray d_rec, d_plan;
    HIP_TRY(hipMalloc(&d_rec.p, n_rec * sizeof(gpis_adaptive_record)));
    HIP_TRY(hipMalloc(&d_plan.p, (n_rec + 1) * sizeof(AdaptivePlanRec)));
    HIP_TRY(hipMemsetAsync(d_rec.p, 0, n_rec * sizeof(gpis_adaptive_record), st));
    uint64_t rng = gpis_adaptive_rng_init_host(a, s->width, s->height);
    gpis_adaptive_info done = {0, 0, 0};
    const size_t chunk_max = (size_t)1 << 28;          // the largest chunk_log2; one record may not hold more
    int rc = GPIS_OK;
    if ((rc = host.acquire(st))) return rc;
    for (uint32_t cur = 0; cur < s->spp_count;) {
        const uint32_t next = s->spp_count - cur < a->spp_step ? s->spp_count : cur + a->spp_step;
        const int go = gpis_adaptive_plan_host(a, s->width, s->height, cur, next - cur, &rng, n_rec, rec.data());
        if (go < 0) return go;
        if (go == 0) { done.stopped_early = 1; break; }
        size_t total = 0, largest = 0;
        for (size_t r = 0; r < n_rec; ++r) {
            const AdaptiveTile t = adaptive_tile(s->width, s->height, (uint32_t)r);
            const size_t n = (size_t)t.w * t.h * rec[r].next_sample_count;
            if (rec[r].next_sample_count == 0 || n > chunk_max)
                return set_err(GPIS_ERR_UNSUPPORTED, "%s: record %zu plans %u samples per pixel in one pass (1 .. 2^28 / 16)", entry, r, rec[r].next_sample_count);
            plan[r] = AdaptivePlanRec{total, rec[r].sample_index, rec[r].next_sample_count};
            total += n;
            if (n > largest) largest = n;
        }
        plan[n_rec] = AdaptivePlanRec{total, 0, 0};
        size_t chunk = 0;
        for (int l = host.chunk_log2();; --l) {
            chunk = (size_t)1 << l;
            if (chunk > total) chunk = total;
            const size_t ns_max = chunk > largest ? chunk : largest;
            bool fits = false;
            if ((rc = size(ns_max, fits))) return rc;
            if (fits) break;
            if (l <= 16 || chunk <= largest) return set_err(GPIS_ERR_DEVICE, "%s: no memory for a workspace of %zu samples", entry, ns_max);
        }
        HIP_TRY(hipMemcpyAsync(d_plan.p, plan.data(), (n_rec + 1) * sizeof(AdaptivePlanRec), hipMemcpyHostToDevice, st));
        if ((rc = bind())) return rc;
        for (size_t r0 = 0; r0 < n_rec;) {
            size_t r1 = r0 + 1;                             // records [r0, r1): as many as the chunk holds, at least one
            while (r1 < n_rec && plan[r1 + 1].offset - plan[r0].offset <= chunk) ++r1;
            const size_t ns = (size_t)(plan[r1].offset - plan[r0].offset);
            const AdaptiveChunk ch{(const AdaptivePlanRec *)d_plan.p, (uint32_t)r0, (uint32_t)(r1 - r0)};
            if ((rc = render(ch, ns, (gpis_adaptive_record *)d_rec.p))) return rc;
            r0 = r1;
        }
        HIP_TRY(hipMemcpyAsync(rec_dev.data(), d_rec.p, n_rec * sizeof(gpis_adaptive_record), hipMemcpyDeviceToHost, st));
        if ((rc = host.before_sync(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if ((rc = host.after_sync(st))) return rc;
        for (size_t r = 0; r < n_rec; ++r) {                 // the device keeps the statistics, the host the schedule
            rec[r].sample_count = rec_dev[r].sample_count;
            rec[r].mean = rec_dev[r].mean;
            rec[r].running_variance = rec_dev[r].running_variance;
        }
        ++done.passes_rendered;
        done.samples += total;
        cur = next;
    }
    if (!done.stopped_early)
        for (size_t r = 0; r < n_rec; ++r)
            rec[r].sample_index += rec[r].next_sample_count;
    if ((rc = host.release(st))) return rc;
    if (records) HIP_TRY(hipMemcpyAsync(records, rec.data(), n_rec * sizeof(gpis_adaptive_record), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info) *info = done;
    return GPIS_OK;
}

}   // namespace gpis
