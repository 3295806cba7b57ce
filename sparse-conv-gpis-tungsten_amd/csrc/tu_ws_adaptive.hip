// tu_ws_adaptive.hip — gpis_ws_render_scene_s_adaptive and gpis_ws_render_scene_s_paths_adaptive (include/gpis.h): the two frame
// drivers of the weight-space GP medium under the adaptive sample schedule.  The pass loop is the one of the sparse-convolution
// adaptive drivers (gpis_adaptive_host.hpp); a chunk of records is one fused launch on the variable-count layout
// (k_ws_scene_adaptive, k_ws_paths_adaptive), the per-pixel sum of its sample records and the tile statistics
// (gpis_ws_adaptive.hpp).  Of ws_frame (gpis_ws_host.hpp) a chunk keeps the grid cap by the kernel's occupancy, the reset of the
// work counter, stage[2] for the sample records and the per-path workspace.
#include <hip/hip_runtime.h>

#include "gpis.h"
#include "gpis_adaptive_host.hpp"
#include "gpis_launch.hpp"
#include "gpis_ws_adaptive.hpp"
#include "gpis_ws_host.hpp"

#pragma clang fp contract(off)

using namespace gpis;
using gpis::launch::grid_of;

namespace {

// what the pass loop takes of a weight-space handle: its lock and device, the entry's chunk_log2, and the cos / sin argument-range
// check read at each pass's synchronisation
struct WsPasses {
    WsHandle *h;
    int log2;
    unsigned long long *overflow;          // the caller's, alive for the whole call
    std::mutex &mu() const { return h->mu; }
    int device() const { return h->device; }
    int chunk_log2() const { return log2; }
    int acquire(hipStream_t) const { return GPIS_OK; }
    int release(hipStream_t) const { return GPIS_OK; }
    int before_sync(hipStream_t st) const { return ws_read_overflow(h, overflow, st); }
    int after_sync(hipStream_t st) const { return ws_overflow_verdict(h, *overflow, st); }
};

// The arguments both entries share (the entry has checked its handle and the pointers of its own), then the pass loop around
// `march` (grid, chunk, samples, records: the fused launch) followed by the sum and the statistics on `values(records)`.
template <typename Rec, typename Kernel, typename March, typename Values>
int ws_adaptive_frame(WsHandle *h, const gpis_scene_s *s, const gpis_adaptive_s *a, int chunk_log2, const char *entry, Kernel kernel, unsigned &grid_cap,
                      float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count, gpis_adaptive_record *records, gpis_adaptive_info *info,
                      hipStream_t st, March march, Values values)
{
    if (!scene_args_ok(s)) return set_err(GPIS_ERR_INVALID_ARG, "%s: scene arguments (size, rows, shard)", entry);
    if (chunk_log2 != 0 && (chunk_log2 < 8 || chunk_log2 > 28)) return set_err(GPIS_ERR_INVALID_ARG, "%s: chunk_log2 %d (0, 8 .. 28)", entry, chunk_log2);
    const SceneConst sc = make_scene_const(s);
    unsigned long long overflow = 0;
    unsigned grid = 0;
    Rec *recs = nullptr;
    return adaptive_passes(
        WsPasses{h, chunk_log2 ? chunk_log2 : 22, &overflow}, s, a, entry, st, records, info,
        [&](size_t n, bool &fits) {
            if (int rc = ws_grid_cap(h, kernel, grid_cap)) return rc;
            if (n + grid_cap >= ((size_t)1 << 32)) return set_err(GPIS_ERR_UNSUPPORTED, "%s: a chunk of %zu samples", entry, n);
            HIP_TRY(h->d_scene_next.grow(sizeof(uint32_t)));
            if (int rc = GrowStage{h->stage}(2, n * sizeof(Rec))) return rc;
            grid = (unsigned)(n < grid_cap ? n : grid_cap);
            fits = true;
            return ws_ensure_work(h, grid);
        },
        [&]() {
            recs = (Rec *)h->stage[2].p;
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            HIP_TRY(hipMemsetAsync(h->d_scene_next.p, 0, sizeof(uint32_t), st));
            if (int rc = march((unsigned)(ns < grid ? ns : grid), sc, ch, (uint32_t)ns, recs)) return rc;
            const auto v = values(sc, recs);
            k_ws_adaptive_sum<<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(sc, ch, v, radiance_sum, sample_count, hit_count);
            if (int rc = launch_check("k_ws_adaptive_sum")) return rc;
            k_ws_adaptive_stats<<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, v, d_records);
            return launch_check("k_ws_adaptive_stats");
        });
}

}   // namespace

extern "C" int gpis_ws_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int chunk_log2, float *radiance_sum,
                                               uint32_t *sample_count, uint32_t *hit_count, gpis_adaptive_record *records, gpis_adaptive_info *info,
                                               void *stream)
{
    WS_HANDLE(m);
    if (!s || !a || !radiance_sum || !sample_count) return set_err(GPIS_ERR_INVALID_ARG, "%s: null pointer", __func__);
    hipStream_t st = (hipStream_t)stream;
    return ws_adaptive_frame<WsSceneRec>(
        h, s, a, chunk_log2, __func__, k_ws_scene_adaptive<0>, h->scene_adaptive_grid_cap, radiance_sum, sample_count, hit_count, records, info, st,
        [&](unsigned grid, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t ns, WsSceneRec *recs) {
            k_ws_scene_adaptive<0><<<grid, 64, 0, st>>>(h->d_model.p, sc, ch, ns, h->d_scene_next.p, recs, h->d_work.p, h->d_counters.p);
            return launch_check("k_ws_scene_adaptive");
        },
        [](const SceneConst &sc, const WsSceneRec *recs) { return WsSceneValues{recs, sc.s.light_radiance}; });
}

extern "C" int gpis_ws_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int chunk_log2, int max_path_bounces,
                                                     float albedo, float *radiance_sum, uint32_t *sample_count, gpis_adaptive_record *records,
                                                     gpis_adaptive_info *info, void *stream)
{
    WS_HANDLE(m);
    if (!s || !a || !radiance_sum || !sample_count) return set_err(GPIS_ERR_INVALID_ARG, "%s: null pointer", __func__);
    if (max_path_bounces < 1) return set_err(GPIS_ERR_INVALID_ARG, "%s: max_path_bounces %d", __func__, max_path_bounces);
    hipStream_t st = (hipStream_t)stream;
    return ws_adaptive_frame<WsPathsRec>(
        h, s, a, chunk_log2, __func__, k_ws_paths_adaptive<0>, h->paths_adaptive_grid_cap, radiance_sum, sample_count, nullptr, records, info, st,
        [&](unsigned grid, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t ns, WsPathsRec *recs) {
            k_ws_paths_adaptive<0><<<grid, 64, 0, st>>>(h->d_model.p, sc, ch, ns, max_path_bounces, albedo, h->d_scene_next.p, recs, h->d_work.p,
                                                        h->d_counters.p);
            return launch_check("k_ws_paths_adaptive");
        },
        [](const SceneConst &, const WsPathsRec *recs) { return WsPathsValues{recs}; });
}
