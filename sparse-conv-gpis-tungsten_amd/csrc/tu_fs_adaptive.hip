// tu_fs_adaptive.hip — gpis_fs_render_scene_s_adaptive and gpis_fs_render_scene_s_paths_adaptive (include/gpis.h): the two frame
// drivers of the function-space GP medium under the adaptive sample schedule.  The pass loop is the one of the other adaptive
// drivers (gpis_adaptive_host.hpp); a chunk of records is one fused launch on the variable-count layout (k_fs_scene_adaptive,
// k_fs_paths_adaptive: tu_fs_scene.hip, tu_fs_paths.hip through gpis_launch.hpp), the per-pixel sum of its sample records and the
// tile statistics (gpis_fs_adaptive.hpp: the bodies of gpis_frame_sum.hpp on this medium's accessors).  Of fs_frame
// (tu_scene.hip) a chunk keeps the reset of the work counter, fs_workspace for the records and the grid cap, and
// grid = min(samples, cap).
#include <hip/hip_runtime.h>

#include "gpis.h"
#include "gpis_adaptive_host.hpp"
#include "gpis_fs_adaptive.hpp"
#include "gpis_host.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

using namespace gpis;
using gpis::launch::grid_of;

namespace {

// What the pass loop takes of a function-space handle.  Its lock for the whole call is fs_host_mu, not mu: fs_workspace takes mu
// itself while it grows the workspace, the records and the counter (as under the uniform entries), so the order is fs_host_mu, then
// mu, the order of the function-space host entries.  Two adaptive calls on one handle, which share the slots, the records and the
// work counter, thereby run one after the other.
struct FsPasses {
    gpis_medium *m;
    std::mutex &mu() const { return m->fs_host_mu; }
    int device() const { return m->device; }
    int chunk_log2() const { return m->opt[GPIS_OPT_CHUNK_LOG2] ? (int)m->opt[GPIS_OPT_CHUNK_LOG2] : 22; }     // as fs_frame
    int acquire(hipStream_t) const { return GPIS_OK; }
    int release(hipStream_t) const { return GPIS_OK; }
    int before_sync(hipStream_t) const { return GPIS_OK; }
    int after_sync(hipStream_t) const { return GPIS_OK; }
};

// The checks both entries share (the entry has checked the pointers and arguments of its own), then the pass loop around `march`
// (grid, scene constants, chunk, samples: the fused launch) followed by the sum and the statistics on `values(scene constants)`.
template <typename March, typename Values>
int fs_adaptive_frame(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, size_t rec_bytes, const char *entry, float *radiance_sum,
                      uint32_t *sample_count, uint32_t *count, gpis_adaptive_record *records, gpis_adaptive_info *info, hipStream_t st, March march,
                      Values values)
{
    if (!scene_args_ok(s)) return set_err(GPIS_ERR_INVALID_ARG, "%s: scene arguments (size, rows, shard)", entry);
    if (int rc = fs_check(m)) return rc;
    const SceneConst sc = make_scene_const(s);
    unsigned cap = 0;
    return adaptive_passes(
        FsPasses{m}, s, a, entry, st, records, info,
        [&](size_t n, bool &fits) {
            if (int rc = fs_workspace(m, cap)) return rc;
            // the work counter runs to at most n + grid
            if (n + cap >= ((size_t)1 << 32)) return set_err(GPIS_ERR_UNSUPPORTED, "%s: a chunk of %zu samples", entry, n);
            fits = true;
            return fs_workspace(m, cap, n * rec_bytes);
        },
        [&]() { return (int)GPIS_OK; },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            HIP_TRY(hipMemsetAsync(m->fs_scene_next.p, 0, sizeof(uint32_t), st));
            if (int rc = march((unsigned)(ns < cap ? ns : cap), sc, ch, (uint32_t)ns)) return rc;
            const auto v = values(sc);
            k_fs_adaptive_sum<<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(sc, ch, v, radiance_sum, sample_count, count);
            if (int rc = launch_check("k_fs_adaptive_sum")) return rc;
            k_fs_adaptive_stats<<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, v, d_records);
            return launch_check("k_fs_adaptive_stats");
        });
}

}   // namespace

extern "C" int gpis_fs_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, float *radiance_sum, uint32_t *sample_count,
                                               uint32_t *hit_count, gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && radiance_sum && sample_count);
    hipStream_t st = (hipStream_t)stream;
    return fs_adaptive_frame(
        m, s, a, launch::fs_scene_rec_bytes(), __func__, radiance_sum, sample_count, hit_count, records, info, st,
        [&](unsigned grid, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t ns) {
            launch::fs_scene_adaptive(grid, m->d_model.p, sc, ch, ns, m->fs_scene_next.p, m->fs_scene_recs.p, m->fs_ws.p, m->fs_slots, st);
            return launch_check("k_fs_scene_adaptive");
        },
        [&](const SceneConst &sc) { return FsSceneValues{(const FsSceneRec *)m->fs_scene_recs.p, sc.s.light_radiance}; });
}

// The second bank of state slots holds the shadow segments' copies, as under gpis_fs_render_scene_s_paths.
extern "C" int gpis_fs_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int max_path_bounces, float albedo,
                                                     float *radiance_sum, uint32_t *sample_count, uint32_t *seg_count, gpis_adaptive_record *records,
                                                     gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && radiance_sum && sample_count && max_path_bounces >= 1);
    hipStream_t st = (hipStream_t)stream;
    return fs_adaptive_frame(
        m, s, a, launch::fs_paths_rec_bytes(), __func__, radiance_sum, sample_count, seg_count, records, info, st,
        [&](unsigned grid, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t ns) {
            launch::fs_paths_adaptive(grid, m->d_model.p, sc, ch, ns, max_path_bounces, albedo, m->fs_scene_next.p, m->fs_scene_recs.p, m->fs_ws.p,
                                      m->fs_slots, m->fs_slots + m->fs_ws_blocks, st);
            return launch_check("k_fs_paths_adaptive");
        },
        [&](const SceneConst &) { return FsPathsValues{(const FsPathsRec *)m->fs_scene_recs.p}; });
}
