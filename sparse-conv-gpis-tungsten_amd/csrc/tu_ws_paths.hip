// tu_ws_paths.hip — gpis_ws_render_scene_s_paths (include/gpis.h): multi-bounce paths on scene S through the weight-space GP
// medium, one fused kernel per chunk of samples (gpis_ws_paths.hpp) and a per-pixel sum of the sample records in sample order.
#include <hip/hip_runtime.h>

#include "gpis.h"
#include "gpis_ws_host.hpp"
#include "gpis_ws_paths.hpp"

#pragma clang fp contract(off)

using namespace gpis;

namespace {

// Samples per chunk, as the scene driver's (tu_ws_scene.hip): the record array is 4 B per sample (16 MB).
constexpr size_t kPathsChunk = (size_t)1 << 22;

}   // namespace

extern "C" int gpis_ws_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo, float *radiance_sum,
                                            void *stream)
{
    WS_HANDLE(m);
    if (!s || !radiance_sum) return ws_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: null pointer");
    if (max_path_bounces < 1) return ws_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: max_path_bounces %d", max_path_bounces);
    if (!scene_args_ok(s)) return ws_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: scene arguments (size, rows, shard)");
    std::lock_guard<std::mutex> lock(h->mu);
    WS_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    if (total_pixels == 0) return GPIS_OK;
    if (!h->paths_grid_cap) {
        hipDeviceProp_t prop;
        WS_HIP_TRY(hipGetDeviceProperties(&prop, h->device));
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_ws_paths<0>, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
        h->paths_grid_cap = (unsigned)(per_cu * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1));
    }
    if (!h->d_scene_next) WS_HIP_TRY(hipMalloc(&h->d_scene_next, sizeof(uint32_t)));
    size_t chunk_pixels = kPathsChunk / s->spp_count;
    if (chunk_pixels < 1) chunk_pixels = 1;
    if (chunk_pixels > total_pixels) chunk_pixels = total_pixels;
    const size_t ns_max = chunk_pixels * s->spp_count;
    if (ns_max + h->paths_grid_cap >= ((size_t)1 << 32)) return ws_err(GPIS_ERR_UNSUPPORTED, "gpis_ws_render_scene_s_paths: spp_count %u", s->spp_count);
    if (int rc = ws_stage(h, 2, ns_max * sizeof(WsPathsRec))) return rc;
    WsPathsRec *recs = (WsPathsRec *)h->stage[2];
    const unsigned grid = (unsigned)(ns_max < h->paths_grid_cap ? ns_max : h->paths_grid_cap);
    if (int rc = ws_ensure_work(h, grid)) return rc;
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        WS_HIP_TRY(hipMemsetAsync(h->d_scene_next, 0, sizeof(uint32_t), st));
        k_ws_paths<0><<<(unsigned)(ns < grid ? ns : grid), 64, 0, st>>>(h->d_model, sc, p0, (uint32_t)ns, max_path_bounces, albedo, h->d_scene_next, recs,
                                                                       h->d_work, h->d_counters);
        if (int rc = ws_launch_check("k_ws_paths")) return rc;
        k_ws_paths_sum<0><<<(unsigned)((np + 255) / 256), 256, 0, st>>>(sc, p0, np, recs, radiance_sum);
        if (int rc = ws_launch_check("k_ws_paths_sum")) return rc;
    }
    return ws_check_overflow(h, st);
}
