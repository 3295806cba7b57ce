// tu_ws_paths.hip — gpis_ws_render_scene_s_paths (include/gpis.h): multi-bounce paths on scene S through the weight-space GP
// medium, one fused kernel per chunk of samples (gpis_ws_paths.hpp) and a per-pixel sum of the sample records in sample order.
#include <hip/hip_runtime.h>

#include "gpis.h"
#include "gpis_ws_host.hpp"
#include "gpis_ws_paths.hpp"

#pragma clang fp contract(off)

using namespace gpis;

extern "C" int gpis_ws_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo, float *radiance_sum,
                                            void *stream)
{
    WS_HANDLE(m);
    if (!s || !radiance_sum) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: null pointer");
    if (max_path_bounces < 1) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: max_path_bounces %d", max_path_bounces);
    if (!scene_args_ok(s)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s_paths: scene arguments (size, rows, shard)");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    return ws_frame(h, s, sizeof(WsPathsRec), __func__, k_ws_paths<0>, h->paths_grid_cap, st,
                    [&](unsigned grid, size_t p0, uint32_t ns, void *recs) {
                        k_ws_paths<0><<<grid, 64, 0, st>>>(h->d_model.p, sc, p0, ns, max_path_bounces, albedo, h->d_scene_next.p, (WsPathsRec *)recs, h->d_work.p,
                                                         h->d_counters.p);
                        return launch_check("k_ws_paths");
                    },
                    [&](size_t p0, size_t np, const void *recs) {
                        k_ws_paths_sum<0><<<(unsigned)((np + 255) / 256), 256, 0, st>>>(sc, p0, np, (const WsPathsRec *)recs, radiance_sum);
                        return launch_check("k_ws_paths_sum");
                    });
}
