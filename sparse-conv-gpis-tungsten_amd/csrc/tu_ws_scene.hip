// tu_ws_scene.hip — gpis_ws_render_scene_s (include/gpis.h): scene S through the weight-space GP medium, one fused kernel per
// chunk of samples (gpis_ws_scene.hpp) and a per-pixel sum of the sample records in sample order.
#include <hip/hip_runtime.h>

#include "gpis.h"
#include "gpis_ws_host.hpp"
#include "gpis_ws_scene.hpp"

#pragma clang fp contract(off)

using namespace gpis;

extern "C" int gpis_ws_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum, uint32_t *hit_count, void *stream)
{
    WS_HANDLE(m);
    if (!s || !radiance_sum) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s: null pointer");
    if (!scene_args_ok(s)) return set_err(GPIS_ERR_INVALID_ARG, "gpis_ws_render_scene_s: scene arguments (size, rows, shard)");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    return ws_frame(h, s, sizeof(WsSceneRec), __func__, k_ws_scene<0>, h->scene_grid_cap, st,
                    [&](unsigned grid, size_t p0, uint32_t ns, void *recs) {
                        k_ws_scene<0><<<grid, 64, 0, st>>>(h->d_model.p, sc, p0, ns, h->d_scene_next.p, (WsSceneRec *)recs, h->d_work.p, h->d_counters.p);
                        return launch_check("k_ws_scene");
                    },
                    [&](size_t p0, size_t np, const void *recs) {
                        k_ws_scene_sum<0><<<(unsigned)((np + 255) / 256), 256, 0, st>>>(sc, p0, np, (const WsSceneRec *)recs, radiance_sum, hit_count);
                        return launch_check("k_ws_scene_sum");
                    });
}
