// gpis_ws_adaptive.hpp — behind the fused kernels of the weight-space adaptive drivers (k_ws_scene_adaptive, k_ws_paths_adaptive:
// gpis_ws_scene.hpp, gpis_ws_paths.hpp): the per-pixel sum over the variable-count layout and the tile statistics
// (gpis_adaptive_sum.hpp, shared with the function-space drivers) on the value accessors of the two weight-space drivers.
#pragma once
#include "gpis_adaptive.hpp"
#include "gpis_adaptive_sum.hpp"
#include "gpis_ws_paths.hpp"
#include "gpis_ws_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

// the value of sample i of a chunk after renderTile's clamp, and whether its primary segment hit
struct WsSceneValues {                    // the Lambert frame: what k_ws_scene_sum adds, clamped
    const WsSceneRec *recs;
    float light_radiance;
    GPIS_DEV float value(size_t i) const
    {
        const WsSceneRec r = recs[i];
        return (r.flags & 2u) ? adaptive_clamp(r.cv * light_radiance) : 0.f;
    }
    GPIS_DEV uint32_t hit(size_t i) const { return recs[i].flags & 1u; }
};
struct WsPathsValues {                    // the path driver, a mono estimator: the scalar emission, clamped; it counts no hits
    const WsPathsRec *recs;
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(recs[i].emission); }
    GPIS_DEV uint32_t hit(size_t) const { return 0u; }
};

// the sum and the statistics of gpis_adaptive_sum.hpp on a weight-space accessor
template <typename Values>
__global__ void __launch_bounds__(256) k_ws_adaptive_sum(SceneConst sc, AdaptiveChunk ch, Values a, float *__restrict__ radiance_sum,
                                                         uint32_t *__restrict__ sample_count, uint32_t *__restrict__ hit_count)
{
    adaptive_values_sum(sc, ch, a, radiance_sum, sample_count, hit_count);
}
template <typename Values>
__global__ void __launch_bounds__(256) k_ws_adaptive_stats(AdaptiveChunk ch, Values a, gpis_adaptive_record *__restrict__ records)
{
    adaptive_values_stats(ch, a, records);
}

}   // namespace gpis
