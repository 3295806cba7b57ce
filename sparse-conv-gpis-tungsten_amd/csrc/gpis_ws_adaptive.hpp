// gpis_ws_adaptive.hpp — behind the fused kernels of the weight-space adaptive drivers (k_ws_scene_adaptive, k_ws_paths_adaptive:
// gpis_ws_scene.hpp, gpis_ws_paths.hpp): the per-pixel sum over the variable-count layout and the tile statistics of
// gpis_frame_sum.hpp on the accessors of the two drivers' sample records (WsSceneValues, WsPathsValues, next to the records).
#pragma once
#include "gpis_frame_sum.hpp"
#include "gpis_ws_paths.hpp"
#include "gpis_ws_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

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
