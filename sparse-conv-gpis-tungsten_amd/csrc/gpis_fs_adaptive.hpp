// gpis_fs_adaptive.hpp — behind the fused kernels of the function-space adaptive drivers (k_fs_scene_adaptive, k_fs_paths_adaptive:
// gpis_fs_scene.hpp, gpis_fs_paths.hpp): what the per-pixel sum over the variable-count layout and the tile statistics read of their
// sample records, and the two kernels, which are the bodies the weight-space drivers run (gpis_adaptive_sum.hpp) on these accessors.
// tu_fs_adaptive.hip instantiates them.
#pragma once
#include "gpis_adaptive.hpp"
#include "gpis_adaptive_sum.hpp"
#include "gpis_fs_paths.hpp"
#include "gpis_fs_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

// the value of sample i of a chunk after renderTile's clamp, and what the sample adds to the per-pixel count beside the image
struct FsSceneValues {                    // the Lambert frame: what k_fs_scene_sum adds, clamped; the count is the primary segment's hit
    const FsSceneRec *recs;
    float light_radiance;
    GPIS_DEV float value(size_t i) const
    {
        const FsSceneRec r = recs[i];
        return (r.flags & 2u) ? adaptive_clamp(r.cv * light_radiance) : 0.f;
    }
    GPIS_DEV uint32_t hit(size_t i) const { return recs[i].flags & 1u; }
};
struct FsPathsValues {                    // the path driver, a mono estimator: the scalar emission, clamped; the count is the sample's
    const FsPathsRec *recs;               // segments, path plus shadow, whether or not the clamp took its value
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(recs[i].emission); }
    GPIS_DEV uint32_t hit(size_t i) const { return recs[i].segs; }
};

template <typename Values>
__global__ void __launch_bounds__(256) k_fs_adaptive_sum(SceneConst sc, AdaptiveChunk ch, Values a, float *__restrict__ radiance_sum,
                                                         uint32_t *__restrict__ sample_count, uint32_t *__restrict__ count)
{
    adaptive_values_sum(sc, ch, a, radiance_sum, sample_count, count);
}
template <typename Values>
__global__ void __launch_bounds__(256) k_fs_adaptive_stats(AdaptiveChunk ch, Values a, gpis_adaptive_record *__restrict__ records)
{
    adaptive_values_stats(ch, a, records);
}

}   // namespace gpis
