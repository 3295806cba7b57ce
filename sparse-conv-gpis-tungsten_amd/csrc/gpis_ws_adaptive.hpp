// gpis_ws_adaptive.hpp — behind the fused kernels of the weight-space adaptive drivers (k_ws_scene_adaptive, k_ws_paths_adaptive:
// gpis_ws_scene.hpp, gpis_ws_paths.hpp): the per-pixel sum over the variable-count layout and the tile statistics, stated once for
// both drivers on a value accessor.  Orders and the one `+=` per pass are k_adaptive_accumulate's and k_adaptive_stats's
// (gpis_adaptive.hpp); the sample records are indexed by the sample's position in the chunk.
#pragma once
#include "gpis_adaptive.hpp"
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

// one lane per pixel slot (16 per record, those past a clipped tile idle): sequential sum over the pixel's samples, in sample order
template <typename Values>
__global__ void __launch_bounds__(256) k_ws_adaptive_sum(SceneConst sc, AdaptiveChunk ch, Values a, float *__restrict__ radiance_sum,
                                                         uint32_t *__restrict__ sample_count, uint32_t *__restrict__ hit_count)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)ch.nrec * (kVarianceTile * kVarianceTile)) return;
    const uint32_t r = ch.r0 + (uint32_t)(j / (kVarianceTile * kVarianceTile)), p = (uint32_t)(j % (kVarianceTile * kVarianceTile));
    const AdaptiveTile t = adaptive_tile(sc.s.width, sc.s.height, r);
    if (p >= t.w * t.h) return;
    const AdaptivePlanRec rec = ch.plan[r];
    const size_t first = (size_t)(rec.offset - ch.plan[ch.r0].offset) + (size_t)p * rec.count;
    float acc = 0.f;
    uint32_t hits = 0;
    for (uint32_t k = 0; k < rec.count; ++k) {
        hits += a.hit(first + k);
        acc += a.value(first + k);
    }
    const size_t pix = (size_t)(t.y0 + p / t.w) * sc.s.width + (t.x0 + p % t.w);
    radiance_sum[pix] += acc;
    sample_count[pix] += rec.count;
    if (hit_count) hit_count[pix] += hits;
}

// one lane per record: SampleRecord::addSample over the tile's pixels row-major, then the sample index — the record's samples in
// the order the layout stores them
template <typename Values>
__global__ void __launch_bounds__(256) k_ws_adaptive_stats(AdaptiveChunk ch, Values a, gpis_adaptive_record *__restrict__ records)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ch.nrec) return;
    const uint32_t r = ch.r0 + (uint32_t)j;
    const size_t first = (size_t)(ch.plan[r].offset - ch.plan[ch.r0].offset), n = (size_t)(ch.plan[r + 1].offset - ch.plan[r].offset);
    gpis_adaptive_record rec = records[r];
    for (size_t q = 0; q < n; ++q)
        adaptive_add_sample(rec, a.value(first + q));
    records[r].sample_count = rec.sample_count;
    records[r].mean = rec.mean;
    records[r].running_variance = rec.running_variance;
}

}   // namespace gpis
