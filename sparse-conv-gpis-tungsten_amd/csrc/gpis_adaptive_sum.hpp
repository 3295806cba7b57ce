// gpis_adaptive_sum.hpp — the per-pixel sum over the variable-count layout of an adaptive pass and the tile statistics, stated once
// for the fused drivers of both GP media on a value accessor (weight-space: gpis_ws_adaptive.hpp, k_ws_adaptive_sum /
// k_ws_adaptive_stats; function-space: gpis_fs_adaptive.hpp, k_fs_adaptive_sum / k_fs_adaptive_stats).  Orders and the one `+=` per
// pass are k_adaptive_accumulate's and k_adaptive_stats's (gpis_adaptive.hpp); the sample records are indexed by the sample's position
// in the chunk.  An accessor gives value(i), the value of sample i of a chunk after renderTile's clamp, and hit(i), what the sample
// adds to the per-pixel count beside the image (the primary segment's hit, or the segments marched).  The bodies take the kernels'
// arguments by value and without a second __restrict__ (the kernels' parameters carry it).
#pragma once
#include "gpis_adaptive.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one lane per pixel slot (16 per record, those past a clipped tile idle): sequential sum over the pixel's samples, in sample order
template <typename Values>
GPIS_DEV void adaptive_values_sum(SceneConst sc, AdaptiveChunk ch, Values a, float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count)
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
GPIS_DEV void adaptive_values_stats(AdaptiveChunk ch, Values a, gpis_adaptive_record *records)
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
