// gpis_frame_sum.hpp — what sits behind a chunk of every scene-S frame driver, stated once: the per-pixel sum of the uniform sample
// layout (frame_values_sum), the per-pixel sum of the variable-count layout of an adaptive pass (adaptive_values_sum) and the tile
// statistics (adaptive_values_stats).  The kernels of the drivers are one-line wrappers around these bodies (k_paths_accumulate,
// k_adaptive_accumulate, k_adaptive_stats, k_paths_adaptive_sum, k_paths_adaptive_tile_stats, k_rgb_adaptive_stats: tu_scene.hip;
// k_ws_scene_sum, k_ws_paths_sum, k_fs_scene_sum, k_fs_paths_sum: next to their fused kernels; k_ws_adaptive_* / k_fs_adaptive_*:
// gpis_ws_adaptive.hpp, gpis_fs_adaptive.hpp).  All of them sum a pixel's samples sequentially from 0.f in sample order and make one
// `+=` per call, which is what the bit-for-bit tests of the drivers against each other rest on.
// A driver states what a sample is worth once, as an accessor next to its sample record; the sample is indexed by its position in
// the chunk.  An accessor offers what the bodies it is used with call:
//   raw(i)    the value the uniform entry adds, unclamped (0.f for a sample that takes no part in the sum);
//   value(i)  the same value after renderTile's clamp (adaptive_clamp), which the adaptive entries add and account;
//   count(i)  what the sample adds to the per-pixel count beside the image: the primary segment's hit, the segments marched, or 0u.
// The bodies take the kernels' arguments by value and without a second __restrict__ (the kernels' parameters carry it).
#pragma once
#include "gpis_adaptive.hpp"

#pragma clang fp contract(off)

namespace gpis {

// The uniform layout, one lane per pixel: sequential sum over the pixel's spp_count samples, in sample order.  The uniform entries
// do not clamp: the body adds raw(i), not value(i).  A masked sample adds raw(i) = 0.f where the drivers' own sums once skipped it;
// that is the same float, since acc starts at +0.f and a sum of floats that starts there never becomes -0.f.  The count is written
// only where the caller asked for it.
template <typename Values>
GPIS_DEV void frame_values_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, Values a, float *radiance_sum, uint32_t *count_out)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pixels) return;
    const uint32_t spp = sc.s.spp_count;
    float acc = 0.f;
    uint32_t count = 0;
    for (uint32_t k = 0; k < spp; ++k) {
        count += a.count(j * spp + k);
        acc += a.raw(j * spp + k);
    }
    const size_t pix = scene_pixel(sc.s, first_pixel + j);
    radiance_sum[pix] += acc;
    if (count_out) count_out[pix] += count;
}

// The variable-count layout, one lane per pixel slot (16 per record, those past a clipped tile idle): sequential sum over the pixel's
// samples, in sample order.  value(i) is clamped already; the body never clamps itself (a luminance clamped a second time can differ
// at 65536).
template <typename Values>
GPIS_DEV void adaptive_values_sum(SceneConst sc, AdaptiveChunk ch, Values a, float *radiance_sum, uint32_t *sample_count, uint32_t *count_out)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)ch.nrec * (kVarianceTile * kVarianceTile)) return;
    const uint32_t r = ch.r0 + (uint32_t)(j / (kVarianceTile * kVarianceTile)), p = (uint32_t)(j % (kVarianceTile * kVarianceTile));
    const AdaptiveTile t = adaptive_tile(sc.s.width, sc.s.height, r);
    if (p >= t.w * t.h) return;
    const AdaptivePlanRec rec = ch.plan[r];
    const size_t first = (size_t)(rec.offset - ch.plan[ch.r0].offset) + (size_t)p * rec.count;
    float acc = 0.f;
    uint32_t count = 0;
    for (uint32_t k = 0; k < rec.count; ++k) {
        count += a.count(first + k);
        acc += a.value(first + k);
    }
    const size_t pix = (size_t)(t.y0 + p / t.w) * sc.s.width + (t.x0 + p % t.w);
    radiance_sum[pix] += acc;
    sample_count[pix] += rec.count;
    if (count_out) count_out[pix] += count;
}

// one lane per record: SampleRecord::addSample over the tile's pixels row-major, then the sample index — the record's samples in
// the order the layout stores them.  value(i) is clamped already, as above.
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
