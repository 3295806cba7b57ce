// tu_adaptive_paths.hip — adaptive sampling for the RGB multi-bounce path driver (gpis_render_scene_s_paths_rgb_adaptive in
// gpis_hip.hip; gpis_adaptive.hpp, gpis_paths_rgb.hpp, gpis_launch.hpp): the camera step of a pass whose records carry different
// sample counts, and after the bounce loop of a chunk of records the clamped luminance of every sample, the tile statistics on it
// and the per-pixel RGB sum.  The bounce kernels, the regrouping and the marches are those of gpis_render_scene_s_paths_rgb.
#include <cstdint>

#include "gpis_adaptive.hpp"
#include "gpis_paths_rgb.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis {

// k_paths_rgb_begin for sample i of a chunk of records
__global__ void __launch_bounds__(256) k_rgb_adaptive_begin(SceneConst sc, AdaptiveChunk ch, size_t n_samples, PathsRgbArrays a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample_adaptive(sc, ch, i, x, y, spp);
    paths_rgb_begin_sample(sc, a, i, g, x, y, spp);
}

// one lane per sample: renderTile's clamp on the sample's em[3] and the luminance SampleRecord::addSample(const Vec3f &) takes of it
__global__ void __launch_bounds__(256) k_rgb_adaptive_value(size_t n_samples, size_t plane, const float *__restrict__ emission,
                                                            float *__restrict__ luminance, uint8_t *__restrict__ clamped)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    const float c0 = emission[i], c1 = emission[plane + i], c2 = emission[2 * plane + i];
    const bool z = adaptive_rgb_clamped(c0, c1, c2);
    luminance[i] = adaptive_luminance(z ? 0.f : c0, z ? 0.f : c1, z ? 0.f : c2);
    clamped[i] = z ? 1 : 0;
}

// one lane per record: SampleRecord::addSample over the record's luminances in the order the layout stores them (k_adaptive_stats)
__global__ void __launch_bounds__(256) k_rgb_adaptive_stats(AdaptiveChunk ch, const float *__restrict__ luminance, gpis_adaptive_record *__restrict__ records)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ch.nrec) return;
    const uint32_t r = ch.r0 + (uint32_t)j;
    const size_t first = (size_t)(ch.plan[r].offset - ch.plan[ch.r0].offset), n = (size_t)(ch.plan[r + 1].offset - ch.plan[r].offset);
    gpis_adaptive_record rec = records[r];
    for (size_t q = 0; q < n; ++q)
        adaptive_add_sample(rec, luminance[first + q]);
    records[r].sample_count = rec.sample_count;
    records[r].mean = rec.mean;
    records[r].running_variance = rec.running_variance;
}

// one lane per pixel slot (16 per record, those past a clipped tile idle): per channel the sequential sum over the pixel's clamped
// samples, in sample order, and the segments marched for them
__global__ void __launch_bounds__(256) k_rgb_adaptive_accumulate(SceneConst sc, AdaptiveChunk ch, size_t plane, const float *__restrict__ emission,
                                                                 const uint8_t *__restrict__ clamped, const uint32_t *__restrict__ segs,
                                                                 float *__restrict__ radiance_sum3, uint32_t *__restrict__ sample_count,
                                                                 uint32_t *__restrict__ seg_count)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)ch.nrec * (kVarianceTile * kVarianceTile)) return;
    const uint32_t r = ch.r0 + (uint32_t)(j / (kVarianceTile * kVarianceTile)), p = (uint32_t)(j % (kVarianceTile * kVarianceTile));
    const AdaptiveTile t = adaptive_tile(sc.s.width, sc.s.height, r);
    if (p >= t.w * t.h) return;
    const AdaptivePlanRec rec = ch.plan[r];
    const size_t first = (size_t)(rec.offset - ch.plan[ch.r0].offset) + (size_t)p * rec.count;
    float acc[3] = {0.f, 0.f, 0.f};
    uint32_t marched = 0;
    for (uint32_t k = 0; k < rec.count; ++k) {
        const bool z = clamped[first + k] != 0;
        for (int c = 0; c < 3; ++c)
            acc[c] += z ? 0.f : emission[c * plane + first + k];
        marched += segs[first + k];
    }
    const size_t pix = (size_t)(t.y0 + p / t.w) * sc.s.width + (t.x0 + p % t.w);
    for (int c = 0; c < 3; ++c)
        radiance_sum3[3 * pix + c] += acc[c];
    sample_count[pix] += rec.count;
    if (seg_count) seg_count[pix] += marched;
}

namespace launch {

void adaptive_paths_rgb_begin(const SceneConst &sc, const AdaptiveChunk &ch, size_t n_samples, const PathsRgbArrays &a, hipStream_t s)
{
    k_rgb_adaptive_begin<<<grid_of(n_samples, 256), 256, 0, s>>>(sc, ch, n_samples, a);
}
void adaptive_paths_rgb_value(size_t n_samples, const PathsRgbArrays &a, float *luminance, uint8_t *clamped, hipStream_t s)
{
    k_rgb_adaptive_value<<<grid_of(n_samples, 256), 256, 0, s>>>(n_samples, a.plane, a.emission, luminance, clamped);
}
void adaptive_paths_rgb_stats(const AdaptiveChunk &ch, const float *luminance, gpis_adaptive_record *records, hipStream_t s)
{
    k_rgb_adaptive_stats<<<grid_of(ch.nrec, 256), 256, 0, s>>>(ch, luminance, records);
}
void adaptive_paths_rgb_accumulate(const SceneConst &sc, const AdaptiveChunk &ch, const PathsRgbArrays &a, const uint8_t *clamped, float *radiance_sum3,
                                   uint32_t *sample_count, uint32_t *seg_count, hipStream_t s)
{
    k_rgb_adaptive_accumulate<<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, s>>>(sc, ch, a.plane, a.emission, clamped, a.segs,
                                                                                                               radiance_sum3, sample_count, seg_count);
}

}   // namespace launch
}   // namespace gpis

using namespace gpis;

extern "C" void gpis_adaptive_rgb_value_host(size_t n, const float *rgb_in, float *rgb_out, float *luminance)
{
    if (!rgb_in) return;
    for (size_t i = 0; i < n; ++i) {
        const float *c = rgb_in + 3 * i;
        const bool z = adaptive_rgb_clamped(c[0], c[1], c[2]);
        const float v[3] = {z ? 0.f : c[0], z ? 0.f : c[1], z ? 0.f : c[2]};
        if (luminance) luminance[i] = adaptive_luminance(v[0], v[1], v[2]);
        if (rgb_out) { rgb_out[3 * i] = v[0]; rgb_out[3 * i + 1] = v[1]; rgb_out[3 * i + 2] = v[2]; }
    }
}
