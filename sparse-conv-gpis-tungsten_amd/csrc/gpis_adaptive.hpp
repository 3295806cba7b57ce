// gpis_adaptive.hpp — the variable-count sample layout and the tile statistics of the adaptive frame drivers
// (gpis_render_scene_s_adaptive, gpis_render_scene_s_paths_rgb_adaptive, gpis_render_scene_s_paths_adaptive and
// gpis_render_scene_s_nee_paths_adaptive in tu_scene.hip; gpis_ws_render_scene_s_adaptive and gpis_ws_render_scene_s_paths_adaptive
// in tu_ws_adaptive.hip; gpis_fs_render_scene_s_adaptive and gpis_fs_render_scene_s_paths_adaptive in tu_fs_adaptive.hip;
// the host plan step in tu_adaptive.hip; include/gpis.h states the contract and cites the reference).
//   host + device: SampleRecord::addSample / errorEstimate (adaptive_add_sample, adaptive_error_estimate), the sample clamp of
//       renderTile on a float and on a Vec3f (adaptive_clamp, adaptive_rgb_clamped), Vec3f::luminance (adaptive_luminance), the 4x4
//       variance tile of a record clipped at the image edge (adaptive_tile);
//   device: scene_sample of an AdaptiveChunk — the camera step of gpis_scene.hpp's scene_sample for a pass whose records carry
//       different sample counts.  A driver whose camera kernel is a template on that argument renders under the adaptive schedule;
//       nothing else of its kernels changes.  The fused weight-space and function-space kernels take the same step inside their
//       work loop (k_ws_scene_adaptive, k_ws_paths_adaptive, k_fs_scene_adaptive, k_fs_paths_adaptive).
//       Behind a chunk, every driver's per-pixel sum and tile statistics are the bodies of gpis_frame_sum.hpp on the driver's
//       accessor (SceneRecValues below for the {cv, flags} records of the two fused Lambert frames); what stays here of the
//       three-channel RGB path driver is its clamp / luminance step and its three-channel sum.  The pass loop of all drivers is
//       gpis_adaptive_host.hpp's.
// Layout of a pass: records in index order; record r owns the samples [offset[r], offset[r+1]) = its pixels row-major x its
// next_sample_count samples, so a pixel's samples stay contiguous (what the cooperative guided evaluator lives on).
#pragma once
#include <cmath>
#include <cfloat>

#include "gpis.h"
#include "gpis_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

constexpr uint32_t kVarianceTile = 4;       // PathTraceIntegrator::VarianceTileSize

// what a pass's kernels read of a record: 16 bytes, uploaded once per pass (entry n_records holds the pass's sample total)
struct AdaptivePlanRec {
    uint64_t offset;                        // exclusive prefix sum of pixels * count over the records before
    uint32_t sample_index, count;           // SampleRecord::sampleIndex, nextSampleCount
};
// the records [r0, r0 + nrec) of a pass as one chunk: its samples are [plan[r0].offset, plan[r0 + nrec].offset)
struct AdaptiveChunk {
    const AdaptivePlanRec *plan;
    uint32_t r0, nrec;
};

struct AdaptiveTile { uint32_t x0, y0, w, h; };
__host__ __device__ inline AdaptiveTile adaptive_tile(uint32_t width, uint32_t height, uint32_t r)
{
    const uint32_t vw = (width + kVarianceTile - 1) / kVarianceTile;
    AdaptiveTile t;
    t.x0 = (r % vw) * kVarianceTile; t.y0 = (r / vw) * kVarianceTile;
    t.w = width - t.x0 < kVarianceTile ? width - t.x0 : kVarianceTile;
    t.h = height - t.y0 < kVarianceTile ? height - t.y0 : kVarianceTile;
    return t;
}

// SampleRecord::addSample(float), SampleRecord.hpp:44-50
__host__ __device__ inline void adaptive_add_sample(gpis_adaptive_record &r, float x)
{
    r.sample_count++;
    const float delta = x - r.mean;
    r.mean += delta / (float)r.sample_count;
    r.running_variance += delta * (x - r.mean);
}
// SampleRecord::variance / errorEstimate, :57-65 (max of MathUtil.hpp:26: a > b ? a : b)
__host__ __device__ inline float adaptive_variance(const gpis_adaptive_record &r) { return r.running_variance / (float)(r.sample_count - 1u); }
__host__ __device__ inline float adaptive_error_estimate(const gpis_adaptive_record &r)
{
    const float m2 = r.mean * r.mean;
    return adaptive_variance(r) / ((float)r.sample_count * (m2 > 1e-3f ? m2 : 1e-3f));
}
// renderTile's clamp, PathTraceIntegrator.cpp:149-156: NaN, +-inf and values above 65536 count as 0
__host__ __device__ inline float adaptive_clamp(float c) { return (!(fabsf(c) <= FLT_MAX) || c > 65536.f) ? 0.f : c; }
// the same clamp on a Vec3f sample: one NaN, infinite or > 65536 component makes all three count as 0
__host__ __device__ inline bool adaptive_rgb_clamped(float c0, float c1, float c2)
{
    return !(fabsf(c0) <= FLT_MAX) || !(fabsf(c1) <= FLT_MAX) || !(fabsf(c2) <= FLT_MAX) || c0 > 65536.f || c1 > 65536.f || c2 > 65536.f;
}
// Vec3f::luminance, Vec.hpp:218-222: what SampleRecord::addSample(const Vec3f &) hands addSample(float), SampleRecord.hpp:52-55
__host__ __device__ inline float adaptive_luminance(float c0, float c1, float c2) { return ((c0 * 0.2126f) + (c1 * 0.7152f)) + (c2 * 0.0722f); }

// What a sample of a fused Lambert frame is worth, on its record {cv, flags} (WsSceneRec, FsSceneRec: bit 0 = the primary segment
// hit, bit 1 = lit, cv takes part in the pixel's sum) — an accessor of gpis_frame_sum.hpp.  raw is what the uniform entry adds,
// unclamped; value is raw after renderTile's clamp, what the adaptive entry adds and accounts.
template <typename Rec>
struct SceneRecValues {
    const Rec *recs;
    float light_radiance;
    GPIS_DEV float raw(size_t i) const
    {
        const Rec r = recs[i];
        return (r.flags & 2u) ? r.cv * light_radiance : 0.f;
    }
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(raw(i)); }
    GPIS_DEV uint32_t count(size_t i) const { return recs[i].flags & 1u; }
};

// Sample i of a chunk -> its record, then its pixel, its sample index k and the sample's PCG32 stream, seeded as scene_sample seeds
// the sample (x, y, k).  The record is the last one of the chunk whose offset is <= the sample's position in the pass.
GPIS_DEV Pcg32 scene_sample(const SceneConst &sc, const AdaptiveChunk &c, size_t i, uint32_t &x, uint32_t &y, uint32_t &spp)
{
    const gpis_scene_s &s = sc.s;
    const uint64_t pos = c.plan[c.r0].offset + i;
    uint32_t lo = c.r0, hi = c.r0 + c.nrec;           // plan[lo].offset <= pos < plan[hi].offset
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (c.plan[mid].offset <= pos) lo = mid; else hi = mid;
    }
    const AdaptivePlanRec rec = c.plan[lo];
    const uint32_t local = (uint32_t)(pos - rec.offset);      // a record holds fewer than 2^32 samples (the entry checks)
    const uint32_t p = local / rec.count;
    const AdaptiveTile t = adaptive_tile(s.width, s.height, lo);
    x = t.x0 + p % t.w; y = t.y0 + p / t.w;
    spp = s.spp_begin + rec.sample_index + local % rec.count;
    Pcg32 g;
    g.set_state((uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s.scene_seed) + 1u));
    return g;
}

// ---- the RGB path driver (gpis_render_scene_s_paths_rgb_adaptive), after the bounce loop of a chunk of records; `emission`: three
// planes of `plane` floats (gpis_paths_rgb.hpp)

// one lane per sample: renderTile's clamp on the sample's em[3] and the luminance SampleRecord::addSample(const Vec3f &) takes of it
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_rgb_adaptive_value(size_t n_samples, size_t plane, const float *__restrict__ emission,
                                                                           float *__restrict__ luminance, uint8_t *__restrict__ clamped)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    const float c0 = emission[i], c1 = emission[plane + i], c2 = emission[2 * plane + i];
    const bool z = adaptive_rgb_clamped(c0, c1, c2);
    luminance[i] = adaptive_luminance(z ? 0.f : c0, z ? 0.f : c1, z ? 0.f : c2);
    clamped[i] = z ? 1 : 0;
}

// one lane per pixel slot (16 per record, those past a clipped tile idle): per channel the sequential sum over the pixel's clamped
// samples, in sample order, and the segments marched for them
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_rgb_adaptive_accumulate(SceneConst sc, AdaptiveChunk ch, size_t plane, const float *__restrict__ emission,
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

}   // namespace gpis
