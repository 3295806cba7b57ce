// tu_adaptive.hip — adaptive sampling for the scene-S Lambert frame (gpis_render_scene_s_adaptive in gpis_hip.hip; gpis_adaptive.hpp,
// gpis_launch.hpp): the camera step, the per-pixel sum and the tile statistics of a pass whose records carry different sample
// counts, and the host plan step (PathTraceIntegrator::generateWork) between the passes.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gpis_adaptive.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis {

int host_set_err(int code, const char *msg);      // gpis_hip.hip: the library's thread-local error text

// ---- kernels.  The two camera steps write what k_scene_primary / k_scene_primary_c write for the sample (x, y, k).
__global__ void __launch_bounds__(256) k_adaptive_primary(SceneConst sc, AdaptiveChunk ch, size_t n_samples, gpis_ray_in *__restrict__ rays,
                                                          float *__restrict__ u_shadow, uint8_t *__restrict__ valid)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample_adaptive(sc, ch, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i()), u1 = normalized_uint(g.next_i());
    gpis_ray_in r;
    bool hit = scene_camera_ray(sc, x, y, spp, jx, jy, r);
    r.u_jitter = u0;
    rays[i] = r;
    u_shadow[i] = u1;
    valid[i] = hit ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_adaptive_primary_c(SceneConst sc, AdaptiveChunk ch, size_t n_samples, SceneRay *__restrict__ rays)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample_adaptive(sc, ch, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i()), u1 = normalized_uint(g.next_i());
    const V3 d = scene_camera_dir(sc, x, y, jx, jy);
    float t0 = 0.f, t1 = 0.f;
    const bool hit = sphere_chord(v3(sc.s.cam_pos[0], sc.s.cam_pos[1], sc.s.cam_pos[2]), d, sc.s.bound_radius, t0, t1);
    float4 *q = reinterpret_cast<float4 *>(rays + i);
    q[0] = make_float4(d.x, d.y, d.z, t0);
    q[1] = make_float4(t1, u0, u1, __uint_as_float(hit ? kSceneRayLive : 0u));
}

// the value of sample i as k_scene_accumulate adds it, after renderTile's clamp
GPIS_DEV float adaptive_sample_value(const launch::AdaptiveLambert &a, size_t i, float light_radiance)
{
    return a.valid2[i] ? adaptive_clamp(a.cosl[i] * (a.vis[i] ? 1.f : 0.f) * light_radiance) : 0.f;
}

// one lane per pixel slot (16 per record, those past a clipped tile idle): sequential sum over the pixel's samples, in sample order
__global__ void __launch_bounds__(256) k_adaptive_accumulate(SceneConst sc, AdaptiveChunk ch, launch::AdaptiveLambert a, float *__restrict__ radiance_sum,
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
        hits += a.hit[first + k];
        acc += adaptive_sample_value(a, first + k, sc.s.light_radiance);
    }
    const size_t pix = (size_t)(t.y0 + p / t.w) * sc.s.width + (t.x0 + p % t.w);
    radiance_sum[pix] += acc;
    sample_count[pix] += rec.count;
    if (hit_count) hit_count[pix] += hits;
}

// one lane per record: SampleRecord::addSample over the tile's pixels row-major, then the sample index — the record's samples in
// the order the layout stores them
__global__ void __launch_bounds__(256) k_adaptive_stats(SceneConst sc, AdaptiveChunk ch, launch::AdaptiveLambert a, gpis_adaptive_record *__restrict__ records)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ch.nrec) return;
    const uint32_t r = ch.r0 + (uint32_t)j;
    const size_t first = (size_t)(ch.plan[r].offset - ch.plan[ch.r0].offset), n = (size_t)(ch.plan[r + 1].offset - ch.plan[r].offset);
    gpis_adaptive_record rec = records[r];
    for (size_t q = 0; q < n; ++q)
        adaptive_add_sample(rec, adaptive_sample_value(a, first + q, sc.s.light_radiance));
    records[r].sample_count = rec.sample_count;
    records[r].mean = rec.mean;
    records[r].running_variance = rec.running_variance;
}

namespace launch {

void adaptive_primary(const SceneConst &sc, const AdaptiveChunk &ch, size_t n_samples, gpis_ray_in *rays, float *u_shadow, uint8_t *valid, hipStream_t s)
{
    k_adaptive_primary<<<grid_of(n_samples, 256), 256, 0, s>>>(sc, ch, n_samples, rays, u_shadow, valid);
}
void adaptive_primary_compact(const SceneConst &sc, const AdaptiveChunk &ch, size_t n_samples, SceneRay *rays, hipStream_t s)
{
    k_adaptive_primary_c<<<grid_of(n_samples, 256), 256, 0, s>>>(sc, ch, n_samples, rays);
}
void adaptive_accumulate(const SceneConst &sc, const AdaptiveChunk &ch, const AdaptiveLambert &a, float *radiance_sum, uint32_t *sample_count,
                         uint32_t *hit_count, hipStream_t s)
{
    k_adaptive_accumulate<<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, s>>>(sc, ch, a, radiance_sum, sample_count, hit_count);
}
void adaptive_stats(const SceneConst &sc, const AdaptiveChunk &ch, const AdaptiveLambert &a, gpis_adaptive_record *records, hipStream_t s)
{
    k_adaptive_stats<<<grid_of(ch.nrec, 256), 256, 0, s>>>(sc, ch, a, records);
}

}   // namespace launch

// ---- the host plan step.  The integrator's sampler: UniformSampler.hpp:41-53 with sequence 0.
namespace {

struct HostPcg {
    uint64_t state;
    uint32_t next_i()
    {
        const uint64_t old = state;
        state = old * 6364136223846793005ULL + 1ULL;
        const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((0u - rot) & 31u));
    }
    float next_1d()
    {
        const uint32_t bits = (next_i() >> 9u) | 0x3F800000u;
        float f;
        memcpy(&f, &bits, sizeof f);
        return f - 1.0f;
    }
};
uint32_t hash32(uint32_t x)     // MathUtil.hpp:169
{
    x = ~x + (x << 15);
    x = x ^ (x >> 12);
    x = x + (x << 2);
    x = x ^ (x >> 4);
    x = x * 2057;
    x = x ^ (x >> 16);
    return x;
}
// int(float) of distributeAdaptiveSamples, defined for every input: NaN -> 0, saturating
int to_int(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.f) return INT32_MAX;
    if (f <= -2147483648.f) return INT32_MIN;
    return (int)f;
}

float error_percentile_95(size_t n, gpis_adaptive_record *rec)     // :43-58
{
    std::vector<float> errors;
    errors.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        rec[i].adaptive_weight = adaptive_error_estimate(rec[i]);
        if (rec[i].adaptive_weight > 0.0f)
            errors.push_back(rec[i].adaptive_weight);
    }
    if (errors.empty())
        return 0.0f;
    std::sort(errors.begin(), errors.end());
    return errors[(errors.size() * 95) / 100];
}
void dilate_adaptive_weights(uint32_t vw, uint32_t vh, gpis_adaptive_record *rec)     // :60-84
{
    auto up = [&](size_t idx, size_t other) {     // a = max(a, b) of MathUtil.hpp:26: a > b ? a : b
        rec[idx].adaptive_weight = rec[idx].adaptive_weight > rec[other].adaptive_weight ? rec[idx].adaptive_weight : rec[other].adaptive_weight;
    };
    for (uint32_t y = 0; y < vh; ++y)
        for (uint32_t x = 0; x < vw; ++x) {
            const size_t idx = x + (size_t)y * vw;
            if (y < vh - 1) up(idx, idx + vw);
            if (x < vw - 1) up(idx, idx + 1);
        }
    for (uint32_t y = vh; y-- > 0;)
        for (uint32_t x = vw; x-- > 0;) {
            const size_t idx = x + (size_t)y * vw;
            if (y > 0) up(idx, idx - vw);
            if (x > 0) up(idx, idx - 1);
        }
}
void distribute_adaptive_samples(uint32_t spp, uint32_t width, uint32_t height, HostPcg &rng, size_t n, gpis_adaptive_record *rec)     // :86-107
{
    double total_weight = 0.0;
    for (size_t i = 0; i < n; ++i)
        total_weight += rec[i].adaptive_weight;
    const int adaptive_budget = (int)((spp - 1u) * width * height);                                    // int * uint32 * uint32: modulo 2^32
    const int budget_per_tile = (int)((uint32_t)adaptive_budget / (kVarianceTile * kVarianceTile));   // int / uint32: unsigned
    const float weight_to_sample_factor = (float)((double)budget_per_tile / total_weight);
    float pixel_pdf = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float fractional_samples = rec[i].adaptive_weight * weight_to_sample_factor;
        uint32_t adaptive_samples = (uint32_t)to_int(fractional_samples);
        pixel_pdf += fractional_samples - (float)(int)adaptive_samples;
        if (rng.next_1d() < pixel_pdf) {
            adaptive_samples++;
            pixel_pdf -= 1.0f;
        }
        rec[i].next_sample_count = adaptive_samples + 1u;
    }
}

}   // namespace
}   // namespace gpis

using namespace gpis;

extern "C" void gpis_default_adaptive_s(gpis_adaptive_s *a)
{
    if (!a) return;
    a->spp_step = 16;
    a->threshold = 16;
    a->seed = 0xBA5EBA11u;
    a->_pad = 0;
}

extern "C" uint64_t gpis_adaptive_rng_init_host(const gpis_adaptive_s *a, uint32_t width, uint32_t height)
{
    if (!a) return 0;
    HostPcg g;
    g.state = hash32(a->seed);                       // UniformSampler(seed): _state = seed, then next2D()
    g.next_i(); g.next_i();
    const uint64_t tiles = (uint64_t)((width + 15u) / 16u) * ((height + 15u) / 16u);     // diceTiles: one nextI() per 16x16 tile
    for (uint64_t t = 0; t < tiles; ++t)
        g.next_i();
    return g.state;
}

extern "C" int gpis_adaptive_plan_host(const gpis_adaptive_s *a, uint32_t width, uint32_t height, uint32_t current_spp, uint32_t pass_spp,
                                       uint64_t *rng_state, size_t n_records, gpis_adaptive_record *records)
{
    const uint32_t vw = (width + kVarianceTile - 1) / kVarianceTile, vh = (height + kVarianceTile - 1) / kVarianceTile;
    if (!a || !rng_state || !records || width == 0 || height == 0 || pass_spp == 0 || a->threshold < 2 || n_records != (size_t)vw * vh)
        return host_set_err(GPIS_ERR_INVALID_ARG, "gpis_adaptive_plan_host: invalid argument");
    for (size_t i = 0; i < n_records; ++i)                                                              // generateWork, :109-133
        records[i].sample_index += records[i].next_sample_count;
    if (current_spp >= a->threshold) {
        const float max_error = error_percentile_95(n_records, records);
        if (max_error == 0.0f)
            return 0;
        for (size_t i = 0; i < n_records; ++i)
            records[i].adaptive_weight = records[i].adaptive_weight < max_error ? records[i].adaptive_weight : max_error;   // min(a, b): a < b ? a : b
        dilate_adaptive_weights(vw, vh, records);
        HostPcg rng{*rng_state};
        distribute_adaptive_samples(pass_spp, width, height, rng, n_records, records);
        *rng_state = rng.state;
    } else {
        for (size_t i = 0; i < n_records; ++i)
            records[i].next_sample_count = pass_spp;
    }
    return 1;
}

extern "C" void gpis_adaptive_record_add_host(gpis_adaptive_record *rec, size_t n, const float *values, float *out2)
{
    if (!rec) return;
    for (size_t i = 0; i < n; ++i)
        adaptive_add_sample(*rec, values[i]);
    if (out2) { out2[0] = adaptive_variance(*rec); out2[1] = adaptive_error_estimate(*rec); }
}
