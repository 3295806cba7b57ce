// tu_adaptive.hip — the host side of the adaptive sample schedule (gpis_adaptive.hpp; the frame drivers that run under it are in
// tu_scene.hip): the plan step between the passes (PathTraceIntegrator::generateWork) and the host restatements of the record
// update and of the RGB sample value that the tests read.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gpis_adaptive.hpp"

#pragma clang fp contract(off)

namespace gpis {

int set_err(int code, const char *fmt, ...);      // gpis_hip.hip: the library's thread-local error text (gpis_host_base.hpp)

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
        return set_err(GPIS_ERR_INVALID_ARG, "gpis_adaptive_plan_host: invalid argument");
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
