/* TEST INFRASTRUCTURE: plain-C restatement of the adaptive sample schedule of gpis_render_scene_s_adaptive (include/gpis.h):
 * SampleRecord::addSample / variance / errorEstimate (SampleRecord.hpp:44-65), the plan step PathTraceIntegrator::generateWork
 * with errorPercentile95, dilateAdaptiveWeights and distributeAdaptiveSamples (PathTraceIntegrator.cpp:43-133), the integrator's
 * sampler (UniformSampler.hpp:22-53, MathUtil.hpp:169) and the whole pass loop with renderTile's clamp and visiting order
 * (:135-163) over sample values the caller supplies.  Written from the reference's text, independently of csrc/tu_adaptive.hip;
 * compiled with the flags of oracle/Makefile (no contraction). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "gpis.h"

static uint32_t pcg_next(uint64_t *state)
{
    uint64_t old = *state;
    *state = old * 6364136223846793005ULL + 1ULL;
    uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
}
static float pcg_next1d(uint64_t *state)
{
    union { uint32_t u; float f; } v;
    v.u = (pcg_next(state) >> 9u) | 0x3F800000u;
    return v.f - 1.0f;
}
static uint32_t hash32(uint32_t x)
{
    x = ~x + (x << 15);
    x = x ^ (x >> 12);
    x = x + (x << 2);
    x = x ^ (x >> 4);
    x = x * 2057u;
    x = x ^ (x >> 16);
    return x;
}

uint64_t adaptive_ref_rng_init(const gpis_adaptive_s *a, uint32_t width, uint32_t height)
{
    uint64_t state = hash32(a->seed);
    pcg_next(&state);
    pcg_next(&state);
    for (uint32_t y = 0; y < height; y += 16)
        for (uint32_t x = 0; x < width; x += 16)
            pcg_next(&state);
    return state;
}

static void add_sample(gpis_adaptive_record *r, float x)
{
    r->sample_count++;
    float delta = x - r->mean;
    r->mean += delta / r->sample_count;
    r->running_variance += delta * (x - r->mean);
}
static float variance(const gpis_adaptive_record *r) { return r->running_variance / (r->sample_count - 1); }
static float fmax_ref(float a, float b) { return a > b ? a : b; }
static float fmin_ref(float a, float b) { return a < b ? a : b; }
static float error_estimate(const gpis_adaptive_record *r) { return variance(r) / (r->sample_count * fmax_ref(r->mean * r->mean, 1e-3f)); }

void adaptive_ref_add(gpis_adaptive_record *rec, size_t n, const float *values, float *out2)
{
    for (size_t i = 0; i < n; ++i)
        add_sample(rec, values[i]);
    if (out2) { out2[0] = variance(rec); out2[1] = error_estimate(rec); }
}

static int cmp_float(const void *a, const void *b)
{
    float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}
static int float_to_int(float f)
{
    if (isnan(f)) return 0;
    if (f >= 2147483648.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int)f;
}

int adaptive_ref_plan(const gpis_adaptive_s *a, uint32_t width, uint32_t height, uint32_t current_spp, uint32_t pass_spp, uint64_t *rng_state,
                      size_t n_records, gpis_adaptive_record *s)
{
    int vw = (int)((width + 3) / 4), vh = (int)((height + 3) / 4);
    if (n_records != (size_t)vw * (size_t)vh || pass_spp == 0)
        return -1;
    for (size_t i = 0; i < n_records; ++i)
        s[i].sample_index += s[i].next_sample_count;
    if (current_spp < a->threshold) {
        for (size_t i = 0; i < n_records; ++i)
            s[i].next_sample_count = pass_spp;
        return 1;
    }
    /* errorPercentile95 */
    float *errors = (float *)malloc(n_records * sizeof(float));
    size_t n_err = 0;
    for (size_t i = 0; i < n_records; ++i) {
        s[i].adaptive_weight = error_estimate(&s[i]);
        if (s[i].adaptive_weight > 0.0f)
            errors[n_err++] = s[i].adaptive_weight;
    }
    float max_error = 0.0f;
    if (n_err) {
        qsort(errors, n_err, sizeof(float), cmp_float);
        max_error = errors[(n_err * 95) / 100];
    }
    free(errors);
    if (max_error == 0.0f)
        return 0;
    for (size_t i = 0; i < n_records; ++i)
        s[i].adaptive_weight = fmin_ref(s[i].adaptive_weight, max_error);
    /* dilateAdaptiveWeights */
    for (int y = 0; y < vh; ++y)
        for (int x = 0; x < vw; ++x) {
            int idx = x + y * vw;
            if (y < vh - 1) s[idx].adaptive_weight = fmax_ref(s[idx].adaptive_weight, s[idx + vw].adaptive_weight);
            if (x < vw - 1) s[idx].adaptive_weight = fmax_ref(s[idx].adaptive_weight, s[idx + 1].adaptive_weight);
        }
    for (int y = vh - 1; y >= 0; --y)
        for (int x = vw - 1; x >= 0; --x) {
            int idx = x + y * vw;
            if (y > 0) s[idx].adaptive_weight = fmax_ref(s[idx].adaptive_weight, s[idx - vw].adaptive_weight);
            if (x > 0) s[idx].adaptive_weight = fmax_ref(s[idx].adaptive_weight, s[idx - 1].adaptive_weight);
        }
    /* distributeAdaptiveSamples */
    double total_weight = 0.0;
    for (size_t i = 0; i < n_records; ++i)
        total_weight += s[i].adaptive_weight;
    int spp = (int)pass_spp;
    int adaptive_budget = (int)((uint32_t)(spp - 1) * width * height);
    int budget_per_tile = (int)((uint32_t)adaptive_budget / 16u);
    float weight_to_sample_factor = (float)((double)budget_per_tile / total_weight);
    float pixel_pdf = 0.0f;
    for (size_t i = 0; i < n_records; ++i) {
        float fractional_samples = s[i].adaptive_weight * weight_to_sample_factor;
        int adaptive_samples = float_to_int(fractional_samples);
        pixel_pdf += fractional_samples - (float)adaptive_samples;
        uint32_t count = (uint32_t)adaptive_samples;
        if (pcg_next1d(rng_state) < pixel_pdf) {
            count++;
            pixel_pdf -= 1.0f;
        }
        s[i].next_sample_count = count + 1u;
    }
    return 1;
}

static float clamp_sample(float c)
{
    if (isinf(c) || c > 65536.0f) return 0.0f;
    if (isnan(c)) return 0.0f;
    return c;
}

/* The whole frame over values[(y*width + x) * k_have + k] (the unclamped contribution of sample k = spp_begin + k of that pixel) and
 * hits[...] likewise.  Returns 0 when done; 1 when a pass needs a sample index >= k_have (*k_needed says how many: nothing of that
 * pass has been added; call again from the start with more).  counts (may be NULL): next_sample_count of every record for each of
 * the first max_passes passes, pass-major. */
int adaptive_ref_frame(const gpis_adaptive_s *a, uint32_t width, uint32_t height, uint32_t spp_total, uint32_t k_have, const float *values,
                       const uint8_t *hits, float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count, gpis_adaptive_record *records,
                       gpis_adaptive_info *info, uint32_t *counts, uint32_t max_passes, uint32_t *k_needed)
{
    uint32_t vw = (width + 3) / 4, vh = (height + 3) / 4;
    size_t n_records = (size_t)vw * vh;
    uint64_t rng = adaptive_ref_rng_init(a, width, height);
    memset(records, 0, n_records * sizeof *records);
    memset(info, 0, sizeof *info);
    *k_needed = 0;
    uint32_t cur = 0;
    while (cur < spp_total) {
        uint32_t next = cur + a->spp_step < spp_total ? cur + a->spp_step : spp_total;
        int go = adaptive_ref_plan(a, width, height, cur, next - cur, &rng, n_records, records);
        if (go < 0) return go;
        if (go == 0) { info->stopped_early = 1; return 0; }
        for (size_t r = 0; r < n_records; ++r) {
            uint32_t need = records[r].sample_index + records[r].next_sample_count;
            if (need > *k_needed) *k_needed = need;
            if (counts && info->passes_rendered < max_passes) counts[info->passes_rendered * n_records + r] = records[r].next_sample_count;
        }
        if (*k_needed > k_have) return 1;
        /* renderTile: tiles of 16 pixels, pixels row-major inside a tile; per record that is its own pixels row-major */
        for (uint32_t ty = 0; ty < height; ty += 16)
            for (uint32_t tx = 0; tx < width; tx += 16)
                for (uint32_t y = ty; y < ty + 16 && y < height; ++y)
                    for (uint32_t x = tx; x < tx + 16 && x < width; ++x) {
                        gpis_adaptive_record *rec = &records[x / 4 + (size_t)(y / 4) * vw];
                        size_t pix = (size_t)y * width + x;
                        float sum = 0.0f;
                        uint32_t h = 0;
                        for (uint32_t i = 0; i < rec->next_sample_count; ++i) {
                            size_t at = pix * k_have + rec->sample_index + i;
                            float c = clamp_sample(values[at]);
                            add_sample(rec, c);
                            sum += c;
                            h += hits[at];
                        }
                        radiance_sum[pix] += sum;
                        sample_count[pix] += rec->next_sample_count;
                        if (hit_count) hit_count[pix] += h;
                        info->samples += rec->next_sample_count;
                    }
        info->passes_rendered++;
        cur = next;
    }
    for (size_t r = 0; r < n_records; ++r)
        records[r].sample_index += records[r].next_sample_count;
    return 0;
}
