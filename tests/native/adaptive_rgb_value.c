/* TEST INFRASTRUCTURE: plain-C restatement of what gpis_render_scene_s_paths_rgb_adaptive does to one Vec3f sample before it reaches
 * the image and the statistics: renderTile's clamp (PathTraceIntegrator.cpp:149-156: isinf of any component, any component above
 * 65536, else isnan of any component — the sample becomes Vec3f(0)) and Vec3f::luminance (Vec.hpp:218-222), which
 * SampleRecord::addSample(const Vec3f &) hands to addSample(float) (SampleRecord.hpp:52-55).  Compiled with the flags of
 * oracle/Makefile (contraction off): every product and every sum is rounded to float. */
#include <math.h>
#include <stddef.h>

static int clamped(const float *c)
{
    if (isinf(c[0]) || isinf(c[1]) || isinf(c[2]) || c[0] > 65536 || c[1] > 65536 || c[2] > 65536)
        return 1;
    if (isnan(c[0]) || isnan(c[1]) || isnan(c[2]))
        return 1;
    return 0;
}

static float luminance(const float *c)
{
    float a = c[0] * 0.2126f;
    float b = c[1] * 0.7152f;
    float ab = a + b;
    float d = c[2] * 0.0722f;
    return ab + d;
}

/* rgb_in[3n] -> rgb_out[3n] (the clamped sample), lum[n] (its luminance), flag[n] (1: the clamp fired); each output may be NULL */
void adaptive_rgb_value_ref(size_t n, const float *rgb_in, float *rgb_out, float *lum, unsigned char *flag)
{
    for (size_t i = 0; i < n; ++i) {
        float v[3] = {rgb_in[3 * i], rgb_in[3 * i + 1], rgb_in[3 * i + 2]};
        int z = clamped(v);
        if (z) v[0] = v[1] = v[2] = 0.0f;
        if (rgb_out) { rgb_out[3 * i] = v[0]; rgb_out[3 * i + 1] = v[1]; rgb_out[3 * i + 2] = v[2]; }
        if (lum) lum[i] = luminance(v);
        if (flag) flag[i] = (unsigned char)z;
    }
}
