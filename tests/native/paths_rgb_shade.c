/* TEST INFRASTRUCTURE: the set-up, the per-bounce shade step with the medium's emission, the NEE add and the pixel sums of the RGB
 * multi-bounce estimator on scene S, for the CPU composite of gpis_render_scene_s_paths_rgb (tests/paths_rgb_ref.py).  Plain C in
 * float, compiled with the restatement flags (no FMA, no contraction).
 *
 * The arithmetic and its association order are those of oracle/gpis_oracle.c (scene_paths_sample, paths_range) per channel;
 * tests/test_paths_rgb_cpu.py pins this file against that oracle: without emission every channel of a composite must equal
 * oracle_render_scene_s_paths of the medium and albedo with that channel rolled to the front.  Per sample one PCG32 stream seeded
 * with xxhash32(x, y, spp, scene_seed) + 1: jx, jy, u_march; then per bounce [u_shadow when NEE runs], the disk pairs, [u_march of
 * the next segment when the path lives on].  thr[c] = 1, em[c] = 0; with E = "the medium emits" and B = max_bounces, per segment b:
 *   !ok ends the path; on a hit when E: em[c] = em[c] + (thr[c] * e[c]), e = float(emission(ro + rd * t)) from the caller;
 *   thr[c] = thr[c] * weight[c]; exited ends the path; b == B - 1 (marched only when E) ends the path;
 *   NEE (wi.z > 0, wo.z > 0, (p, l) meets the bound): contrib[c] = thr[c] * (((albedo[c] * (1/pi_f)) * wo.z) * L), added to em after
 *   the shadow march when visible; bounce (wi.z > 0): thr[c] *= albedo[c], lives on when (p, w) meets the bound.
 * Arrays of three channels are interleaved here: [3 * i + c].
 */

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "gpis.h"

#define PRIME32_2 2246822519U
#define PRIME32_3 3266489917U
#define PRIME32_4 668265263U
#define PRIME32_5 374761393U

static uint32_t rotl17(uint32_t h) { return (h << 17) | (h >> 15); }
static uint32_t xxhash32_4(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    uint32_t h = w + PRIME32_5 + x * PRIME32_3;
    h = PRIME32_4 * rotl17(h);
    h += y * PRIME32_3;
    h = PRIME32_4 * rotl17(h);
    h += z * PRIME32_3;
    h = PRIME32_4 * rotl17(h);
    h = PRIME32_2 * (h ^ (h >> 15));
    h = PRIME32_3 * (h ^ (h >> 13));
    return h ^ (h >> 16);
}
static uint32_t pcg_next_i(uint64_t *s)
{
    uint64_t old = *s;
    *s = old * 6364136223846793005ULL + 1ULL;
    uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((0u - rot) & 31u));
}
static float pcg_next_1d(uint64_t *s)
{
    union { uint32_t u; float f; } c;
    c.u = (pcg_next_i(s) >> 9u) | 0x3F800000u;
    return c.f - 1.0f;
}

typedef struct { float x, y, z; } v3f;
static v3f v3(float x, float y, float z) { v3f r = {x, y, z}; return r; }
static float dot3(v3f a, v3f b) { float s = a.x * b.x; s += a.y * b.y; s += a.z * b.z; return s; }
static v3f normalized3(v3f a)
{
    float r = 0.f;
    r += a.x * a.x; r += a.y * a.y; r += a.z * a.z;
    float inv = 1.0f / sqrtf(r);
    return v3(a.x * inv, a.y * inv, a.z * inv);
}
typedef struct { v3f normal, tangent, bitangent; } frame;
static frame frame_from_normal(v3f n)
{
    frame f;
    f.normal = normalized3(n);
    float sign = copysignf(1.0f, f.normal.z);
    const float a = -1.0f / (sign + f.normal.z);
    const float b = f.normal.x * f.normal.y * a;
    f.tangent = normalized3(v3(1.0f + sign * f.normal.x * f.normal.x * a, sign * b, -sign * f.normal.x));
    f.bitangent = normalized3(v3(b, sign + f.normal.y * f.normal.y * a, -f.normal.y));
    return f;
}
static v3f to_local(const frame *f, v3f p) { return v3(dot3(f->tangent, p), dot3(f->bitangent, p), dot3(f->normal, p)); }
static v3f to_global(const frame *f, v3f p)
{
    return v3((f->tangent.x * p.x + f->bitangent.x * p.y) + f->normal.x * p.z, (f->tangent.y * p.x + f->bitangent.y * p.y) + f->normal.y * p.z,
              (f->tangent.z * p.x + f->bitangent.z * p.y) + f->normal.z * p.z);
}

/* ray / sphere(|x| = R) in double; 0 on a miss */
static int sphere_chord(v3f o, v3f d, float R, float *t0, float *t1)
{
    double ox = o.x, oy = o.y, oz = o.z, dx = d.x, dy = d.y, dz = d.z;
    double a = dx * dx + dy * dy + dz * dz;
    double b = ox * dx + oy * dy + oz * dz;
    double c = ox * ox + oy * oy + oz * oz - (double)R * (double)R;
    double disc = b * b - a * c;
    if (!(disc > 0.0))
        return 0;
    double sq = sqrt(disc);
    double ta = (-b - sq) / a, tb = (-b + sq) / a;
    if (tb <= 0.0)
        return 0;
    if (ta < 0.0) ta = 0.0;
    *t0 = (float)ta; *t1 = (float)tb;
    return 1;
}

static v3f light_of(const gpis_scene_s *s)
{
    float lx = s->light_dir[0], ly = s->light_dir[1], lz = s->light_dir[2];
    float l2 = 0.f;
    l2 += lx * lx; l2 += ly * ly; l2 += lz * lz;
    float inv = 1.0f / sqrtf(l2);
    return v3(lx * inv, ly * inv, lz * inv);
}

/* the state of sample (x, y, spp)'s stream after jx, jy and the first march jitter */
uint64_t paths_rgb_stream(const gpis_scene_s *s, uint32_t x, uint32_t y, uint32_t spp)
{
    uint64_t g = (uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s->scene_seed) + 1u);
    (void)pcg_next_i(&g); (void)pcg_next_i(&g);            /* set_state discards next2D() */
    (void)pcg_next_i(&g); (void)pcg_next_i(&g); (void)pcg_next_i(&g);
    return g;
}

/* n path states: thr = 1, em = 0, no segment marched */
void paths_rgb_begin(size_t n, float *thr3, float *em3, uint32_t *segs)
{
    for (size_t i = 0; i < 3 * n; ++i) { thr3[i] = 1.f; em3[i] = 0.f; }
    for (size_t i = 0; i < n; ++i) segs[i] = 0;
}

/* After sampleDistance of the live paths: the segment counts, hit[i] = ok && !exited, and for the hits the point the emission is
 * evaluated at: ro + rd * t with ro the ray position widened to double, rd the direction normalised in double, t = seg.t
 * (GPM.cpp:317; the point of gpis_mean_color_emission_*). */
void paths_rgb_setup(size_t n, const uint8_t *alive, const gpis_ray_in *rays, const gpis_seg_out *seg, uint32_t *segs, uint8_t *hit, double *p3)
{
    for (size_t i = 0; i < n; ++i) {
        hit[i] = 0;
        p3[3 * i] = p3[3 * i + 1] = p3[3 * i + 2] = 0.;
        if (!alive[i])
            continue;
        segs[i] += 1;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok || o->exited)
            continue;
        hit[i] = 1;
        const gpis_ray_in *ray = &rays[i];
        double rx = ray->dir[0], ry = ray->dir[1], rz = ray->dir[2];
        double r = 0.;
        r += rx * rx; r += ry * ry; r += rz * rz;
        double inv = 1.0 / sqrt(r);
        rx *= inv; ry *= inv; rz *= inv;
        p3[3 * i] = (double)ray->pos[0] + o->t * rx;
        p3[3 * i + 1] = (double)ray->pos[1] + o->t * ry;
        p3[3 * i + 2] = (double)ray->pos[2] + o->t * rz;
    }
}

/* One bounce level over n paths.  In: alive[i], rays[i] (the segment of this bounce), seg[i] (its sampleDistance result), hit[i]
 * and, when `emissive`, e3 (the medium's emission at the hits), rng[i], thr3, em3.  Out, for the paths that were alive:
 * thr_before3 (the throughput the emission term used: before the weight), nee[i] / shadow[i] / contrib3 (a shadow segment is to
 * be marched; counted in segs[i]), and when the path lives on rays[i] (the next segment), with rng / thr3 / alive advanced. */
void paths_rgb_shade(const gpis_scene_s *s, size_t n, int bounce, int max_bounces, int emissive, const float *albedo, gpis_ray_in *rays,
                     const gpis_seg_out *seg, const uint8_t *hit, const float *e3, uint64_t *rng, float *thr3, float *em3, uint32_t *segs,
                     uint8_t *alive, float *thr_before3, gpis_ray_in *shadow, float *contrib3, uint8_t *nee)
{
    const v3f l = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        nee[i] = 0;
        for (int c = 0; c < 3; ++c) { contrib3[3 * i + c] = 0.f; thr_before3[3 * i + c] = 0.f; }
        if (!alive[i])
            continue;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok) { alive[i] = 0; continue; }
        float thr[3];
        for (int c = 0; c < 3; ++c) thr[c] = thr3[3 * i + c];
        if (hit[i] && emissive)
            for (int c = 0; c < 3; ++c) {
                thr_before3[3 * i + c] = thr[c];
                const float prod = thr[c] * e3[3 * i + c];
                em3[3 * i + c] = em3[3 * i + c] + prod;
            }
        for (int c = 0; c < 3; ++c) thr[c] = thr[c] * o->weight[c];
        if (o->exited || bounce >= max_bounces - 1) {
            alive[i] = 0;
            for (int c = 0; c < 3; ++c) thr3[3 * i + c] = thr[c];
            continue;
        }
        const gpis_ray_in ray = rays[i];
        uint64_t g = rng[i];
        double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
        double len = sqrt(ax * ax + ay * ay + az * az);
        const v3f nn = v3((float)(ax / len), (float)(ay / len), (float)(az / len));
        const frame fr = frame_from_normal(nn);
        const v3f wi = normalized3(to_local(&fr, v3(-ray.dir[0], -ray.dir[1], -ray.dir[2])));
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        gpis_ray_in next;
        memset(&next, 0, sizeof next);
        next.pos[0] = p.x; next.pos[1] = p.y; next.pos[2] = p.z;
        next.near_t = 0.f;
        next.pixel[0] = ray.pixel[0]; next.pixel[1] = ray.pixel[1]; next.spp = ray.spp;
        next.scene_seed = ray.scene_seed;
        next.info_t = ray.info_t + o->sample_t;
        next.first_scatter = 0;
        next.bounce = ray.bounce + 1;
        next.last_val = o->last_val;
        next.last_gp_id = o->gp_id;
        next.last_aniso[0] = o->aniso[0]; next.last_aniso[1] = o->aniso[1]; next.last_aniso[2] = o->aniso[2];
        const v3f wo = normalized3(to_local(&fr, l));
        if (wi.z > 0.0f && wo.z > 0.0f) {
            float t0, t1;
            if (sphere_chord(p, l, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = next;
                sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                sh.far_t = t1;
                sh.segment = (uint32_t)bounce + 1;
                sh.u_jitter = pcg_next_1d(&g);
                shadow[i] = sh;
                for (int c = 0; c < 3; ++c) {
                    const float f = albedo[c] * (1.0f / 3.1415926536f) * wo.z;
                    contrib3[3 * i + c] = thr[c] * (f * s->light_radiance);
                }
                segs[i] += 1;
                nee[i] = 1;
            }
        }
        int lives = wi.z > 0.0f;
        if (lives) {
            float dx, dy, d2;
            do {
                dx = 2.f * pcg_next_1d(&g) - 1.f;
                dy = 2.f * pcg_next_1d(&g) - 1.f;
                d2 = dx * dx + dy * dy;
            } while (!(d2 < 1.f));
            const float rem = 1.0f - d2;
            const v3f w = normalized3(to_global(&fr, v3(dx, dy, sqrtf(rem > 0.f ? rem : 0.f))));
            for (int c = 0; c < 3; ++c) thr[c] *= albedo[c];
            float t0, t1;
            lives = sphere_chord(p, w, s->bound_radius, &t0, &t1);
            if (lives) {
                next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
                next.far_t = t1;
                next.segment = (uint32_t)bounce + 1;
                next.u_jitter = pcg_next_1d(&g);
                rays[i] = next;
            }
        }
        alive[i] = lives ? 1 : 0;
        for (int c = 0; c < 3; ++c) thr3[3 * i + c] = thr[c];
        rng[i] = g;
    }
}

/* em[c] += visible ? contrib[c] : 0 for the paths whose shadow segment was marched */
void paths_rgb_nee_add(size_t n, const uint8_t *nee, const uint8_t *visible, const float *contrib3, float *em3)
{
    for (size_t i = 0; i < n; ++i)
        if (nee[i])
            for (int c = 0; c < 3; ++c)
                em3[3 * i + c] += visible[i] ? contrib3[3 * i + c] : 0.f;
}

/* Adds the n samples, given in the order (pixel, sample), to the image and the counts: pixel_of[i] is the sample's index
 * y*width+x; samples of one pixel are consecutive.  Per channel each pixel's emissions are summed from zero in order and the sum
 * is added to the image once, which is what a driver call does. */
void paths_rgb_sum(size_t n, const uint32_t *pixel_of, const float *em3, const uint32_t *segs, float *radiance_sum3, uint32_t *seg_count)
{
    size_t i = 0;
    while (i < n) {
        const uint32_t pix = pixel_of[i];
        float acc[3] = {0.f, 0.f, 0.f};
        uint32_t cnt = 0;
        for (; i < n && pixel_of[i] == pix; ++i) {
            for (int c = 0; c < 3; ++c)
                acc[c] += em3[3 * i + c];
            cnt += segs[i];
        }
        for (int c = 0; c < 3; ++c)
            radiance_sum3[3 * (size_t)pix + c] += acc[c];
        seg_count[pix] += cnt;
    }
}
