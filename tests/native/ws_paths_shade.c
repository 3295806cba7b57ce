/* TEST INFRASTRUCTURE: the camera step, the per-bounce shade step and the emission and pixel sums of the multi-bounce estimator on
 * scene S, for the CPU composite of the weight-space path frame (tests/ws_paths_ref.py).  Plain C, compiled with the restatement
 * flags (no FMA, no contraction).
 *
 * The arithmetic and its association order are those of oracle/gpis_oracle.c (oracle_scene_s_primary, scene_paths_sample,
 * paths_range), which the sparse-convolution image tests pin against the device's k_paths_begin / k_paths_shade /
 * k_paths_accumulate; tests/test_ws_paths_cpu.py pins this file against that oracle by composing a sparse-convolution frame
 * through it.  Per sample one PCG32 stream seeded with xxhash32(x, y, spp, scene_seed) + 1:
 *   jx, jy, u_march; then per bounce [u_shadow when NEE runs], the disk pairs, [u_march of the next segment when the path lives on]
 *   light  l = light_dir * (1 / sqrtf(((0 + lx lx) + ly ly) + lz lz))                            (float)
 *   normal n = float(aniso / sqrt((ax ax + ay ay) + az az))                                       (double, rounded per component)
 *   frame    = TangentFrame(n) (Duff), wi = normalized(toLocal(-dir)), wo = normalized(toLocal(l))
 *   NEE (bounce < max - 1, wi.z > 0, wo.z > 0, the ray (p, l) meets the bound): contrib = thr * (((albedo * (1/pi_f)) * wo.z) * L)
 *   bounce (wi.z > 0): w = normalized(toGlobal(dx, dy, sqrtf(max(1 - d2, 0)))), thr *= albedo, lives on when (p, w) meets the bound
 *   sample emission += visible ? contrib : 0, in bounce order; pixel acc = 0; acc += emission in sample order; image += acc
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

/* The camera step of sample (x, y, spp): the segment-0 ray and the stream's state after jx, jy, u_march.  Returns 0 when the ray
 * misses the bounding sphere (the sample's emission is 0 and nothing is marched). */
int ws_paths_begin(const gpis_scene_s *s, uint32_t x, uint32_t y, uint32_t spp, gpis_ray_in *ray, uint64_t *rng)
{
    uint64_t g = (uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s->scene_seed) + 1u);
    (void)pcg_next_i(&g); (void)pcg_next_i(&g);            /* set_state discards next2D() */
    float jx = pcg_next_1d(&g), jy = pcg_next_1d(&g), u0 = pcg_next_1d(&g);
    const float pi_f = 3.1415926536f;
    float fov_rad = s->cam_fov_deg * (pi_f / 180.0f);
    float plane_dist = 1.0f / tanf(fov_rad * 0.5f);
    float ratio = (float)s->height / (float)s->width;
    float psx = 1.0f / (float)s->width;
    v3f local = normalized3(v3(-1.0f + ((float)x + jx) * 2.0f * psx, ratio - ((float)y + jy) * 2.0f * psx, plane_dist));
    v3f d = v3(local.x, local.y, -local.z);
    v3f o = v3(s->cam_pos[0], s->cam_pos[1], s->cam_pos[2]);
    memset(ray, 0, sizeof *ray);
    ray->pos[0] = o.x; ray->pos[1] = o.y; ray->pos[2] = o.z;
    ray->dir[0] = d.x; ray->dir[1] = d.y; ray->dir[2] = d.z;
    ray->pixel[0] = x; ray->pixel[1] = y; ray->spp = spp; ray->segment = 0;
    ray->scene_seed = s->scene_seed; ray->info_t = 0.f; ray->u_jitter = u0;
    ray->first_scatter = 1;
    *rng = g;
    float t0, t1;
    if (!sphere_chord(o, d, s->bound_radius, &t0, &t1))
        return 0;
    ray->near_t = t0; ray->far_t = t1;
    return 1;
}

/* what ended a path at this bounce (end[i]); 0 while it lives on */
enum { WS_PATHS_LIVES = 0, WS_PATHS_NOT_OK = 1, WS_PATHS_EXITED = 2, WS_PATHS_BELOW = 3, WS_PATHS_NO_CHORD = 4 };

/* One bounce level over n paths.  In: alive[i], rays[i] (the segment of this bounce), seg[i] (its sampleDistance result), rng[i],
 * throughput[i].  Out, for the paths that were alive: nee[i] / shadow[i] / contrib[i] (a shadow segment is to be marched),
 * end[i], and when the path lives on rays[i] (the next segment), with rng[i] / throughput[i] / alive[i] advanced. */
void ws_paths_shade(const gpis_scene_s *s, size_t n, int bounce, int max_bounces, float albedo, gpis_ray_in *rays, const gpis_seg_out *seg,
                    uint64_t *rng, float *throughput, uint8_t *alive, gpis_ray_in *shadow, float *contrib, uint8_t *nee, uint8_t *end)
{
    const v3f l = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        nee[i] = 0; end[i] = WS_PATHS_LIVES; contrib[i] = 0.f;
        if (!alive[i])
            continue;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok) { alive[i] = 0; end[i] = WS_PATHS_NOT_OK; continue; }
        float thr = throughput[i] * o->weight[0];
        if (o->exited) { alive[i] = 0; end[i] = WS_PATHS_EXITED; throughput[i] = thr; continue; }
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
        if (bounce < max_bounces - 1) {
            const v3f wo = normalized3(to_local(&fr, l));
            if (wi.z > 0.0f && wo.z > 0.0f) {
                const float f = albedo * (1.0f / 3.1415926536f) * wo.z;
                float t0, t1;
                if (sphere_chord(p, l, s->bound_radius, &t0, &t1)) {
                    gpis_ray_in sh = next;
                    sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                    sh.far_t = t1;
                    sh.segment = (uint32_t)bounce + 1;
                    sh.u_jitter = pcg_next_1d(&g);
                    shadow[i] = sh;
                    contrib[i] = thr * (f * s->light_radiance);
                    nee[i] = 1;
                }
            }
        }
        int lives = wi.z > 0.0f;
        if (!lives)
            end[i] = WS_PATHS_BELOW;
        else {
            float dx, dy, d2;
            do {
                dx = 2.f * pcg_next_1d(&g) - 1.f;
                dy = 2.f * pcg_next_1d(&g) - 1.f;
                d2 = dx * dx + dy * dy;
            } while (!(d2 < 1.f));
            const float rem = 1.0f - d2;
            const v3f w = normalized3(to_global(&fr, v3(dx, dy, sqrtf(rem > 0.f ? rem : 0.f))));
            thr *= albedo;
            float t0, t1;
            lives = sphere_chord(p, w, s->bound_radius, &t0, &t1);
            if (!lives)
                end[i] = WS_PATHS_NO_CHORD;
            else {
                next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
                next.far_t = t1;
                next.segment = (uint32_t)bounce + 1;
                next.u_jitter = pcg_next_1d(&g);
                rays[i] = next;
            }
        }
        alive[i] = lives ? 1 : 0;
        throughput[i] = thr;
        rng[i] = g;
    }
}

/* emission[i] += visible[i] ? contrib[i] : 0 for the paths whose shadow segment was marched */
void ws_paths_nee_add(size_t n, const uint8_t *nee, const uint8_t *visible, const float *contrib, float *emission)
{
    for (size_t i = 0; i < n; ++i)
        if (nee[i])
            emission[i] += visible[i] ? contrib[i] : 0.f;
}

/* Adds the n samples, given in the order (pixel, sample), to the image: pixel_of[i] is the sample's index y*width+x; samples of
 * one pixel are consecutive.  Each pixel's emissions are summed from zero in order and the sum is added to the image once, which
 * is what a driver call does. */
void ws_paths_sum(size_t n, const uint32_t *pixel_of, const float *emission, float *radiance_sum)
{
    size_t i = 0;
    while (i < n) {
        const uint32_t pix = pixel_of[i];
        float acc = 0.f;
        for (; i < n && pixel_of[i] == pix; ++i)
            acc += emission[i];
        radiance_sum[pix] += acc;
    }
}
