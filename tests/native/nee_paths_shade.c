/* TEST INFRASTRUCTURE: the per-bounce set-up, shade, bounce and sums of the multi-bounce conductor NEE / MIS estimator on scene S,
 * for the CPU composite of gpis_render_scene_s_nee_paths (tests/nee_paths_ref.py).  Plain C in float, compiled with the
 * restatement flags (no FMA, no contraction).
 *
 * The arithmetic and its association order are those of oracle/gpis_oracle.c (scene_nee_sample from `scheme = o.scheme` to
 * `return L`, nee_scene_range); tests/test_nee_paths_cpu.py pins the helpers against the oracle's pinning surface and the whole
 * file against oracle_render_scene_s_nee by composing a frame of max_path_bounces = 2 through it.  The stream is used in the
 * serial order, draw by draw: after jx, jy and the first march jitter, per hit
 *   [z, disk pairs until 1e-12 < d2 < 1]                     schemes NEE and MIS (nee_paths_setup)
 *   [jitter of the light shadow segment]                     when it is marched: F * neePDF(half vector) != 0 and (p, d) has a chord
 *   [jitter of the phase shadow segment]                     when it is marched: schemes UNI and MIS, w inside the cap, (p, w) has a chord
 *   [jitter of the next path segment]                        when the path goes on: thr * F != 0, (p, w) has a chord, b + 2 < max
 * Per sample: thr = 1, E = 0; per bounce thr = thr * weight[0]; E = E + thr * L; thr = thr * F.
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

static float conductor_reflectance(float eta, float k, float cosThetaI)   /* Fresnel.hpp:102-123 */
{
    if (eta == 0 && k == 0)
        return 1;
    float cosThetaISq = cosThetaI * cosThetaI;
    float sinThetaISq = 1.0f - cosThetaISq > 0.0f ? 1.0f - cosThetaISq : 0.0f;
    float sinThetaIQu = sinThetaISq * sinThetaISq;
    float innerTerm = eta * eta - k * k - sinThetaISq;
    float q = innerTerm * innerTerm + 4.0f * eta * eta * k * k;
    float aSqPlusBSq = sqrtf(q > 0.0f ? q : 0.0f);
    float h = (aSqPlusBSq + innerTerm) * 0.5f;
    float a = sqrtf(h > 0.0f ? h : 0.0f);
    float Rs = ((aSqPlusBSq + cosThetaISq) - (2.0f * a * cosThetaI)) /
               ((aSqPlusBSq + cosThetaISq) + (2.0f * a * cosThetaI));
    float Rp = ((cosThetaISq * aSqPlusBSq + sinThetaIQu) - (2.0f * a * cosThetaI * sinThetaISq)) /
               ((cosThetaISq * aSqPlusBSq + sinThetaIQu) + (2.0f * a * cosThetaI * sinThetaISq));
    return 0.5f * (Rs + Rs * Rp);
}
static float power_heuristic(float pdf0, float pdf1) { return (pdf0 * pdf0) / (pdf0 * pdf0 + pdf1 * pdf1); }
static float spherical_cap_pdf(float cosThetaMax) { return (0.5f * (1.0f / 3.1415926536f)) / (1.0f - cosThetaMax); }

/* ---- the helpers, for the pins against the oracle's pinning surface */
float nee_paths_conductor_reflectance(float eta, float k, float c) { return conductor_reflectance(eta, k, c); }
float nee_paths_power_heuristic(float a, float b) { return power_heuristic(a, b); }
float nee_paths_spherical_cap_pdf(float c) { return spherical_cap_pdf(c); }
void nee_paths_tangent_frame(const float *n, float *o)
{
    frame f = frame_from_normal(v3(n[0], n[1], n[2]));
    o[0] = f.tangent.x; o[1] = f.tangent.y; o[2] = f.tangent.z;
    o[3] = f.bitangent.x; o[4] = f.bitangent.y; o[5] = f.bitangent.z;
    o[6] = f.normal.x; o[7] = f.normal.y; o[8] = f.normal.z;
}
void nee_paths_frame_to_local(const float *n, const float *p, float *o)
{
    frame f = frame_from_normal(v3(n[0], n[1], n[2]));
    v3f r = to_local(&f, v3(p[0], p[1], p[2]));
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
}
void nee_paths_frame_to_global(const float *n, const float *p, float *o)
{
    frame f = frame_from_normal(v3(n[0], n[1], n[2]));
    v3f r = to_global(&f, v3(p[0], p[1], p[2]));
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
}

/* the state of sample (x, y, spp)'s stream after jx, jy and the first march jitter */
uint64_t nee_paths_stream(const gpis_scene_s *s, uint32_t x, uint32_t y, uint32_t spp)
{
    uint64_t g = (uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s->scene_seed) + 1u);
    (void)pcg_next_i(&g); (void)pcg_next_i(&g);            /* set_state discards next2D() */
    (void)pcg_next_i(&g); (void)pcg_next_i(&g); (void)pcg_next_i(&g);
    return g;
}

/* what one hit carries from the set-up to the gather (numpy mirror: nee_paths_ref.HIT) */
typedef struct {
    float d[3];               /* sampled light direction */
    float w[3];               /* mirror direction */
    float F;
    float thr;                /* throughput at the hit: weight[0] included, F not */
    int32_t scheme;
    uint8_t hit;              /* this bounce's segment ended on the surface */
    uint8_t want_light, want_phase, want_pdf_normal;      /* neePDF + neeGrad(half vector) / w sees the cap / neePDF(normal) */
    float pdf_half, grad_half[3], pdf_normal;             /* filled by the caller between set-up and shade */
    uint8_t go_light, go_phase;                           /* shadow segments to march */
    uint8_t vis_light, vis_phase;                         /* filled by the caller between shade and gather */
    float contrib_light, contrib_phase;
} nee_paths_hit;

/* After sampleDistance of the live paths: segment counts, !ok / exited, thr * weight[0], and for the hits the light direction
 * with its half-vector query, the mirror direction, the cap test and the query at the sampled normal.  alive[i] becomes "hit". */
void nee_paths_setup(const gpis_scene_s *s, const gpis_surface_s *sf, size_t n, uint8_t *alive, const gpis_ray_in *rays, const gpis_seg_out *seg,
                     const gpis_cond_coeff *coeff, uint64_t *rng, float *throughput, uint32_t *segs, nee_paths_hit *hits,
                     gpis_nee_query *q_half, gpis_nee_query *q_normal)
{
    const v3f capDir = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        nee_paths_hit *x = &hits[i];
        memset(x, 0, sizeof *x);
        if (!alive[i])
            continue;
        segs[i] += 1;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok) { alive[i] = 0; continue; }
        throughput[i] = throughput[i] * o->weight[0];
        if (o->exited) { alive[i] = 0; continue; }
        const gpis_ray_in *ray = &rays[i];
        x->hit = 1;
        x->thr = throughput[i];
        x->scheme = o->scheme;
        double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
        double len = sqrt(ax * ax + ay * ay + az * az);
        const v3f nn = v3((float)(ax / len), (float)(ay / len), (float)(az / len));
        const frame fr = frame_from_normal(nn);
        const v3f dir = v3(ray->dir[0], ray->dir[1], ray->dir[2]);
        const v3f wi = normalized3(to_local(&fr, v3(-dir.x, -dir.y, -dir.z)));
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        x->F = sf->albedo * conductor_reflectance(sf->eta, sf->k, wi.z);
        gpis_nee_query q;
        memset(&q, 0, sizeof q);
        q.ray_dir[0] = dir.x; q.ray_dir[1] = dir.y; q.ray_dir[2] = dir.z;
        q.p[0] = p.x; q.p[1] = p.y; q.p[2] = p.z;
        q.t_segment = o->sample_t;
        q.info_t = ray->info_t + o->sample_t;
        q.pixel[0] = ray->pixel[0]; q.pixel[1] = ray->pixel[1]; q.spp = ray->spp; q.segment = ray->segment;
        q.scene_seed = ray->scene_seed;
        q.coeff = coeff[i];
        if (x->scheme != GPIS_UNI) {   /* volumeLightSample */
            uint64_t g = rng[i];
            float z = pcg_next_1d(&g) * (1.0f - sf->cap_cos) + sf->cap_cos;
            float dx, dy, d2;
            do {
                dx = 2.f * pcg_next_1d(&g) - 1.f;
                dy = 2.f * pcg_next_1d(&g) - 1.f;
                d2 = dx * dx + dy * dy;
            } while (!(d2 < 1.f) || !(d2 > 1e-12f));
            rng[i] = g;
            float rr = 1.0f - z * z;
            float rad = sqrtf(rr > 0.f ? rr : 0.f) / sqrtf(d2);
            frame cf = frame_from_normal(capDir);
            v3f d = to_global(&cf, v3(dx * rad, dy * rad, z));
            v3f wo = normalized3(to_local(&fr, d));
            v3f sum = v3(wi.x + wo.x, wi.y + wo.y, wi.z + wo.z);
            v3f nl = v3(sum.x * 0.5f, sum.y * 0.5f, sum.z * 0.5f);
            v3f nw = normalized3(to_global(&fr, nl));
            x->d[0] = d.x; x->d[1] = d.y; x->d[2] = d.z;
            q_half[i] = q;
            q_half[i].normal[0] = nw.x; q_half[i].normal[1] = nw.y; q_half[i].normal[2] = nw.z;
            x->want_light = 1;
        }
        /* ConductorBsdf::sample mirrors about the sampled normal: the phase sample's direction and the bounce's */
        const v3f w = normalized3(to_global(&fr, v3(-wi.x, -wi.y, wi.z)));
        x->w[0] = w.x; x->w[1] = w.y; x->w[2] = w.z;
        if (x->scheme != GPIS_NEE) {   /* volumePhaseSample */
            float t0, t1;
            if (!(dot3(w, capDir) < sf->cap_cos) && sphere_chord(p, w, s->bound_radius, &t0, &t1)) {
                x->want_phase = 1;
                if (x->scheme != GPIS_UNI) {
                    q_normal[i] = q;
                    q_normal[i].normal[0] = nn.x; q_normal[i].normal[1] = nn.y; q_normal[i].normal[2] = nn.z;
                    x->want_pdf_normal = 1;
                }
            }
        }
    }
}

/* handleVolume's copy of the state at the hit: segment word + 1, bounce + 1, first_scatter = 0 */
static gpis_ray_in state_copy(const gpis_ray_in *ray, const gpis_seg_out *o)
{
    gpis_ray_in sh0;
    memset(&sh0, 0, sizeof sh0);
    sh0.pos[0] = o->p[0]; sh0.pos[1] = o->p[1]; sh0.pos[2] = o->p[2];
    sh0.near_t = 0.f;
    sh0.pixel[0] = ray->pixel[0]; sh0.pixel[1] = ray->pixel[1]; sh0.spp = ray->spp;
    sh0.segment = ray->segment + 1;
    sh0.scene_seed = ray->scene_seed;
    sh0.info_t = ray->info_t + o->sample_t;
    sh0.first_scatter = 0;
    sh0.bounce = ray->bounce + 1;
    sh0.last_val = o->last_val;
    sh0.last_gp_id = o->gp_id;
    sh0.last_aniso[0] = o->aniso[0]; sh0.last_aniso[1] = o->aniso[1]; sh0.last_aniso[2] = o->aniso[2];
    return sh0;
}

/* After neePDF / neeGrad: the shadow segments that are marched and their contributions, then the bounce and the next ray.
 * alive[i] becomes "rays[i] is the next path segment". */
void nee_paths_shade(const gpis_scene_s *s, const gpis_surface_s *sf, size_t n, int bounce, int max_bounces, uint8_t *alive, gpis_ray_in *rays,
                     const gpis_seg_out *seg, uint64_t *rng, float *throughput, uint32_t *segs, nee_paths_hit *hits,
                     gpis_ray_in *shadow_light, gpis_ray_in *shadow_phase)
{
    const float pdf_l = spherical_cap_pdf(sf->cap_cos);
    for (size_t i = 0; i < n; ++i) {
        nee_paths_hit *x = &hits[i];
        if (!x->hit)
            continue;
        const gpis_seg_out *o = &seg[i];
        const gpis_ray_in ray = rays[i];
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        const gpis_ray_in sh0 = state_copy(&ray, o);
        uint64_t g = rng[i];
        if (x->want_light) {
            const float pdf = x->pdf_half;
            const float f = x->F * pdf;
            const v3f d = v3(x->d[0], x->d[1], x->d[2]);
            float t0, t1;
            if (f != 0.0f && sphere_chord(p, d, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = sh0;
                sh.dir[0] = d.x; sh.dir[1] = d.y; sh.dir[2] = d.z;
                sh.far_t = t1;
                sh.u_jitter = pcg_next_1d(&g);
                sh.last_aniso[0] = x->grad_half[0]; sh.last_aniso[1] = x->grad_half[1]; sh.last_aniso[2] = x->grad_half[2];
                shadow_light[i] = sh;
                float lightF = f * (1.f * sf->cap_radiance) / pdf_l;
                if (x->scheme != GPIS_NEE)
                    lightF *= power_heuristic(pdf_l, pdf);
                x->contrib_light = lightF;
                x->go_light = 1;
                segs[i] += 1;
            }
        }
        const v3f w = v3(x->w[0], x->w[1], x->w[2]);
        float t0, t1 = 0.f;
        const int chord = sphere_chord(p, w, s->bound_radius, &t0, &t1);
        if (x->want_phase) {           /* the chord exists (nee_paths_setup) */
            gpis_ray_in sh = sh0;
            sh.dir[0] = w.x; sh.dir[1] = w.y; sh.dir[2] = w.z;
            sh.far_t = t1;
            sh.u_jitter = pcg_next_1d(&g);
            shadow_phase[i] = sh;
            float phaseF = (1.f * sf->cap_radiance) * x->F;
            if (x->scheme != GPIS_UNI)
                phaseF *= power_heuristic(x->pdf_normal, pdf_l);
            x->contrib_phase = phaseF;
            x->go_phase = 1;
            segs[i] += 1;
        }
        /* the bounce */
        throughput[i] = x->thr * x->F;
        int lives = !(throughput[i] == 0.0f) && chord && bounce + 2 < max_bounces;
        if (lives) {
            gpis_ray_in next = sh0;
            next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
            next.far_t = t1;
            next.u_jitter = pcg_next_1d(&g);
            rays[i] = next;
        }
        rng[i] = g;
        alive[i] = lives ? 1 : 0;
    }
}

/* After the shadow marches: E = E + thr * L for every hit */
void nee_paths_gather(const gpis_surface_s *sf, size_t n, const nee_paths_hit *hits, float *emission)
{
    for (size_t i = 0; i < n; ++i) {
        const nee_paths_hit *x = &hits[i];
        if (!x->hit)
            continue;
        float L = 0.f;
        if (x->go_light) {
            float e = (x->vis_light ? 1.f : 0.f) * sf->cap_radiance;
            if (e != 0.0f)
                L += x->contrib_light;
        }
        if (x->go_phase) {
            float e = (x->vis_phase ? 1.f : 0.f) * sf->cap_radiance;
            if (e != 0.0f)
                L += x->contrib_phase;
        }
        emission[i] = emission[i] + x->thr * L;
    }
}

/* Adds the n samples, given in the order (pixel, sample), to the image and the counts: pixel_of[i] is the sample's index
 * y*width+x; samples of one pixel are consecutive.  Each pixel's emissions are summed from zero in order and the sum is added to
 * the image once, which is what a driver call does. */
void nee_paths_sum(size_t n, const uint32_t *pixel_of, const float *emission, const uint32_t *segs, float *radiance_sum, uint32_t *seg_count)
{
    size_t i = 0;
    while (i < n) {
        const uint32_t pix = pixel_of[i];
        float acc = 0.f;
        uint32_t cnt = 0;
        for (; i < n && pixel_of[i] == pix; ++i) {
            acc += emission[i];
            cnt += segs[i];
        }
        radiance_sum[pix] += acc;
        seg_count[pix] += cnt;
    }
}

size_t nee_paths_hit_size(void) { return sizeof(nee_paths_hit); }
