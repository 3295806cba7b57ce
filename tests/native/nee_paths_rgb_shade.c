/* TEST INFRASTRUCTURE: the per-bounce set-up, shade, bounce, gather and sums of the conductor NEE / MIS path estimator on scene S in
 * RGB with the medium's emission, for the CPU composite of gpis_render_scene_s_nee_paths_rgb (tests/nee_paths_rgb_ref.py).  Plain C
 * in float, compiled with the restatement flags (no FMA, no contraction).
 *
 * The geometry, the draws and their order are those of tests/native/nee_paths_shade.c (which tests/test_nee_paths_cpu.py pins to
 * the oracle); tests/test_nee_paths_rgb_cpu.py pins this file to that one: with equal channels and no emission every channel, the
 * segment counts and the per-bounce counts of a composite through this file equal the mono composite's.  Colour is carried by
 *   F[c] = albedo[c] * conductorReflectance(eta[c], k[c], wi.z)                       (Fresnel.hpp:136-143)
 *   f[c] = F[c] * neePDF(half vector); the light's shadow segment is marched unless f is zero in EVERY channel (Vec.hpp:452-458)
 *   lightF[c] = f[c] * cap_radiance[c] / pdf_l [* heuristic], phaseF[c] = cap_radiance[c] * F[c] [* heuristic]
 *   L = 0 for both estimators iff cap_radiance is zero in every channel
 * Per sample: thr[c] = 1, em[c] = 0; per bounce, on a hit: em[c] += thr[c] * e[c] (emissive media), thr[c] *= weight[c],
 * em[c] += thr[c] * L[c], thr[c] *= F[c]; the path ends when max(thr) == 0 (Vec.hpp:418-425).  An emissive medium marches the
 * segment max_bounces - 1 too: its hit only emits.  Colour arrays are interleaved here: channel c of sample i at [3 * i + c].
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


void nee_paths_rgb_fresnel(const gpis_surface_rgb_s *sf, float cosThetaI, float *F3)
{
    for (int c = 0; c < 3; ++c)
        F3[c] = sf->albedo[c] * conductor_reflectance(sf->eta[c], sf->k[c], cosThetaI);
}

/* the state of sample (x, y, spp)'s stream after jx, jy and the first march jitter */
uint64_t nee_paths_rgb_stream(const gpis_scene_s *s, uint32_t x, uint32_t y, uint32_t spp)
{
    uint64_t g = (uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s->scene_seed) + 1u);
    (void)pcg_next_i(&g); (void)pcg_next_i(&g);            /* set_state discards next2D() */
    (void)pcg_next_i(&g); (void)pcg_next_i(&g); (void)pcg_next_i(&g);
    return g;
}

/* what one hit carries from the set-up to the gather (numpy mirror: nee_paths_rgb_ref.HIT) */
typedef struct {
    float d[3];               /* sampled light direction */
    float w[3];               /* mirror direction */
    float F[3];
    float thr[3];             /* throughput at the hit: weight included, F not */
    int32_t scheme;
    uint8_t hit;              /* this bounce's segment ended on the surface and the estimators follow */
    uint8_t want_light, want_phase, want_pdf_normal;
    float pdf_half, grad_half[3], pdf_normal;             /* filled by the caller between set-up and shade */
    uint8_t go_light, go_phase;                           /* shadow segments to march */
    uint8_t vis_light, vis_phase;                         /* filled by the caller between shade and gather */
    float contrib_light[3], contrib_phase[3];
} nee_paths_rgb_hit;

/* After sampleDistance of the live paths: surf[i] = ok && !exited, and for those the point the emission is evaluated at: ro + rd * t
 * with ro widened to double, rd normalised in double, t = seg.t (GPM.cpp:317; the point of gpis_mean_color_emission_*). */
void nee_paths_rgb_points(size_t n, const uint8_t *alive, const gpis_ray_in *rays, const gpis_seg_out *seg, uint8_t *surf, double *p3)
{
    for (size_t i = 0; i < n; ++i) {
        surf[i] = 0;
        p3[3 * i] = p3[3 * i + 1] = p3[3 * i + 2] = 0.;
        if (!alive[i] || !seg[i].ok || seg[i].exited)
            continue;
        surf[i] = 1;
        const gpis_ray_in *ray = &rays[i];
        double rx = ray->dir[0], ry = ray->dir[1], rz = ray->dir[2];
        double r = 0.;
        r += rx * rx; r += ry * ry; r += rz * rz;
        double inv = 1.0 / sqrt(r);
        rx *= inv; ry *= inv; rz *= inv;
        p3[3 * i] = (double)ray->pos[0] + seg[i].t * rx;
        p3[3 * i + 1] = (double)ray->pos[1] + seg[i].t * ry;
        p3[3 * i + 2] = (double)ray->pos[2] + seg[i].t * rz;
    }
}

/* After sampleDistance of the live paths (and, when `emissive`, the emission e3 at the points above): segment counts, !ok / exited,
 * em += thr * e with thr BEFORE the weight, thr * weight, and — for bounce + 1 < max_bounces — for the hits the light direction
 * with its half-vector query, the mirror direction, the cap test and the query at the sampled normal.  alive[i] becomes "hit". */
void nee_paths_rgb_setup(const gpis_scene_s *s, const gpis_surface_rgb_s *sf, size_t n, int bounce, int max_bounces, int emissive, uint8_t *alive,
                         const gpis_ray_in *rays, const gpis_seg_out *seg, const gpis_cond_coeff *coeff, const float *e3, uint64_t *rng, float *thr3,
                         float *em3, uint32_t *segs, nee_paths_rgb_hit *hits, gpis_nee_query *q_half, gpis_nee_query *q_normal)
{
    const v3f capDir = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        nee_paths_rgb_hit *x = &hits[i];
        memset(x, 0, sizeof *x);
        if (!alive[i])
            continue;
        segs[i] += 1;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok) { alive[i] = 0; continue; }
        if (!o->exited && emissive)
            for (int c = 0; c < 3; ++c) {
                const float prod = thr3[3 * i + c] * e3[3 * i + c];
                em3[3 * i + c] = em3[3 * i + c] + prod;
            }
        for (int c = 0; c < 3; ++c)
            thr3[3 * i + c] = thr3[3 * i + c] * o->weight[c];
        if (o->exited || !(bounce + 1 < max_bounces)) { alive[i] = 0; continue; }
        const gpis_ray_in *ray = &rays[i];
        x->hit = 1;
        for (int c = 0; c < 3; ++c)
            x->thr[c] = thr3[3 * i + c];
        x->scheme = o->scheme;
        double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
        double len = sqrt(ax * ax + ay * ay + az * az);
        const v3f nn = v3((float)(ax / len), (float)(ay / len), (float)(az / len));
        const frame fr = frame_from_normal(nn);
        const v3f dir = v3(ray->dir[0], ray->dir[1], ray->dir[2]);
        const v3f wi = normalized3(to_local(&fr, v3(-dir.x, -dir.y, -dir.z)));
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        nee_paths_rgb_fresnel(sf, wi.z, x->F);
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


/* After neePDF / neeGrad: the shadow segments that are marched and their contributions, then the bounce and the next ray, which
 * follows only if its segment is marched: bounce + 1 < n_marched, n_marched = max_bounces - 1 or, on an emissive medium,
 * max_bounces.  alive[i] becomes "rays[i] is the next path segment". */
void nee_paths_rgb_shade(const gpis_scene_s *s, const gpis_surface_rgb_s *sf, size_t n, int bounce, int n_marched, uint8_t *alive, gpis_ray_in *rays,
                         const gpis_seg_out *seg, uint64_t *rng, float *thr3, uint32_t *segs, nee_paths_rgb_hit *hits,
                         gpis_ray_in *shadow_light, gpis_ray_in *shadow_phase)
{
    const float pdf_l = spherical_cap_pdf(sf->cap_cos);
    for (size_t i = 0; i < n; ++i) {
        nee_paths_rgb_hit *x = &hits[i];
        if (!x->hit)
            continue;
        const gpis_seg_out *o = &seg[i];
        const gpis_ray_in ray = rays[i];
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        const gpis_ray_in sh0 = state_copy(&ray, o);
        uint64_t g = rng[i];
        if (x->want_light) {
            const float pdf = x->pdf_half;
            float f[3];
            for (int c = 0; c < 3; ++c)
                f[c] = x->F[c] * pdf;
            const int all_zero = f[0] == 0.0f && f[1] == 0.0f && f[2] == 0.0f;
            const v3f d = v3(x->d[0], x->d[1], x->d[2]);
            float t0, t1;
            if (!all_zero && sphere_chord(p, d, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = sh0;
                sh.dir[0] = d.x; sh.dir[1] = d.y; sh.dir[2] = d.z;
                sh.far_t = t1;
                sh.u_jitter = pcg_next_1d(&g);
                sh.last_aniso[0] = x->grad_half[0]; sh.last_aniso[1] = x->grad_half[1]; sh.last_aniso[2] = x->grad_half[2];
                shadow_light[i] = sh;
                for (int c = 0; c < 3; ++c) {
                    float lightF = f[c] * (1.f * sf->cap_radiance[c]) / pdf_l;
                    if (x->scheme != GPIS_NEE)
                        lightF *= power_heuristic(pdf_l, pdf);
                    x->contrib_light[c] = lightF;
                }
                x->go_light = 1;
                segs[i] += 1;
            }
        }
        const v3f w = v3(x->w[0], x->w[1], x->w[2]);
        float t0, t1 = 0.f;
        const int chord = sphere_chord(p, w, s->bound_radius, &t0, &t1);
        if (x->want_phase) {           /* the chord exists (nee_paths_rgb_setup) */
            gpis_ray_in sh = sh0;
            sh.dir[0] = w.x; sh.dir[1] = w.y; sh.dir[2] = w.z;
            sh.far_t = t1;
            sh.u_jitter = pcg_next_1d(&g);
            shadow_phase[i] = sh;
            for (int c = 0; c < 3; ++c) {
                float phaseF = (1.f * sf->cap_radiance[c]) * x->F[c];
                if (x->scheme != GPIS_UNI)
                    phaseF *= power_heuristic(x->pdf_normal, pdf_l);
                x->contrib_phase[c] = phaseF;
            }
            x->go_phase = 1;
            segs[i] += 1;
        }
        /* the bounce */
        for (int c = 0; c < 3; ++c)
            thr3[3 * i + c] = x->thr[c] * x->F[c];
        float top = thr3[3 * i];
        for (int c = 1; c < 3; ++c)
            if (thr3[3 * i + c] > top)
                top = thr3[3 * i + c];
        int lives = !(top == 0.0f) && chord && bounce + 1 < n_marched;
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

/* After the shadow marches: em[c] = em[c] + thr[c] * L[c] for every hit; e = visible * cap_radiance is a Vec3f, and e == 0 (every
 * channel) skips the estimator (TraceBase.cpp:374, 410) */
void nee_paths_rgb_gather(const gpis_surface_rgb_s *sf, size_t n, const nee_paths_rgb_hit *hits, float *em3)
{
    for (size_t i = 0; i < n; ++i) {
        const nee_paths_rgb_hit *x = &hits[i];
        if (!x->hit)
            continue;
        float L[3] = {0.f, 0.f, 0.f};
        for (int which = 0; which < 2; ++which) {
            if (!(which ? x->go_phase : x->go_light))
                continue;
            const float v = (which ? x->vis_phase : x->vis_light) ? 1.f : 0.f;
            const float e[3] = {v * sf->cap_radiance[0], v * sf->cap_radiance[1], v * sf->cap_radiance[2]};
            if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f)
                continue;
            for (int c = 0; c < 3; ++c)
                L[c] += which ? x->contrib_phase[c] : x->contrib_light[c];
        }
        for (int c = 0; c < 3; ++c)
            em3[3 * i + c] = em3[3 * i + c] + x->thr[c] * L[c];
    }
}

/* Adds the n samples, given in the order (pixel, sample), to the image and the counts: pixel_of[i] is the sample's index
 * y*width+x; samples of one pixel are consecutive.  Per channel each pixel's emissions are summed from zero in order and the sum
 * is added to the image once, which is what a driver call does. */
void nee_paths_rgb_sum(size_t n, const uint32_t *pixel_of, const float *em3, const uint32_t *segs, float *radiance_sum3, uint32_t *seg_count)
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
            radiance_sum3[3 * pix + c] += acc[c];
        seg_count[pix] += cnt;
    }
}

size_t nee_paths_rgb_hit_size(void) { return sizeof(nee_paths_rgb_hit); }
