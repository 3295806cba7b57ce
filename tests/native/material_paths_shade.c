/* TEST INFRASTRUCTURE: the per-bounce set-up, shade, bounce and gather of gpis_render_scene_s_material_paths_rgb, the RGB path
 * estimator on scene S whose material is chosen per hit by the GP id, for the CPU composite (tests/material_paths_ref.py).  Plain C
 * in float, compiled with the restatement flags (no FMA, no contraction).
 *
 * A CONDUCTOR hit runs the step of tests/native/nee_paths_rgb_shade.c, which is included here as it is (its geometry, PCG32 and
 * state copy serve the Lambert step too), one sample at a time, with the material's eta, k, albedo and the table's cap.
 * A LAMBERT hit is BRDFPhaseFunction over LambertBsdf under a non-Dirac light, restated from TraceBase.cpp:346-420 / 552 and
 * LambertBsdf.cpp:27-68 as include/gpis.h states it (steps L1-L4).  Its parity with the reference is UNPINNED above its pieces: the
 * disk sampler is pinned to tests/native/paths_rgb_shade.c's and the MIS estimator to its closed form
 * (tests/test_material_paths_cpu.py).  Order of draws at a Lambert hit: the light direction, the phase direction, the shadow
 * jitters (the light's first), the bounce direction, the next segment's jitter.
 */
#include "nee_paths_rgb_shade.c"

typedef struct {
    nee_paths_rgb_hit h;      /* LAMBERT: d = the light direction, w = the phase direction; F, pdf_*, grad_half unused */
    int32_t type;
    uint32_t material;        /* gp_id < n_materials ? gp_id : 0 */
    float wi_z, wo_z, wop_z;  /* LAMBERT: cosines of wi, the light direction and the phase direction in the hit's frame */
} mat_paths_hit;

size_t mat_paths_hit_size(void) { return sizeof(mat_paths_hit); }

static gpis_surface_rgb_s surface_of(const gpis_materials_s *mt, uint32_t k)
{
    gpis_surface_rgb_s sf;
    memset(&sf, 0, sizeof sf);
    for (int c = 0; c < 3; ++c) {
        sf.eta[c] = mt->material[k].eta[c]; sf.k[c] = mt->material[k].k[c]; sf.albedo[c] = mt->material[k].albedo[c];
        sf.cap_radiance[c] = mt->cap_radiance[c];
    }
    sf.cap_cos = mt->cap_cos;
    return sf;
}

static frame hit_frame(const gpis_seg_out *o)
{
    double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
    double len = sqrt(ax * ax + ay * ay + az * az);
    return frame_from_normal(v3((float)(ax / len), (float)(ay / len), (float)(az / len)));
}

/* LambertBsdf::sample's direction in the local frame by unit-disk rejection */
static v3f lambert_disk(uint64_t *g)
{
    float dx, dy, d2;
    do {
        dx = 2.f * pcg_next_1d(g) - 1.f;
        dy = 2.f * pcg_next_1d(g) - 1.f;
        d2 = dx * dx + dy * dy;
    } while (!(d2 < 1.f));
    const float rem = 1.0f - d2;
    return v3(dx, dy, sqrtf(rem > 0.f ? rem : 0.f));
}

/* the sampler alone, around the normal n3: the world direction; *state is advanced */
void mat_paths_lambert_direction(uint64_t *state, const float *n3, float *w3)
{
    const frame fr = frame_from_normal(v3(n3[0], n3[1], n3[2]));
    const v3f w = normalized3(to_global(&fr, lambert_disk(state)));
    w3[0] = w.x; w3[1] = w.y; w3[2] = w.z;
}

/* nee_paths_rgb_setup with the material of every hit */
void mat_paths_setup(const gpis_scene_s *s, const gpis_materials_s *mt, size_t n, int bounce, int max_bounces, int emissive, uint8_t *alive,
                     const gpis_ray_in *rays, const gpis_seg_out *seg, const gpis_cond_coeff *coeff, const float *e3, uint64_t *rng, float *thr3,
                     float *em3, uint32_t *segs, mat_paths_hit *hits, gpis_nee_query *q_half, gpis_nee_query *q_normal)
{
    const v3f capDir = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        mat_paths_hit *x = &hits[i];
        memset(x, 0, sizeof *x);
        if (!alive[i])
            continue;
        const gpis_seg_out *o = &seg[i];
        const uint32_t k = (uint32_t)o->gp_id < mt->n_materials ? (uint32_t)o->gp_id : 0u;
        x->material = k;
        x->type = mt->material[k].type;
        if (x->type == GPIS_MATERIAL_CONDUCTOR) {
            const gpis_surface_rgb_s sf = surface_of(mt, k);
            nee_paths_rgb_setup(s, &sf, 1, bounce, max_bounces, emissive, alive + i, rays + i, o, coeff + i, e3 + 3 * i, rng + i, thr3 + 3 * i, em3 + 3 * i,
                                segs + i, &x->h, q_half + i, q_normal + i);
            continue;
        }
        /* up to the material: as nee_paths_rgb_setup */
        segs[i] += 1;
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
        x->h.hit = 1;
        for (int c = 0; c < 3; ++c)
            x->h.thr[c] = thr3[3 * i + c];
        x->h.scheme = o->scheme;
        const frame fr = hit_frame(o);
        const v3f wi = normalized3(to_local(&fr, v3(-ray->dir[0], -ray->dir[1], -ray->dir[2])));
        x->wi_z = wi.z;
        uint64_t g = rng[i];
        /* L1: the cap direction, always */
        float z = pcg_next_1d(&g) * (1.0f - mt->cap_cos) + mt->cap_cos;
        float dx, dy, d2;
        do {
            dx = 2.f * pcg_next_1d(&g) - 1.f;
            dy = 2.f * pcg_next_1d(&g) - 1.f;
            d2 = dx * dx + dy * dy;
        } while (!(d2 < 1.f) || !(d2 > 1e-12f));
        float rr = 1.0f - z * z;
        float rad = sqrtf(rr > 0.f ? rr : 0.f) / sqrtf(d2);
        frame cf = frame_from_normal(capDir);
        v3f d = to_global(&cf, v3(dx * rad, dy * rad, z));
        v3f wo = normalized3(to_local(&fr, d));
        x->h.d[0] = d.x; x->h.d[1] = d.y; x->h.d[2] = d.z;
        x->wo_z = wo.z;
        /* L2: the phase direction */
        if (wi.z > 0.0f) {
            const v3f wop = lambert_disk(&g);
            const v3f w = normalized3(to_global(&fr, wop));
            x->h.w[0] = w.x; x->h.w[1] = w.y; x->h.w[2] = w.z;
            x->wop_z = wop.z;
        }
        rng[i] = g;
    }
}

/* nee_paths_rgb_shade with the material of every hit */
void mat_paths_shade(const gpis_scene_s *s, const gpis_materials_s *mt, size_t n, int bounce, int n_marched, uint8_t *alive, gpis_ray_in *rays,
                     const gpis_seg_out *seg, uint64_t *rng, float *thr3, uint32_t *segs, mat_paths_hit *hits, gpis_ray_in *shadow_light,
                     gpis_ray_in *shadow_phase)
{
    const float pdf_l = spherical_cap_pdf(mt->cap_cos);
    const v3f capDir = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        mat_paths_hit *x = &hits[i];
        if (!x->h.hit)
            continue;
        if (x->type == GPIS_MATERIAL_CONDUCTOR) {
            const gpis_surface_rgb_s sf = surface_of(mt, x->material);
            nee_paths_rgb_shade(s, &sf, 1, bounce, n_marched, alive + i, rays + i, seg + i, rng + i, thr3 + 3 * i, segs + i, &x->h, shadow_light + i,
                                shadow_phase + i);
            continue;
        }
        const float *albedo = mt->material[x->material].albedo;
        const gpis_seg_out *o = &seg[i];
        const gpis_ray_in ray = rays[i];
        const v3f p = v3(o->p[0], o->p[1], o->p[2]);
        const gpis_ray_in sh0 = state_copy(&ray, o);      /* last_aniso: the hit's own */
        uint64_t g = rng[i];
        float t0, t1;
        {   /* L1 */
            float f[3];
            for (int c = 0; c < 3; ++c)
                f[c] = x->wi_z > 0.0f && x->wo_z > 0.0f ? albedo[c] * (1.0f / 3.1415926536f) * x->wo_z : 0.0f;
            const int all_zero = f[0] == 0.0f && f[1] == 0.0f && f[2] == 0.0f;
            const v3f d = v3(x->h.d[0], x->h.d[1], x->h.d[2]);
            if (!all_zero && sphere_chord(p, d, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = sh0;
                sh.dir[0] = d.x; sh.dir[1] = d.y; sh.dir[2] = d.z;
                sh.far_t = t1;
                sh.u_jitter = pcg_next_1d(&g);
                shadow_light[i] = sh;
                for (int c = 0; c < 3; ++c) {
                    float lightF = f[c] * (1.f * mt->cap_radiance[c]) / pdf_l;
                    lightF *= power_heuristic(pdf_l, x->wo_z * (1.0f / 3.1415926536f));
                    x->h.contrib_light[c] = lightF;
                }
                x->h.go_light = 1;
                segs[i] += 1;
            }
        }
        if (x->wi_z > 0.0f) {   /* L2 */
            const v3f w = v3(x->h.w[0], x->h.w[1], x->h.w[2]);
            if (!(dot3(w, capDir) < mt->cap_cos) && sphere_chord(p, w, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = sh0;
                sh.dir[0] = w.x; sh.dir[1] = w.y; sh.dir[2] = w.z;
                sh.far_t = t1;
                sh.u_jitter = pcg_next_1d(&g);
                shadow_phase[i] = sh;
                for (int c = 0; c < 3; ++c) {
                    float phaseF = (1.f * mt->cap_radiance[c]) * albedo[c];
                    phaseF *= power_heuristic(x->wop_z * (1.0f / 3.1415926536f), pdf_l);
                    x->h.contrib_phase[c] = phaseF;
                }
                x->h.go_phase = 1;
                segs[i] += 1;
            }
        }
        /* L4: the bounce */
        int lives = x->wi_z > 0.0f;
        if (lives) {
            const frame fr = hit_frame(o);
            const v3f w = normalized3(to_global(&fr, lambert_disk(&g)));
            for (int c = 0; c < 3; ++c)
                thr3[3 * i + c] = x->h.thr[c] * albedo[c];
            float top = thr3[3 * i];
            for (int c = 1; c < 3; ++c)
                if (thr3[3 * i + c] > top)
                    top = thr3[3 * i + c];
            lives = !(top == 0.0f) && sphere_chord(p, w, s->bound_radius, &t0, &t1) && bounce + 1 < n_marched;
            if (lives) {
                gpis_ray_in next = sh0;
                next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
                next.far_t = t1;
                next.u_jitter = pcg_next_1d(&g);
                rays[i] = next;
            }
        }
        rng[i] = g;
        alive[i] = lives ? 1 : 0;
    }
}

/* nee_paths_rgb_gather: L of either material is the visible ones of contrib_light and contrib_phase under the table's light */
void mat_paths_gather(const gpis_materials_s *mt, size_t n, const mat_paths_hit *hits, float *em3)
{
    const gpis_surface_rgb_s sf = surface_of(mt, 0);
    for (size_t i = 0; i < n; ++i)
        nee_paths_rgb_gather(&sf, 1, &hits[i].h, em3 + 3 * i);
}
