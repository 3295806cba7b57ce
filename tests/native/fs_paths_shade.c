/* TEST INFRASTRUCTURE: the per-bounce shade step of the multi-bounce estimator on scene S for the CPU composite of the
 * function-space path frame (tests/fs_paths_ref.py).  Plain C, compiled with the restatement flags (no FMA, no contraction).
 *
 * The arithmetic and its association order are those of ws_paths_shade (ws_paths_shade.c, included here for its static helpers
 * and for ws_paths_nee_add / ws_paths_sum), which tests/test_ws_paths_cpu.py pins to the oracle of gpis_render_scene_s_paths;
 * tests/test_fs_paths_cpu.py pins this file to ws_paths_shade bit for bit.  What differs is the sampler: the function-space
 * medium draws from the path's own stream, so the shade step is cut in two around the shadow segment and draws no jitter —
 *   path segment b                                   (the medium draws)
 *   fs_paths_nee      decides NEE, builds the shadow ray, computes the contribution; draws nothing
 *   shadow segment    on a copy of the path's state  (the medium draws, from where path segment b stopped)
 *   fs_paths_bounce   draws the disk pairs from where the shadow segment stopped, throughput, the next ray
 *   path segment b+1                                 (the medium draws, from where the bounce stopped)
 */
#include "ws_paths_shade.c"

/* normal frame, wi, hit point and the template of the next ray: the lines of ws_paths_shade between `exited` and the NEE block */
static void fs_paths_hit(const gpis_ray_in *ray, const gpis_seg_out *o, int bounce, frame *fr, v3f *wi, v3f *p, gpis_ray_in *next)
{
    double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
    double len = sqrt(ax * ax + ay * ay + az * az);
    const v3f nn = v3((float)(ax / len), (float)(ay / len), (float)(az / len));
    *fr = frame_from_normal(nn);
    *wi = normalized3(to_local(fr, v3(-ray->dir[0], -ray->dir[1], -ray->dir[2])));
    *p = v3(o->p[0], o->p[1], o->p[2]);
    memset(next, 0, sizeof *next);
    next->pos[0] = p->x; next->pos[1] = p->y; next->pos[2] = p->z;
    next->near_t = 0.f;
    next->pixel[0] = ray->pixel[0]; next->pixel[1] = ray->pixel[1]; next->spp = ray->spp;
    next->scene_seed = ray->scene_seed;
    next->info_t = ray->info_t + o->sample_t;
    next->first_scatter = 0;
    next->bounce = ray->bounce + 1;
    next->last_val = o->last_val;
    next->last_gp_id = o->gp_id;
    next->last_aniso[0] = o->aniso[0]; next->last_aniso[1] = o->aniso[1]; next->last_aniso[2] = o->aniso[2];
    next->segment = (uint32_t)bounce + 1;
}

/* After the path segments of one bounce level.  In: alive[i], rays[i] (the segment of this bounce), seg[i] (its sampleDistance
 * result), throughput[i].  Out, for the paths that were alive: throughput[i] *= weight[0]; end[i] / alive[i] = 0 for !ok and
 * exited; nee[i] / shadow[i] / contrib[i] when a shadow segment is to be marched (bounce < max_bounces - 1 only). */
void fs_paths_nee(const gpis_scene_s *s, size_t n, int bounce, int max_bounces, float albedo, const gpis_ray_in *rays, const gpis_seg_out *seg,
                  float *throughput, uint8_t *alive, gpis_ray_in *shadow, float *contrib, uint8_t *nee, uint8_t *end)
{
    const v3f l = light_of(s);
    for (size_t i = 0; i < n; ++i) {
        nee[i] = 0; end[i] = WS_PATHS_LIVES; contrib[i] = 0.f;
        if (!alive[i])
            continue;
        const gpis_seg_out *o = &seg[i];
        if (!o->ok) { alive[i] = 0; end[i] = WS_PATHS_NOT_OK; continue; }
        float thr = throughput[i] * o->weight[0];
        throughput[i] = thr;
        if (o->exited) { alive[i] = 0; end[i] = WS_PATHS_EXITED; continue; }
        if (!(bounce < max_bounces - 1))
            continue;
        frame fr;
        v3f wi, p;
        gpis_ray_in next;
        fs_paths_hit(&rays[i], o, bounce, &fr, &wi, &p, &next);
        const v3f wo = normalized3(to_local(&fr, l));
        if (wi.z > 0.0f && wo.z > 0.0f) {
            const float f = albedo * (1.0f / 3.1415926536f) * wo.z;
            float t0, t1;
            if (sphere_chord(p, l, s->bound_radius, &t0, &t1)) {
                gpis_ray_in sh = next;
                sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                sh.far_t = t1;
                shadow[i] = sh;
                contrib[i] = thr * (f * s->light_radiance);
                nee[i] = 1;
            }
        }
    }
}

/* After the shadow segments of one bounce level.  In: alive[i] (the path hit at this bounce), rays[i], seg[i], rng[i] (the
 * stream where the medium left it), throughput[i] (as fs_paths_nee left it).  Out: end[i]; when the path lives on rays[i] (the
 * next segment); rng[i] / throughput[i] / alive[i] advanced. */
void fs_paths_bounce(const gpis_scene_s *s, size_t n, int bounce, float albedo, gpis_ray_in *rays, const gpis_seg_out *seg, uint64_t *rng,
                     float *throughput, uint8_t *alive, uint8_t *end)
{
    for (size_t i = 0; i < n; ++i) {
        if (!alive[i])
            continue;
        frame fr;
        v3f wi, p;
        gpis_ray_in next;
        fs_paths_hit(&rays[i], &seg[i], bounce, &fr, &wi, &p, &next);
        float thr = throughput[i];
        uint64_t g = rng[i];
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
                rays[i] = next;
            }
        }
        alive[i] = lives ? 1 : 0;
        throughput[i] = thr;
        rng[i] = g;
    }
}
