/* TEST INFRASTRUCTURE: the shade step and the pixel sum of scene S, for the CPU composite of the weight-space frame
 * (tests/ws_scene_ref.py).  Plain C, compiled with the restatement flags (no FMA, no contraction).
 *
 * The arithmetic and its association order are those of oracle/gpis_oracle.c (scene_s_shadow_ray, render_range), which the
 * sparse-convolution image tests pin against the device's k_scene_shade / k_scene_accumulate:
 *   light  l = light_dir * (1 / sqrtf(((0 + lx lx) + ly ly) + lz lz))                        (float)
 *   normal n = float(aniso / sqrt((ax ax + ay ay) + az az))                                   (double, rounded per component)
 *   cos    c = (n.x l.x + n.y l.y) + n.z l.z                                                  (float)
 *   a shadow segment exists when c > 0 and the ray (p, l) meets the bounding sphere
 *   pixel  acc = 0; for each sample in order: acc += (c * (visible ? 1 : 0)) * light_radiance (float)
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "gpis.h"

/* ray / sphere(|x| = R) in double: the far root as float, 0 on a miss */
static int chord_far(const float o[3], const float d[3], float R, float *t1)
{
    double ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
    double a = dx * dx + dy * dy + dz * dz;
    double b = ox * dx + oy * dy + oz * dz;
    double c = ox * ox + oy * oy + oz * oz - (double)R * (double)R;
    double disc = b * b - a * c;
    if (!(disc > 0.0))
        return 0;
    double sq = sqrt(disc);
    double tb = (-b + sq) / a;
    if (tb <= 0.0)
        return 0;
    *t1 = (float)tb;
    return 1;
}

/* For each of the n primary results: hit[i] (the segment ended on the surface), lit[i] (a shadow segment is to be marched:
 * shadow[i] is its ray) and cosl[i].  u_shadow[i] is the sample's fourth draw. */
void ws_scene_shade(const gpis_scene_s *s, size_t n, const gpis_ray_in *prim, const gpis_seg_out *seg, const float *u_shadow,
                    gpis_ray_in *shadow, float *cosl, uint8_t *hit, uint8_t *lit)
{
    float l[3];
    {
        float lx = s->light_dir[0], ly = s->light_dir[1], lz = s->light_dir[2];
        float l2 = 0.f;
        l2 += lx * lx; l2 += ly * ly; l2 += lz * lz;
        float inv = 1.0f / sqrtf(l2);
        l[0] = lx * inv; l[1] = ly * inv; l[2] = lz * inv;
    }
    for (size_t i = 0; i < n; ++i) {
        const gpis_seg_out *o = &seg[i];
        const gpis_ray_in *p = &prim[i];
        gpis_ray_in *sh = &shadow[i];
        memset(sh, 0, sizeof *sh);
        cosl[i] = 0.f; hit[i] = 0; lit[i] = 0;
        if (!o->ok || o->exited)
            continue;
        hit[i] = 1;
        double ax = o->aniso[0], ay = o->aniso[1], az = o->aniso[2];
        double len = sqrt(ax * ax + ay * ay + az * az);
        float nx = (float)(ax / len), ny = (float)(ay / len), nz = (float)(az / len);
        float c = nx * l[0];
        c += ny * l[1];
        c += nz * l[2];
        cosl[i] = c;
        float t1;
        if (!(c > 0.f) || !chord_far(o->p, l, s->bound_radius, &t1))
            continue;
        sh->pos[0] = o->p[0]; sh->pos[1] = o->p[1]; sh->pos[2] = o->p[2];
        sh->dir[0] = l[0]; sh->dir[1] = l[1]; sh->dir[2] = l[2];
        sh->near_t = 0.f; sh->far_t = t1;
        sh->pixel[0] = p->pixel[0]; sh->pixel[1] = p->pixel[1]; sh->spp = p->spp;
        sh->segment = p->segment + 1;
        sh->scene_seed = p->scene_seed;
        sh->info_t = p->info_t + o->sample_t;
        sh->u_jitter = u_shadow[i];
        sh->first_scatter = 0;
        sh->bounce = p->bounce + 1;
        sh->last_val = o->last_val;
        sh->last_gp_id = o->gp_id;
        sh->last_aniso[0] = o->aniso[0]; sh->last_aniso[1] = o->aniso[1]; sh->last_aniso[2] = o->aniso[2];
        lit[i] = 1;
    }
}

/* Adds the n samples, given in the order (pixel, sample), to the image: pixel_of[i] is the sample's index y*width+x; samples of
 * one pixel are consecutive.  Each pixel's samples are summed from zero in order and the sum is added to the image once, which
 * is what a driver call does. */
void ws_scene_sum(const gpis_scene_s *s, size_t n, const uint32_t *pixel_of, const float *cosl, const uint8_t *hit, const uint8_t *lit,
                  const uint8_t *visible, float *radiance_sum, uint32_t *hit_count)
{
    size_t i = 0;
    while (i < n) {
        const uint32_t pix = pixel_of[i];
        float acc = 0.f;
        uint32_t hits = 0;
        for (; i < n && pixel_of[i] == pix; ++i) {
            hits += hit[i];
            if (lit[i])
                acc += cosl[i] * (visible[i] ? 1.f : 0.f) * s->light_radiance;
        }
        radiance_sum[pix] += acc;
        if (hit_count) hit_count[pix] += hits;
    }
}
