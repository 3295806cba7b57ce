// gpis_scene.hpp — what the scene-S drivers of every medium share.  One definition, so that the drivers cannot drift apart in a
// single bit.
//   host: the host-precomputed camera constants (SceneConst, make_scene_const), the pixel order of a call (scene_pixel,
//       scene_rows) and the argument check (scene_args_ok) — tu_scene.hip, tu_ws_scene.hip, tu_ws_paths.hip;
//   camera step: scene_sample (pixel, spp index, seeded stream) — k_scene_primary, k_scene_primary_c, k_paths_begin,
//       k_paths_rgb_begin, k_ws_scene, k_ws_paths, k_fs_scene, k_fs_paths — and scene_camera_ray (direction, bounding-sphere chord,
//       the first gpis_ray_in) — the same but k_scene_primary_c and k_fs_paths.  The sample layout is scene_sample's second
//       argument: here the first pixel of a chunk with spp_count samples per pixel; gpis_adaptive.hpp overloads it for the records
//       of an adaptive pass, and the three staged camera kernels of tu_scene.hip are templates on that argument's type;
//   hit_normal — the seven shading kernels (k_scene_shade, k_paths_shade, k_paths_rgb_shade, k_ws_scene, k_ws_paths, k_fs_scene,
//       k_fs_paths) and the set-up of the conductor NEE drivers (nee_setup_sample in tu_scene.hip);
//   the compact records of the Lambert frame (SceneRay, SceneHit: 32 B each, what gpis_render_scene_s passes between its kernels on
//       the resident guided march), scene_camera_dir and scene_lambert_shade, which k_scene_primary / k_scene_shade share with
//       their compact forms k_scene_primary_c / k_scene_shade_c;
//   scene_next_ray, the ray that continues a path from a hit — the Lambert shadow rays of k_scene_shade, k_ws_scene and
//       k_fs_scene, the shadow rays of the conductor NEE drivers (nee_shade_sample) and the next path segment of
//       k_nee_paths_shade.
// The device helpers draw nothing, hold no barrier and branch only on their arguments: called with wave-uniform arguments they
// return wave-uniform results (gpis_fs_scene.hpp and gpis_fs_paths.hpp rest on this).
// Not here: the shade step of the path kernels (k_paths_shade, k_paths_rgb_shade, k_ws_paths, k_fs_paths: Duff frame, wi / wo, next-event
// estimation, disk rejection, the `next` template) and the camera ray of k_fs_paths, which those kernels state in full.  As
// functions around the inlined marches they changed the code of the whole kernel and made k_ws_paths and k_fs_paths slower.
#pragma once
#include <cmath>

#include "gpis.h"
#include "gpis_device.hpp"

#pragma clang fp contract(off)

namespace gpis {

struct SceneConst {   // host-precomputed scene-S constants (host libm: tanf, normalisation)
    gpis_scene_s s;
    float plane_dist, ratio, psx;
    float light[3];
};

// Pixel `local` of a driver call -> index y*width + x in the image.  A call renders the image rows
// [y_begin, y_begin + y_count); with shard_count > 1 only the tile rows t (tile_size pixels high, counted
// from y_begin) with t % shard_count == shard_index — the interleaved tile-row split of the multi-GPU
// driver, kept in ONE batch per rank so that every stage stays one launch.
__host__ __device__ inline size_t scene_pixel(const gpis_scene_s &s, size_t local)
{
    if (s.shard_count <= 1u)
        return (size_t)s.y_begin * s.width + local;
    const size_t ly = local / s.width, x = local % s.width;
    const size_t lt = ly / s.tile_size, r = ly % s.tile_size;
    return ((size_t)s.y_begin + (lt * s.shard_count + s.shard_index) * s.tile_size + r) * s.width + x;
}
// rows this call renders
inline size_t scene_rows(const gpis_scene_s &s)
{
    if (s.shard_count <= 1u)
        return s.y_count;
    size_t rows = 0;
    for (size_t t = s.shard_index, y0 = (size_t)s.shard_index * s.tile_size; y0 < s.y_count; t += s.shard_count, y0 = t * s.tile_size)
        rows += (s.y_count - y0 < s.tile_size) ? s.y_count - y0 : s.tile_size;
    return rows;
}
inline bool scene_args_ok(const gpis_scene_s *s)
{
    return s->width > 0 && s->height > 0 && s->spp_count > 0 && s->y_begin + s->y_count <= s->height &&
           (s->shard_count <= 1u || (s->shard_index < s->shard_count && s->tile_size > 0));
}

inline SceneConst make_scene_const(const gpis_scene_s *s)
{
    SceneConst sc;
    sc.s = *s;
    const float pi_f = 3.1415926536f;
    float fov_rad = s->cam_fov_deg * (pi_f / 180.0f);
    sc.plane_dist = 1.0f / tanf(fov_rad * 0.5f);
    sc.ratio = (float)s->height / (float)s->width;
    sc.psx = 1.0f / (float)s->width;
    {
        float lx = s->light_dir[0], ly = s->light_dir[1], lz = s->light_dir[2];
        float l2 = 0.f; l2 += lx * lx; l2 += ly * ly; l2 += lz * lz;
        float inv = 1.0f / sqrtf(l2);
        sc.light[0] = lx * inv; sc.light[1] = ly * inv; sc.light[2] = lz * inv;
    }
    return sc;
}

// ---- the compact records of the Lambert frame driver (gpis_render_scene_s on the resident guided march, GPIS_OPT_SCENE_COMPACT).
// Of the 128 B of a gpis_ray_in the guided march reads 11 words, and of those the origin of a primary ray (the camera) and the
// direction of a shadow ray (the light) are the same for every sample of a launch, as are first_scatter and bounce: they travel as
// kernel arguments.  One 32-byte record per lane remains, 16-byte aligned so that it moves as two dwordx4.
struct alignas(16) SceneRay {
    float v[3];          // primary ray: direction; shadow ray: origin (the hit point)
    float near_t, far_t;
    float u_jitter;
    float u_aux;         // primary ray: the jitter of the sample's shadow ray; shadow ray: unused (0)
    uint32_t flags;      // bit 0 — primary ray: it crosses the bound; shadow ray: the sample has one
};
// What k_scene_shade_c reads of a segment result.  g is the `aniso` of the full record: that is to_d() of the float gradient, so
// three floats hold it exactly.
struct alignas(16) SceneHit {
    float p[3];
    float g[3];
    uint32_t flags;      // bit 0: ok, bit 1: exited
    uint32_t spare;
};
static_assert(sizeof(SceneRay) == 32 && alignof(SceneRay) == 16, "SceneRay: one 32-byte record per sample");
static_assert(sizeof(SceneHit) == 32 && alignof(SceneHit) == 16, "SceneHit: one 32-byte record per sample");
constexpr uint32_t kSceneRayLive = 1u, kSceneHitOk = 1u, kSceneHitExited = 2u;

// ray / sphere(|x| = R) intersection in double; false on a miss
__device__ __forceinline__ bool sphere_chord(V3 o, V3 d, float R, float &t0, float &t1)
{
    double ox = o.x, oy = o.y, oz = o.z, dx = d.x, dy = d.y, dz = d.z;
    double a = dx * dx + dy * dy + dz * dz;
    double b = ox * dx + oy * dy + oz * dz;
    double c = ox * ox + oy * oy + oz * oz - (double)R * (double)R;
    double disc = b * b - a * c;
    if (!(disc > 0.0))
        return false;
    double sq = sqrt(disc);
    double ta = (-b - sq) / a, tb = (-b + sq) / a;
    if (tb <= 0.0)
        return false;
    if (ta < 0.0) ta = 0.0;
    t0 = (float)ta; t1 = (float)tb;
    return true;
}

// ---- the camera step.  Sample i of a driver call -> its pixel, its spp index and the sample's PCG32 stream, freshly seeded.
template <typename Index>
GPIS_DEV Pcg32 scene_sample(const SceneConst &sc, size_t first_pixel, Index i, uint32_t &x, uint32_t &y, uint32_t &spp)
{
    const gpis_scene_s &s = sc.s;
    const size_t pix = scene_pixel(s, first_pixel + i / s.spp_count);
    x = (uint32_t)(pix % s.width); y = (uint32_t)(pix / s.width);
    spp = s.spp_begin + (uint32_t)(i % s.spp_count);
    Pcg32 g;
    g.set_state((uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s.scene_seed) + 1u));
    return g;
}
// direction of the camera ray through pixel (x, y) jittered by (jx, jy)
GPIS_DEV V3 scene_camera_dir(const SceneConst &sc, uint32_t x, uint32_t y, float jx, float jy)
{
    const V3 local = normalized(v3(-1.0f + ((float)x + jx) * 2.0f * sc.psx, sc.ratio - ((float)y + jy) * 2.0f * sc.psx, sc.plane_dist));
    return v3(local.x, local.y, -local.z);
}
// The camera ray through pixel (x, y) jittered by (jx, jy), clipped to the bounding sphere: every field of the path's first
// gpis_ray_in but u_jitter (the caller's own draw).  false: the ray misses the bound (near_t = far_t = 0).
GPIS_DEV bool scene_camera_ray(const SceneConst &sc, uint32_t x, uint32_t y, uint32_t spp, float jx, float jy, gpis_ray_in &ray)
{
    const gpis_scene_s &s = sc.s;
    const V3 d = scene_camera_dir(sc, x, y, jx, jy);
    const V3 o = v3(s.cam_pos[0], s.cam_pos[1], s.cam_pos[2]);
    memset(&ray, 0, sizeof ray);
    ray.pos[0] = o.x; ray.pos[1] = o.y; ray.pos[2] = o.z;
    ray.dir[0] = d.x; ray.dir[1] = d.y; ray.dir[2] = d.z;
    ray.pixel[0] = x; ray.pixel[1] = y; ray.spp = spp; ray.segment = 0;
    ray.scene_seed = s.scene_seed; ray.info_t = 0.f;
    ray.first_scatter = 1;
    float t0 = 0.f, t1 = 0.f;
    const bool hit = sphere_chord(o, d, s.bound_radius, t0, t1);
    ray.near_t = t0; ray.far_t = t1;
    return hit;
}

// the sampled gradient at a hit, normalised in double and rounded per component
GPIS_DEV V3 hit_normal(double ax, double ay, double az)
{
    const double len = sqrt(ax * ax + ay * ay + az * az);
    return v3((float)(ax / len), (float)(ay / len), (float)(az / len));
}
GPIS_DEV V3 hit_normal(const gpis_seg_out &o) { return hit_normal(o.aniso[0], o.aniso[1], o.aniso[2]); }
GPIS_DEV V3 hit_normal(const SceneHit &o) { return hit_normal((double)o.g[0], (double)o.g[1], (double)o.g[2]); }

// The Lambert shade step at a hit at p with normal n: c = cos to the light; true where the sample gets a shadow ray (lit, and the
// ray from p towards the light crosses the bound), which then ends at far_t.
GPIS_DEV bool scene_lambert_shade(const SceneConst &sc, V3 n, V3 p, float &c, float &far_t)
{
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    c = dot(n, l);
    float t0;
    return c > 0.f && sphere_chord(p, l, sc.s.bound_radius, t0, far_t);
}

// The shadow ray that continues the path of `ray` from the hit `o`: everything but dir, far_t and u_jitter, which the caller
// fills.
GPIS_DEV gpis_ray_in scene_next_ray(const gpis_ray_in &ray, const gpis_seg_out &o)
{
    gpis_ray_in next;
    memset(&next, 0, sizeof next);
    next.pos[0] = o.p[0]; next.pos[1] = o.p[1]; next.pos[2] = o.p[2];
    next.near_t = 0.f;
    next.pixel[0] = ray.pixel[0]; next.pixel[1] = ray.pixel[1]; next.spp = ray.spp;
    next.segment = ray.segment + 1;
    next.scene_seed = ray.scene_seed;
    next.info_t = ray.info_t + o.sample_t;
    next.first_scatter = 0;
    next.bounce = ray.bounce + 1;
    next.last_val = o.last_val;
    next.last_gp_id = o.gp_id;
    next.last_aniso[0] = o.aniso[0]; next.last_aniso[1] = o.aniso[1]; next.last_aniso[2] = o.aniso[2];
    return next;
}

}   // namespace gpis
