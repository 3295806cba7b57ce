// gpis_scene.hpp — what the scene-S frame drivers of every medium share (gpis_hip.hip: the sparse-convolution drivers;
// tu_ws_scene.hip: the weight-space driver; gpis_fs_scene.hpp: the function-space driver): the host-precomputed camera constants, the pixel order of a call, the argument
// check and the bounding-sphere chord.  One definition, so that the drivers cannot drift apart in a single bit.
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

}   // namespace gpis
