// tu_scene.hip — the staged scene-S frame drivers of the sparse-convolution medium and the frame loops of the function-space one
// (gpis_host.hpp: the handle and the marches they call; gpis_hip.hip defines those).  A staged driver runs a chunk of samples
// through small one-thread-per-sample kernels — defined here, in gpis_paths_rgb.hpp and in gpis_adaptive.hpp, and launched
// directly — between the medium's march launches (gpis_launch.hpp):
//   the Lambert frame               gpis_render_scene_s, gpis_render_scene_s_adaptive, gpis_reserve_scene_workspace
//   the Lambert multi-bounce paths  gpis_render_scene_s_paths, gpis_render_scene_s_paths_adaptive, gpis_render_scene_s_paths_rgb,
//                                   gpis_render_scene_s_paths_rgb_adaptive
//   the conductor NEE / MIS frames  gpis_render_scene_s_nee, gpis_render_scene_s_nee_paths, gpis_render_scene_s_nee_paths_adaptive,
//                                   gpis_render_scene_s_nee_paths_rgb, gpis_render_scene_s_nee_paths_rgb_adaptive (gpis_cond_rgb.hpp)
//   materials chosen by GP id       gpis_render_scene_s_material_paths_rgb, gpis_render_scene_s_material_paths_rgb_adaptive
//                                   (gpis_material_rgb.hpp)
//   the function-space frames       gpis_fs_render_scene_s, gpis_fs_render_scene_s_paths (fused kernels: tu_fs_scene.hip, tu_fs_paths.hip)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "gpis.h"
#include "gpis_host.hpp"
#include "gpis_launch.hpp"
#include "gpis_scene.hpp"       // SceneConst, scene_sample, scene_camera_ray, hit_normal, the compact records
#include "gpis_adaptive.hpp"    // the variable-count sample layout: scene_sample of an AdaptiveChunk, the tile statistics' arithmetic, the clamps
#include "gpis_frame_sum.hpp"   // the per-pixel sums and the tile statistics behind a chunk, on the accessors below
#include "gpis_adaptive_host.hpp"   // adaptive_passes: the pass loop of the adaptive drivers
#include "gpis_paths_rgb.hpp"   // PathsRgbArrays and the kernels of the RGB path drivers

#pragma clang fp contract(off)

using namespace gpis;
using gpis::launch::grid_of;

// ======================================================================================
// scene-S tile → ray-batch driver.  Sample index within a chunk:
// ((y*W + x) * spp_count + k): the 64 lanes of a wave carry consecutive spp of one pixel.
// The camera steps are templates on the sample layout `where` (scene_sample): size_t, the first pixel of a chunk with spp_count
// samples per pixel, or AdaptiveChunk, the records of an adaptive pass (gpis_adaptive.hpp).
// ======================================================================================
template <typename Where>
__global__ void __launch_bounds__(256) k_scene_primary(SceneConst sc, Where where, size_t n_samples,
                                                       gpis_ray_in *__restrict__ rays, float *__restrict__ u_shadow, uint8_t *__restrict__ valid)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample(sc, where, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i()), u1 = normalized_uint(g.next_i());
    gpis_ray_in r;
    bool hit = scene_camera_ray(sc, x, y, spp, jx, jy, r);
    r.u_jitter = u0;
    rays[i] = r;
    u_shadow[i] = u1;
    valid[i] = hit ? 1 : 0;
}

// the same camera step into the compact record (gpis_scene.hpp): the direction, the chord, both jitters and the "inside the bound" flag
template <typename Where>
__global__ void __launch_bounds__(256) k_scene_primary_c(SceneConst sc, Where where, size_t n_samples, SceneRay *__restrict__ rays)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample(sc, where, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i()), u1 = normalized_uint(g.next_i());
    const V3 d = scene_camera_dir(sc, x, y, jx, jy);
    float t0 = 0.f, t1 = 0.f;
    const bool hit = sphere_chord(v3(sc.s.cam_pos[0], sc.s.cam_pos[1], sc.s.cam_pos[2]), d, sc.s.bound_radius, t0, t1);
    float4 *q = reinterpret_cast<float4 *>(rays + i);
    q[0] = make_float4(d.x, d.y, d.z, t0);
    q[1] = make_float4(t1, u0, u1, __uint_as_float(hit ? kSceneRayLive : 0u));
}

// `shadow` may be `prim` itself (the Lambert driver writes each shadow ray over the primary ray it came from: the same thread has
// read that record by then, and nothing reads the primary rays afterwards) — hence no __restrict__ on the two.
__global__ void __launch_bounds__(256) k_scene_shade(SceneConst sc, size_t n_samples, const gpis_ray_in *prim,
                                                     const gpis_seg_out *__restrict__ seg, const float *__restrict__ u_shadow,
                                                     const uint8_t *__restrict__ valid, gpis_ray_in *shadow,
                                                     float *__restrict__ cosl, uint8_t *__restrict__ valid2, uint8_t *__restrict__ hit)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t v2 = 0, h = 0;
    float c = 0.f;
    if (valid[i]) {
        gpis_seg_out o = seg[i];
        if (o.ok && !o.exited) {
            h = 1;
            float t1;
            if (scene_lambert_shade(sc, hit_normal(o), v3(o.p[0], o.p[1], o.p[2]), c, t1)) {
                gpis_ray_in p = prim[i];
                gpis_ray_in sh = scene_next_ray(p, o);
                sh.dir[0] = sc.light[0]; sh.dir[1] = sc.light[1]; sh.dir[2] = sc.light[2];
                sh.far_t = t1;
                sh.u_jitter = u_shadow[i];
                shadow[i] = sh;
                v2 = 1;
            }
        }
    }
    cosl[i] = c;
    valid2[i] = v2;
    hit[i] = h;
}

// The shade step on the compact records.  Every sample's ray record is rewritten in place — the shadow ray (origin = the hit point,
// near_t = 0) or an empty record — because its flag is the mask of the shadow march; valid2 repeats the flag as the byte
// k_scene_accumulate reads four at a time.
__global__ void __launch_bounds__(256) k_scene_shade_c(SceneConst sc, size_t n_samples, SceneRay *rays, const SceneHit *__restrict__ seg,
                                                       float *__restrict__ cosl, uint8_t *__restrict__ valid2, uint8_t *__restrict__ hit)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t h = 0;
    float c = 0.f;
    float4 *q = reinterpret_cast<float4 *>(rays + i);
    const float4 r1 = q[1];                      // far_t, u_jitter, u_aux, flags of the primary ray
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (__float_as_uint(r1.w) & kSceneRayLive) {
        const float4 a = reinterpret_cast<const float4 *>(seg + i)[0], b = reinterpret_cast<const float4 *>(seg + i)[1];
        SceneHit o;
        o.p[0] = a.x; o.p[1] = a.y; o.p[2] = a.z; o.g[0] = a.w; o.g[1] = b.x; o.g[2] = b.y; o.flags = __float_as_uint(b.z);
        if ((o.flags & kSceneHitOk) && !(o.flags & kSceneHitExited)) {
            h = 1;
            float t1;
            if (scene_lambert_shade(sc, hit_normal(o), v3(o.p[0], o.p[1], o.p[2]), c, t1)) {
                s0 = make_float4(o.p[0], o.p[1], o.p[2], 0.f);
                s1 = make_float4(t1, r1.z, 0.f, __uint_as_float(kSceneRayLive));
            }
        }
    }
    q[0] = s0; q[1] = s1;
    cosl[i] = c;
    valid2[i] = (__float_as_uint(s1.w) & kSceneRayLive) ? 1 : 0;
    hit[i] = h;
}

// one lane per pixel: sequential sum over its spp, in sample order (matches the CPU estimator)
__global__ void __launch_bounds__(256) k_scene_accumulate(SceneConst sc, size_t first_pixel, size_t n_pixels, const float *__restrict__ cosl,
                                                          const uint8_t *__restrict__ valid2, const uint8_t *__restrict__ vis,
                                                          const uint8_t *__restrict__ hit, float *__restrict__ radiance_sum,
                                                          uint32_t *__restrict__ hit_count)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pixels) return;
    const uint32_t spp = sc.s.spp_count;
    float acc = 0.f;
    uint32_t hits = 0;
    if ((spp & 3u) == 0u) {
        // four samples per load (the arrays start 256-byte aligned and a pixel's run is a multiple of 4): the same sum in the same
        // order with a quarter of the load instructions (a thread walks its own 64-byte lines; 4.7 -> 2 ms per C1 frame)
        for (uint32_t k = 0; k < spp; k += 4) {
            const size_t i = j * spp + k;
            const uint32_t h4 = *reinterpret_cast<const uint32_t *>(hit + i), v4 = *reinterpret_cast<const uint32_t *>(valid2 + i),
                           s4 = *reinterpret_cast<const uint32_t *>(vis + i);
            const float4 c4 = *reinterpret_cast<const float4 *>(cosl + i);
            const float c[4] = {c4.x, c4.y, c4.z, c4.w};
            for (int u = 0; u < 4; ++u) {
                hits += (h4 >> (8 * u)) & 0xFFu;
                if ((v4 >> (8 * u)) & 0xFFu)
                    acc += c[u] * (((s4 >> (8 * u)) & 0xFFu) ? 1.f : 0.f) * sc.s.light_radiance;
            }
        }
    } else {
        for (uint32_t k = 0; k < spp; ++k) {
            size_t i = j * spp + k;
            hits += hit[i];
            if (valid2[i])
                acc += cosl[i] * (vis[i] ? 1.f : 0.f) * sc.s.light_radiance;
        }
    }
    const size_t pix = scene_pixel(sc.s, first_pixel + j);
    radiance_sum[pix] += acc;
    if (hit_count) hit_count[pix] += hits;
}

// What the shade step and the shadow march leave per sample of a chunk of the Lambert frame (lambert_chunk): the staged arrays, and
// what a sample of them is worth under the adaptive schedule at the scene's light radiance — an accessor of gpis_frame_sum.hpp.
// value: what k_scene_accumulate adds, after renderTile's clamp; count: whether the primary segment hit.  The kernels take the
// arrays and build the accessor themselves, so their parameters stay the four pointers.  (No raw: k_scene_accumulate, the one
// uniform sum of these arrays, stays its own kernel, scalar tail included.  The kernels of the adaptive schedule are templates in
// namespace gpis, as the headers' kernels.)
namespace gpis {
struct AdaptiveLambert {
    const float *cosl;
    const uint8_t *valid2, *vis, *hit;
};
struct LambertValues {
    AdaptiveLambert a;
    float light_radiance;
    GPIS_DEV float value(size_t i) const { return a.valid2[i] ? adaptive_clamp(a.cosl[i] * (a.vis[i] ? 1.f : 0.f) * light_radiance) : 0.f; }
    GPIS_DEV uint32_t count(size_t i) const { return a.hit[i]; }
};

// gpis_render_scene_s_adaptive behind a chunk of records: the per-pixel sum of the variable-count layout and the tile statistics
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_adaptive_accumulate(SceneConst sc, AdaptiveChunk ch, AdaptiveLambert a, float *__restrict__ radiance_sum,
                                                                            uint32_t *__restrict__ sample_count, uint32_t *__restrict__ hit_count)
{
    adaptive_values_sum(sc, ch, LambertValues{a, sc.s.light_radiance}, radiance_sum, sample_count, hit_count);
}
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_adaptive_stats(SceneConst sc, AdaptiveChunk ch, AdaptiveLambert a, gpis_adaptive_record *__restrict__ records)
{
    adaptive_values_stats(ch, LambertValues{a, sc.s.light_radiance}, records);
}
}   // namespace gpis

// --------------------------------------------------------------------------------------
// multi-bounce wavefront driver (gpis_render_scene_s_paths): PathTracer.cpp:62-75,
// TraceBase.cpp:346-386 and 539-563 with a Lambertian micro-surface (BRDFPhaseFunction.cpp:27-96,
// LambertBsdf.cpp:27-47) and a directional (Dirac) light.  Path state lives in SoA arrays; the
// medium kernels are the same batch entries a host integrator would call.
// --------------------------------------------------------------------------------------
struct PathArrays {
    gpis_ray_in *rays;       // current segment of every path (rewritten in place at each bounce)
    gpis_seg_out *seg;
    gpis_ray_in *shadow;
    uint64_t *rng;           // PCG32 state of the sample's stream
    float *throughput, *emission, *contrib;
    uint8_t *alive, *nee, *vis;
};

// The camera step: the path state of slot i.  `where` is the sample layout scene_sample takes: size_t, the first pixel of a chunk
// with spp_count samples per pixel (k_paths_begin), or AdaptiveChunk (k_paths_adaptive_begin).
template <typename Where>
__device__ __forceinline__ void paths_begin_sample(const SceneConst &sc, const Where &where, size_t i, const PathArrays &a)
{
    uint32_t x, y, spp;
    Pcg32 g = scene_sample(sc, where, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i());
    gpis_ray_in r;
    bool hit = scene_camera_ray(sc, x, y, spp, jx, jy, r);
    r.u_jitter = u0;
    a.rays[i] = r;
    a.rng[i] = g.state;
    a.throughput[i] = 1.f;
    a.emission[i] = 0.f;
    a.alive[i] = hit ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_paths_begin(SceneConst sc, size_t first_pixel, size_t n_samples, PathArrays a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    paths_begin_sample(sc, first_pixel, i, a);
}
// the same step for the records of an adaptive pass (the mono path drivers under the adaptive schedule)
__global__ void __launch_bounds__(256) k_paths_adaptive_begin(SceneConst sc, AdaptiveChunk ch, size_t n_samples, PathArrays a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    paths_begin_sample(sc, ch, i, a);
}

// Regrouping of a bounce's segments (k_paths_keys → radix sort → k_paths_gather).  Key = Morton code of
// the lattice cell the segment starts in, computed in the space the medium's grid lives in: in
// isotropic-ray space every ray travels along the lattice's +z axis (SCN.cpp:296-301: the frame's normal
// is the whitened direction), so segments that start in the same lattice cell stay neighbours for
// their whole length, whatever their world-space directions; in world space the direction octant is
// appended.  Dead paths get the largest key: the sort is also the compaction.
__device__ __forceinline__ uint32_t spread3(uint32_t v)   // 9 bits -> every third bit
{
    v &= 0x1FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__global__ void __launch_bounds__(256) k_paths_keys(const DevModel *__restrict__ Mp, float cell_size, size_t n, const gpis_ray_in *__restrict__ rays,
                                                    const uint8_t *__restrict__ alive, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t key = 0xFFFFFFFFu;
    if (alive[i]) {
        const DevModel &M = *Mp;
        const V3 p = v3(rays[i].pos[0], rays[i].pos[1], rays[i].pos[2]);
        const V3 d = v3(rays[i].dir[0], rays[i].dir[1], rays[i].dir[2]);
        V3 u = p;
        if (M.iso3d) {
            const Frame coord = frame_from_normal(normalized(generic::cov_pos_w2l(M, d, 1.0f)));
            u = to_local(coord, generic::cov_pos_w2l(M, p, 1.0f));
        }
        const float inv = 1.0f / cell_size;
        const int cx = (int)floorf(fminf(fmaxf(u.x * inv, -255.f), 255.f)) + 256;
        const int cy = (int)floorf(fminf(fmaxf(u.y * inv, -255.f), 255.f)) + 256;
        const int cz = (int)floorf(fminf(fmaxf(u.z * inv, -255.f), 255.f)) + 256;
        const uint32_t morton = (spread3((uint32_t)cx) << 2) | (spread3((uint32_t)cy) << 1) | spread3((uint32_t)cz);
        const uint32_t oct = M.iso3d ? 0u : ((d.x < 0.f ? 4u : 0u) | (d.y < 0.f ? 2u : 0u) | (d.z < 0.f ? 1u : 0u));
        key = (morton << 3) | oct;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}
__global__ void __launch_bounds__(256) k_paths_gather(size_t n, const uint32_t *__restrict__ keys_sorted, const uint32_t *__restrict__ order,
                                                      const gpis_ray_in *__restrict__ rays, gpis_ray_in *__restrict__ rays_sorted,
                                                      uint8_t *__restrict__ live_sorted)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool live = keys_sorted[j] != 0xFFFFFFFFu;
    live_sorted[j] = live ? 1 : 0;
    if (live)
        rays_sorted[j] = rays[order[j]];
}

// after sampleDistance of segment `bounce`: next-event estimation set-up + the bounce itself.
// Slot j of the batch (seg, shadow, nee, contrib, vis, and rays_in) belongs to path i = order[j]
// (identity when order is null); the path state (rng, throughput, emission, alive, next ray) is
// indexed by i.
__global__ void __launch_bounds__(256) k_paths_shade(SceneConst sc, size_t n_samples, int bounce, int max_bounces, float albedo, PathArrays a,
                                                     const uint32_t *__restrict__ order, const gpis_ray_in *__restrict__ rays_in,
                                                     const uint8_t *__restrict__ live)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_samples) return;
    uint8_t nee = 0;
    if (live ? !live[j] : !a.alive[j]) { a.nee[j] = 0; return; }
    const size_t i = order ? (size_t)order[j] : j;
    const gpis_seg_out o = a.seg[j];
    if (!o.ok) { a.alive[i] = 0; a.nee[j] = 0; return; }
    float thr = a.throughput[i] * o.weight[0];
    if (o.exited) { a.alive[i] = 0; a.nee[j] = 0; a.throughput[i] = thr; return; }
    const gpis_ray_in ray = rays_in[j];
    Pcg32 g;
    g.state = a.rng[i];
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    const V3 n = hit_normal(o);
    const Frame fr = frame_from_normal(n);
    const V3 dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
    const V3 wi = normalized(to_local(fr, v3(-dir.x, -dir.y, -dir.z)));
    const V3 p = v3(o.p[0], o.p[1], o.p[2]);
    gpis_ray_in next;
    memset(&next, 0, sizeof next);
    next.pos[0] = p.x; next.pos[1] = p.y; next.pos[2] = p.z;
    next.near_t = 0.f;
    next.pixel[0] = ray.pixel[0]; next.pixel[1] = ray.pixel[1]; next.spp = ray.spp;
    next.scene_seed = ray.scene_seed;
    next.info_t = ray.info_t + o.sample_t;
    next.first_scatter = 0;
    next.bounce = ray.bounce + 1;
    next.last_val = o.last_val;
    next.last_gp_id = o.gp_id;
    next.last_aniso[0] = o.aniso[0]; next.last_aniso[1] = o.aniso[1]; next.last_aniso[2] = o.aniso[2];
    if (bounce < max_bounces - 1) {
        const V3 wo = normalized(to_local(fr, l));
        if (wi.z > 0.0f && wo.z > 0.0f) {
            const float f = albedo * (1.0f / 3.1415926536f) * wo.z;
            float t0, t1;
            if (sphere_chord(p, l, sc.s.bound_radius, t0, t1)) {
                gpis_ray_in sh = next;
                sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                sh.far_t = t1;
                sh.segment = (uint32_t)bounce + 1;
                sh.u_jitter = normalized_uint(g.next_i());
                a.shadow[j] = sh;
                a.contrib[j] = thr * (f * sc.s.light_radiance);
                nee = 1;
            }
        }
    }
    a.nee[j] = nee;
    bool alive = wi.z > 0.0f;
    if (alive) {
        float dx, dy, d2;
        do {
            dx = 2.f * normalized_uint(g.next_i()) - 1.f;
            dy = 2.f * normalized_uint(g.next_i()) - 1.f;
            d2 = dx * dx + dy * dy;
        } while (!(d2 < 1.f));
        const float rem = 1.0f - d2;
        const V3 w = normalized(to_global(fr, v3(dx, dy, sqrtf(rem > 0.f ? rem : 0.f))));
        thr *= albedo;
        float t0, t1;
        alive = sphere_chord(p, w, sc.s.bound_radius, t0, t1);
        if (alive) {
            next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
            next.far_t = t1;
            next.segment = (uint32_t)bounce + 1;
            next.u_jitter = normalized_uint(g.next_i());
            a.rays[i] = next;
        }
    }
    a.alive[i] = alive ? 1 : 0;
    a.throughput[i] = thr;
    a.rng[i] = g.state;
}

// slot k of the (possibly regrouped) shadow batch -> slot j of the bounce batch -> path i
__global__ void __launch_bounds__(256) k_paths_nee_add(size_t n_samples, PathArrays a, const uint32_t *__restrict__ order,
                                                       const uint32_t *__restrict__ shadow_order, const uint8_t *__restrict__ shadow_live,
                                                       const uint8_t *__restrict__ vis)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_samples) return;
    if (shadow_order ? !shadow_live[k] : !a.nee[k]) return;
    const size_t j = shadow_order ? (size_t)shadow_order[k] : k;
    a.emission[order ? (size_t)order[j] : j] += vis[k] ? a.contrib[j] : 0.f;
}

// What a sample of a mono path driver is worth (gpis_render_scene_s_paths, gpis_render_scene_s_nee[_paths], the per-sample E of the
// RGB drivers where k_paths_accumulate runs on it, and their adaptive forms) — an accessor of gpis_frame_sum.hpp on the per-sample E
// and the segments marched for the sample (NULL where the driver counts none or the caller wants none).  raw: E as the uniform
// entries add it, unclamped; value: E after renderTile's clamp, as the adaptive entries add and account it; a clamped sample's
// segments count too.
struct PathValues {
    const float *emission;
    const uint32_t *segs;
    GPIS_DEV float raw(size_t i) const { return emission[i]; }
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(raw(i)); }
    GPIS_DEV uint32_t count(size_t i) const { return segs ? segs[i] : 0u; }
};
// The luminance plane k_rgb_adaptive_value leaves of a chunk of the RGB path driver: clamped there already, so value(i) is the
// plane's float as it stands (clamping a luminance a second time can differ at 65536).  The statistics alone read it.
struct LuminanceValues {
    const float *luminance;
    GPIS_DEV float value(size_t i) const { return luminance[i]; }
};

// one lane per pixel: sequential sum over its samples' E, in sample order
__global__ void __launch_bounds__(256) k_paths_accumulate(SceneConst sc, size_t first_pixel, size_t n_pixels, const float *__restrict__ emission,
                                                          float *__restrict__ radiance_sum)
{
    frame_values_sum(sc, first_pixel, n_pixels, PathValues{emission, nullptr}, radiance_sum, nullptr);
}

// The mono path drivers and the RGB path driver under the adaptive schedule, behind the bounce loop of a chunk of records: the
// per-pixel sum of the variable-count layout (the segments where `segs` is given; seg_count is then the caller's) and the tile
// statistics.
namespace gpis {
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_paths_adaptive_sum(SceneConst sc, AdaptiveChunk ch, const float *__restrict__ emission,
                                                                           const uint32_t *__restrict__ segs, float *__restrict__ radiance_sum,
                                                                           uint32_t *__restrict__ sample_count, uint32_t *__restrict__ seg_count)
{
    adaptive_values_sum(sc, ch, PathValues{emission, segs}, radiance_sum, sample_count, seg_count);
}
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_paths_adaptive_tile_stats(AdaptiveChunk ch, const float *__restrict__ emission,
                                                                                  gpis_adaptive_record *__restrict__ records)
{
    adaptive_values_stats(ch, PathValues{emission, nullptr}, records);
}
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_rgb_adaptive_stats(AdaptiveChunk ch, const float *__restrict__ luminance,
                                                                           gpis_adaptive_record *__restrict__ records)
{
    adaptive_values_stats(ch, LuminanceValues{luminance}, records);
}
}   // namespace gpis

// one lane per pixel: the sum of a per-sample count over its spp (the segments marched for a pixel's samples, path plus shadow: the
// RGB path drivers and gpis_render_scene_s_nee_paths)
__global__ void __launch_bounds__(256) k_scene_sum_u32(SceneConst sc, size_t first_pixel, size_t n_pixels, const uint32_t *__restrict__ per_sample,
                                                       uint32_t *__restrict__ per_pixel)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pixels) return;
    const uint32_t spp = sc.s.spp_count;
    uint32_t acc = 0;
    for (uint32_t k = 0; k < spp; ++k)
        acc += per_sample[j * spp + k];
    per_pixel[scene_pixel(sc.s, first_pixel + j)] += acc;
}

// --------------------------------------------------------------------------------------
// scene S with the specular NEE coupling (gpis_render_scene_s_nee): TraceBase.cpp:346-420,
// BRDFPhaseFunction.cpp:27-96, ConductorBsdf.cpp:59-139, Fresnel.hpp:102-123.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ float conductor_reflectance(float eta, float k, float cosThetaI)
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
__device__ __forceinline__ float power_heuristic(float pdf0, float pdf1) { return (pdf0 * pdf0) / (pdf0 * pdf0 + pdf1 * pdf1); }

template <int N>           // channels: 1 (gpis_surface_s) or 3 (gpis_surface_rgb_s, gpis_cond_rgb.hpp)
struct NeeAuxN {           // per sample, between the set-up and the shading kernel
    float d[3];            // sampled light direction
    float w[3];            // mirror direction of the phase sample
    float F[N];            // albedo * conductorReflectance(wi.z), per channel
    float v1, v2;          // the next two draws of the sample's stream (march jitters of the shadow segments)
    int32_t scheme;
};
using NeeAux = NeeAuxN<1>;
// fn(c) for every channel, stated without a loop: the mono kernels compile to the code they had before the estimator had channels
template <int N, typename Fn>
__device__ __forceinline__ void for_channels(Fn fn)
{
    static_assert(N == 1 || N == 3, "one channel or RGB");
    fn(0);
    if constexpr (N == 3) { fn(1); fn(2); }
}
// channel c of a surface: the mono surface has one
__device__ __forceinline__ float surface_F(const gpis_surface_s &sf, int, float cosThetaI) { return sf.albedo * conductor_reflectance(sf.eta, sf.k, cosThetaI); }
__device__ __forceinline__ float surface_F(const gpis_surface_rgb_s &sf, int c, float cosThetaI)
{
    return sf.albedo[c] * conductor_reflectance(sf.eta[c], sf.k[c], cosThetaI);
}
__device__ __forceinline__ float surface_cap_radiance(const gpis_surface_s &sf, int) { return sf.cap_radiance; }
__device__ __forceinline__ float surface_cap_radiance(const gpis_surface_rgb_s &sf, int c) { return sf.cap_radiance[c]; }
struct NeeArrays {
    gpis_cond_coeff *coeff;
    gpis_nee_query *q_half, *q_normal;
    NeeAux *aux;
    gpis_ray_in *shadow_light, *shadow_phase;
    float *pdf_half, *grad_half, *pdf_normal;
    float *contrib_light, *contrib_phase;
    uint8_t *want_light, *want_phase, *want_pdf_normal, *go_light, *go_phase, *vis_light, *vis_phase;
};

// ---- the light and phase estimators of one hit, stated once for the single-bounce driver (k_nee_setup, k_nee_shade,
// k_nee_gather) and the path driver (k_nee_paths_setup, k_nee_paths_shade, k_nee_paths_gather).

// Before the neePDF / neeGrad launches, at the hit `o` of `ray` (sample i): F, the light direction (volumeLightSample: a direction
// inside the cap, drawn from g — z, then the disk pairs — for the schemes NEE and MIS) with its half-vector query, and the mirror
// direction of ConductorBsdf::sample for EVERY scheme (the path driver bounces along it) with, for UNI and MIS, the test whether
// it sees the cap and the query at the sampled normal.  Fills x but v1 / v2; writes b.q_half[i] / b.q_normal[i] where wanted.
// Only F depends on the channel.
template <int N, typename Surface>
__device__ __forceinline__ void nee_setup_sample(const SceneConst &sc, const Surface &sf, const gpis_ray_in &ray, const gpis_seg_out &o,
                                                 Pcg32 &g, size_t i, const NeeArrays &b, NeeAuxN<N> &x, uint8_t &wl, uint8_t &wp, uint8_t &wn)
{
    x.scheme = o.scheme;
    const V3 capDir = v3(sc.light[0], sc.light[1], sc.light[2]);
    const V3 n = hit_normal(o);
    const Frame fr = frame_from_normal(n);
    const V3 dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
    const V3 wi = normalized(to_local(fr, v3(-dir.x, -dir.y, -dir.z)));
    for_channels<N>([&](int c) __attribute__((always_inline)) { x.F[c] = surface_F(sf, c, wi.z); });
    gpis_nee_query q;
    memset(&q, 0, sizeof q);
    q.ray_dir[0] = dir.x; q.ray_dir[1] = dir.y; q.ray_dir[2] = dir.z;
    q.p[0] = o.p[0]; q.p[1] = o.p[1]; q.p[2] = o.p[2];
    q.t_segment = o.sample_t;
    q.info_t = ray.info_t + o.sample_t;
    q.pixel[0] = ray.pixel[0]; q.pixel[1] = ray.pixel[1]; q.spp = ray.spp; q.segment = ray.segment;
    q.scene_seed = ray.scene_seed;
    q.coeff = b.coeff[i];
    x.d[0] = x.d[1] = x.d[2] = 0.f;
    if (x.scheme != GPIS_UNI) {     // volumeLightSample: a direction inside the cap
        const float z = normalized_uint(g.next_i()) * (1.0f - sf.cap_cos) + sf.cap_cos;
        float dx, dy, d2;
        do {
            dx = 2.f * normalized_uint(g.next_i()) - 1.f;
            dy = 2.f * normalized_uint(g.next_i()) - 1.f;
            d2 = dx * dx + dy * dy;
        } while (!(d2 < 1.f) || !(d2 > 1e-12f));
        const float rr = 1.0f - z * z;
        const float rad = sqrtf(rr > 0.f ? rr : 0.f) / sqrtf(d2);
        const Frame cf = frame_from_normal(capDir);
        const V3 d = to_global(cf, v3(dx * rad, dy * rad, z));
        const V3 wo = normalized(to_local(fr, d));
        const V3 nl = (wi + wo) * 0.5f;
        const V3 nw = normalized(to_global(fr, nl));
        x.d[0] = d.x; x.d[1] = d.y; x.d[2] = d.z;
        gpis_nee_query qh = q;
        qh.normal[0] = nw.x; qh.normal[1] = nw.y; qh.normal[2] = nw.z;
        b.q_half[i] = qh;
        wl = 1;
    }
    const V3 w = normalized(to_global(fr, v3(-wi.x, -wi.y, wi.z)));     // ConductorBsdf::sample: mirror about the sampled normal
    x.w[0] = w.x; x.w[1] = w.y; x.w[2] = w.z;
    if (x.scheme != GPIS_NEE) {     // volumePhaseSample
        float t0, t1;
        if (!(dot(w, capDir) < sf.cap_cos) && sphere_chord(v3(o.p[0], o.p[1], o.p[2]), w, sc.s.bound_radius, t0, t1)) {
            wp = 1;
            if (x.scheme != GPIS_UNI) {
                gpis_nee_query qn = q;
                qn.normal[0] = n.x; qn.normal[1] = n.y; qn.normal[2] = n.z;
                b.q_normal[i] = qn;
                wn = 1;
            }
        }
    }
}

// After the neePDF / neeGrad launches, for a sample with want_light or want_phase: the shadow segments that are marched (gl, gp;
// the light's takes the jitter x.v1, the phase's the next one) and what each adds to L when it is visible: channel c into
// contrib_light / contrib_phase[c * plane + i].  The light's segment is marched unless f is zero in EVERY channel (Vec3f == 0.0f,
// Vec.hpp:452-458); the pdfs and the heuristics are scalars.
template <int N, typename Surface>
__device__ __forceinline__ void nee_shade_sample(const SceneConst &sc, const Surface &sf, const gpis_ray_in &ray, const gpis_seg_out &o,
                                                 const NeeAuxN<N> &x, size_t i, const NeeArrays &b, float *contrib_light, float *contrib_phase, size_t plane,
                                                 uint8_t &gl, uint8_t &gp)
{
    const float pdf_l = (0.5f * (1.0f / 3.1415926536f)) / (1.0f - sf.cap_cos);
    const V3 p = v3(o.p[0], o.p[1], o.p[2]);
    const gpis_ray_in sh0 = scene_next_ray(ray, o);      // handleVolume's copy of the state: segment word + 1
    if (b.want_light[i]) {
        const float pdf = b.pdf_half[i];
        float f[N];
        bool some = false;
        for_channels<N>([&](int c) __attribute__((always_inline)) {
            f[c] = x.F[c] * pdf;
            some = some || f[c] != 0.0f;
        });
        float t0, t1;
        const V3 d = v3(x.d[0], x.d[1], x.d[2]);
        if (some && sphere_chord(p, d, sc.s.bound_radius, t0, t1)) {
            gpis_ray_in sh = sh0;
            sh.dir[0] = d.x; sh.dir[1] = d.y; sh.dir[2] = d.z;
            sh.far_t = t1;
            sh.u_jitter = x.v1;
            sh.last_aniso[0] = (double)b.grad_half[3 * i]; sh.last_aniso[1] = (double)b.grad_half[3 * i + 1]; sh.last_aniso[2] = (double)b.grad_half[3 * i + 2];
            b.shadow_light[i] = sh;
            for_channels<N>([&](int c) __attribute__((always_inline)) {
                const float e = 1.f * surface_cap_radiance(sf, c);
                float lightF = f[c] * e / pdf_l;
                if (x.scheme != GPIS_NEE)
                    lightF *= power_heuristic(pdf_l, pdf);
                contrib_light[c * plane + i] = lightF;
            });
            gl = 1;
        }
    }
    if (b.want_phase[i]) {
        float t0, t1;
        const V3 w = v3(x.w[0], x.w[1], x.w[2]);
        (void)sphere_chord(p, w, sc.s.bound_radius, t0, t1);   // known to succeed (nee_setup_sample)
        gpis_ray_in sh = sh0;
        sh.dir[0] = w.x; sh.dir[1] = w.y; sh.dir[2] = w.z;
        sh.far_t = t1;
        sh.u_jitter = gl ? x.v2 : x.v1;
        b.shadow_phase[i] = sh;
        for_channels<N>([&](int c) __attribute__((always_inline)) {
            const float e = 1.f * surface_cap_radiance(sf, c);
            float phaseF = e * x.F[c];
            if (x.scheme != GPIS_UNI)
                phaseF *= power_heuristic(b.pdf_normal[i], pdf_l);
            contrib_phase[c * plane + i] = phaseF;
        });
        gp = 1;
    }
}

// After the shadow marches: L of sample i
__device__ __forceinline__ float nee_gather_sample(float cap_radiance, size_t i, const NeeArrays &b)
{
    float L = 0.f;
    if (cap_radiance != 0.0f) {     // e == 0 ends both estimators (TraceBase.cpp:374, 410)
        if (b.go_light[i] && b.vis_light[i]) L += b.contrib_light[i];
        if (b.go_phase[i] && b.vis_phase[i]) L += b.contrib_phase[i];
    }
    return L;
}

__global__ void __launch_bounds__(256) k_nee_setup(SceneConst sc, gpis_surface_s sf, size_t n_samples, PathArrays a, NeeArrays b)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t wl = 0, wp = 0, wn = 0;
    const gpis_seg_out o = a.seg[i];
    if (a.alive[i] && o.ok && !o.exited) {
        const gpis_ray_in ray = a.rays[i];
        Pcg32 g;
        g.state = a.rng[i];
        NeeAux x;
        nee_setup_sample(sc, sf, ray, o, g, i, b, x, wl, wp, wn);
        x.v1 = normalized_uint(g.next_i());
        x.v2 = normalized_uint(g.next_i());
        b.aux[i] = x;
    }
    b.want_light[i] = wl;
    b.want_phase[i] = wp;
    b.want_pdf_normal[i] = wn;
}

__global__ void __launch_bounds__(256) k_nee_shade(SceneConst sc, gpis_surface_s sf, size_t n_samples, PathArrays a, NeeArrays b)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t gl = 0, gp = 0;
    if (b.want_light[i] || b.want_phase[i])
        nee_shade_sample(sc, sf, a.rays[i], a.seg[i], b.aux[i], i, b, b.contrib_light, b.contrib_phase, 0, gl, gp);
    b.go_light[i] = gl;
    b.go_phase[i] = gp;
}

__global__ void __launch_bounds__(256) k_nee_gather(float cap_radiance, size_t n_samples, PathArrays a, NeeArrays b)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    a.emission[i] = nee_gather_sample(cap_radiance, i, b);
}

// ---- the bounce loop of the same estimator (gpis_render_scene_s_nee_paths): PathTracer.cpp:62-169 over TraceBase.cpp:539-563,
// ConductorBsdf.cpp:59-76.  Per bounce: march the live paths, k_nee_paths_setup, neePDF / neeGrad, k_nee_paths_shade, the two
// shadow marches, k_nee_paths_gather.  a.alive is the mask of each stage in turn: the paths to march, then (set-up) the paths that
// hit, then (shade) the paths whose next segment a.rays holds.
struct NeePathArrays {     // per sample
    float *thr_hit;        // throughput at this bounce's hit, weight[0] included and F not: the factor of L
    uint32_t *segs;        // segments marched so far: path, light shadow and phase shadow segments
};

__global__ void __launch_bounds__(256) k_nee_paths_setup(SceneConst sc, gpis_surface_s sf, size_t n_samples, PathArrays a, NeeArrays b, NeePathArrays c)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t wl = 0, wp = 0, wn = 0;
    if (a.alive[i]) {
        c.segs[i] += 1;
        uint8_t hit = 0;
        const gpis_seg_out o = a.seg[i];
        if (o.ok) {
            const float thr = a.throughput[i] * o.weight[0];
            a.throughput[i] = thr;
            if (!o.exited) {        // the light seen directly is never added
                const gpis_ray_in ray = a.rays[i];
                Pcg32 g;
                g.state = a.rng[i];
                NeeAux x;
                nee_setup_sample(sc, sf, ray, o, g, i, b, x, wl, wp, wn);
                a.rng[i] = g.state;     // v1, v2 look ahead: how many of them the shadow segments take is known after neePDF
                x.v1 = normalized_uint(g.next_i());
                x.v2 = normalized_uint(g.next_i());
                b.aux[i] = x;
                c.thr_hit[i] = thr;
                hit = 1;
            }
        }
        a.alive[i] = hit;
    }
    b.want_light[i] = wl;
    b.want_phase[i] = wp;
    b.want_pdf_normal[i] = wn;
}

__global__ void __launch_bounds__(256) k_nee_paths_shade(SceneConst sc, gpis_surface_s sf, size_t n_samples, int bounce, int max_bounces, PathArrays a,
                                                         NeeArrays b, NeePathArrays c)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t gl = 0, gp = 0;
    if (a.alive[i]) {       // hit at this bounce
        const gpis_seg_out o = a.seg[i];
        const gpis_ray_in ray = a.rays[i];
        const NeeAux x = b.aux[i];
        if (b.want_light[i] || b.want_phase[i])
            nee_shade_sample(sc, sf, ray, o, x, i, b, b.contrib_light, b.contrib_phase, 0, gl, gp);
        c.segs[i] += (uint32_t)gl + (uint32_t)gp;
        Pcg32 g;
        g.state = a.rng[i];
        for (int k = 0; k < (int)gl + (int)gp; ++k)     // one jitter per shadow segment that is marched
            (void)g.next_i();
        // the bounce: no Russian roulette, no neePDF of the mirror direction (the reference's value is unused)
        const float thr = c.thr_hit[i] * x.F[0];
        a.throughput[i] = thr;
        float t0, t1;
        const V3 w = v3(x.w[0], x.w[1], x.w[2]);
        bool alive = !(thr == 0.0f) && sphere_chord(v3(o.p[0], o.p[1], o.p[2]), w, sc.s.bound_radius, t0, t1) && bounce + 2 < max_bounces;
        if (alive) {
            gpis_ray_in next = scene_next_ray(ray, o);
            next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
            next.far_t = t1;
            next.u_jitter = normalized_uint(g.next_i());
            a.rays[i] = next;
        }
        a.rng[i] = g.state;
        a.alive[i] = alive ? 1 : 0;
    }
    b.go_light[i] = gl;
    b.go_phase[i] = gp;
}

// E = E + thr * L.  A hit without a shadow segment has L = 0 and leaves E as it is.
__global__ void __launch_bounds__(256) k_nee_paths_gather(float cap_radiance, size_t n_samples, PathArrays a, NeeArrays b, NeePathArrays c)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    if (b.go_light[i] || b.go_phase[i])
        a.emission[i] = a.emission[i] + c.thr_hit[i] * nee_gather_sample(cap_radiance, i, b);
}

// ---- the same bounce loop in RGB (gpis_render_scene_s_nee_paths_rgb): k_cond_rgb_setup, k_cond_rgb_emit, k_cond_rgb_shade,
// k_cond_rgb_gather
#include "gpis_cond_rgb.hpp"
// ---- and with the material of a hit chosen by its GP id (gpis_render_scene_s_material_paths_rgb): k_mat_rgb_setup, k_mat_rgb_shade
#include "gpis_material_rgb.hpp"

// ---- scene S driver ----------------------------------------------------------------------
extern "C" void gpis_default_scene_s(gpis_scene_s *s, uint32_t width, uint32_t height, uint32_t spp)
{
    memset(s, 0, sizeof *s);
    s->width = width; s->height = height;
    s->spp_begin = 0; s->spp_count = spp;
    s->scene_seed = 0xBA5EBA11u;
    s->tile_size = 16;
    s->cam_pos[0] = 0.f; s->cam_pos[1] = 0.f; s->cam_pos[2] = 4.f;
    s->cam_fov_deg = 35.f;
    s->bound_radius = 1.5f;
    s->light_dir[0] = 0.5f; s->light_dir[1] = 0.7f; s->light_dir[2] = 0.5f;
    s->light_radiance = 1.f;
    s->y_begin = 0; s->y_count = height;
    s->shard_index = 0; s->shard_count = 1;
}

// Samples per chunk of the tile drivers: 2^default_log2 unless GPIS_CHUNK_LOG2 says otherwise.  Chunks are
// sized for the 288 GB of an MI355X — one launch per stage and frame where it fits — because every launch
// ends in a tail of half-empty waves and the wavefront march in a tail of thin iterations (C1 frame:
// 8 Mi-sample chunks 268.8, 32 Mi 284.8, 128 Mi 291.3 Msamples/s; multi-bounce 65 → 80 M paths/s).
static int chunk_log2(const gpis_medium *m, int default_log2)
{
    return m->opt[GPIS_OPT_CHUNK_LOG2] ? (int)m->opt[GPIS_OPT_CHUNK_LOG2] : default_log2;
}
// pixels per chunk of a frame of total_pixels pixels at spp samples each, for chunks of about 2^log2_samples samples: whole pixels,
// at least one, at most the frame
static size_t chunk_pixels_of(int log2_samples, uint32_t spp, size_t total_pixels)
{
    size_t chunk_pixels = ((size_t)1 << log2_samples) / spp;
    if (chunk_pixels < 1) chunk_pixels = 1;
    if (chunk_pixels > total_pixels) chunk_pixels = total_pixels;
    return chunk_pixels;
}
// grows stage[slot] to `bytes` if the device has the memory; false (and no error state) otherwise
static bool try_stage(gpis_medium *m, int slot, size_t bytes)
{
    if (stage_size(m, slot) >= bytes)
        return true;
    if (ensure_stage(m, slot, bytes) == GPIS_OK)
        return true;
    (void)hipGetLastError();
    return false;
}

// Workspace of the Lambert driver in three allocations: slot 3 [primary rays, overwritten in place by the shadow rays | shadow
// jitter | mask], slot 5 [segment results], slot 6 [cos | mask | visible | hit].  Full-record body: 236 B per sample (gpis_ray_in
// 128 + 5, gpis_seg_out 96, 7).  Compact body (lambert_compact): 71 B per sample (SceneRay 32, which carries the jitter and the
// mask; SceneHit 32; 7).  The chunk is the largest the device can hold, starting from the whole frame (2^27 samples = 9.5 GB
// compact, 31.3 GB full; 48.3 GB with separate shadow rays until round 3).
struct LambertWs {
    bool compact;                                      // which body the sizes are for
    size_t chunk_pixels, ns_max;
    size_t b_prim, b_seg, b_shadow;                    // bytes of slots 3, 5, 6
    size_t o_prim, o_us, o_v1;                         // offsets inside slot 3
    size_t o_cos, o_v2, o_vis, o_hit;                  // offsets inside slot 6
};
// The layout of a workspace for chunks of up to n samples (W.compact says of which body), and whether the device can hold it.
static int lambert_ws_carve(gpis_medium *m, LambertWs &W, size_t n, bool &fits)
{
    const size_t ray_bytes = W.compact ? sizeof(SceneRay) : sizeof(gpis_ray_in), seg_bytes = W.compact ? sizeof(SceneHit) : sizeof(gpis_seg_out);
    W.ns_max = n;
    size_t off = 0;
    W.o_prim = ws_carve(off, n * ray_bytes);
    W.o_us = W.o_v1 = 0;
    if (!W.compact) { W.o_us = ws_carve(off, n * 4); W.o_v1 = ws_carve(off, n); }
    W.b_prim = off;
    W.b_seg = n * seg_bytes;
    off = 0;
    W.o_cos = ws_carve(off, n * 4); W.o_v2 = ws_carve(off, n); W.o_vis = ws_carve(off, n); W.o_hit = ws_carve(off, n);
    W.b_shadow = off;
    // what is still to be allocated must fit the free memory (with 1 GiB to spare)
    const size_t have3 = stage_size(m, 3), have5 = stage_size(m, 5), have6 = stage_size(m, 6);
    const size_t missing = (have3 >= W.b_prim ? 0 : W.b_prim) + (have5 >= W.b_seg ? 0 : W.b_seg) + (have6 >= W.b_shadow ? 0 : W.b_shadow);
    fits = missing == 0;
    if (fits) return GPIS_OK;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t reclaim = (have3 >= W.b_prim ? 0 : have3) + (have5 >= W.b_seg ? 0 : have5) + (have6 >= W.b_shadow ? 0 : have6);   // freed on growth
    fits = missing + ((size_t)1 << 30) <= free_b + reclaim;
    return GPIS_OK;
}
// First-use policy: memory this process allocates for the first time costs 15-30 ms per GB on these boxes (DESIGN.md §6 "cold
// frame"), so the whole-frame workspace (9.5 GB compact, 31 GB full) would add to the latency of a handle's FIRST frame.  That frame
// therefore runs in 16 Mi-sample chunks (1.2 GB compact, 4 GB full; -4 % throughput); from the second call on — the handle is evidently reused — the workspace grows to
// the whole frame.  A workspace that is already large enough (gpis_reserve_scene_workspace, an earlier larger call) is used as is,
// and GPIS_CHUNK_LOG2 / GPIS_OPT_CHUNK_LOG2 override the policy.
static int lambert_ws_plan(gpis_medium *m, const gpis_scene_s *s, size_t total_pixels, LambertWs &W, bool guided, bool first_call = false)
{
    int l0 = chunk_log2(m, 27);
    W.compact = lambert_compact(m, guided);
    const size_t ray_bytes = W.compact ? sizeof(SceneRay) : sizeof(gpis_ray_in), seg_bytes = W.compact ? sizeof(SceneHit) : sizeof(gpis_seg_out);
    if (first_call && !m->opt[GPIS_OPT_CHUNK_LOG2]) {
        const size_t whole = (total_pixels * s->spp_count < ((size_t)1 << 27) ? total_pixels * s->spp_count : ((size_t)1 << 27));
        const bool have_whole = stage_size(m, 3) >= whole * (ray_bytes + (W.compact ? 0 : 5)) && stage_size(m, 5) >= whole * seg_bytes && stage_size(m, 6) >= whole * 7;
        if (!have_whole) l0 = 24;
    }
    for (int l = l0;; --l) {
        W.chunk_pixels = chunk_pixels_of(l, s->spp_count, total_pixels);
        bool fits = false;
        if (int rc = lambert_ws_carve(m, W, W.chunk_pixels * s->spp_count, fits)) return rc;
        if (fits) return GPIS_OK;
        if (l <= 20) return set_err(GPIS_ERR_DEVICE, "scene driver: no memory for a 1 Mi-sample workspace");
    }
}

extern "C" int gpis_reserve_scene_workspace(gpis_medium *m, const gpis_scene_s *s)
{
    CHECK_ARGS(std_handle(m) && s);
    CHECK_ARGS(scene_args_ok(s));
    HIP_TRY(hipSetDevice(m->device));
    LambertWs W;
    // Sized for the guided body wherever the medium can carry a guide: the call is made beside gpis_build_guide, before the guide
    // is enabled.  A handle that then renders without a guide grows the three arrays on demand.
    if (int rc = lambert_ws_plan(m, s, scene_rows(*s) * s->width, W, m->fast.enabled != 0)) return rc;
    if (int rc = ensure_stage(m, 3, W.b_prim, true)) return rc;      // in the order the first frame needs them
    if (int rc = ensure_stage(m, 5, W.b_seg, true)) return rc;
    return ensure_stage(m, 6, W.b_shadow, true);
}

// The camera step of ns samples laid out by `where` (k_scene_primary) into compact records, or into full records with the shadow
// jitters and the mask beside them.
template <typename Where>
static int scene_primary(const SceneConst &sc, const Where &where, size_t ns, hipStream_t st, SceneRay *rays)
{
    k_scene_primary_c<<<grid_of(ns, 256), 256, 0, st>>>(sc, where, ns, rays);
    return launch_check("k_scene_primary_c");
}
template <typename Where>
static int scene_primary(const SceneConst &sc, const Where &where, size_t ns, hipStream_t st, gpis_ray_in *rays, float *u_shadow, uint8_t *valid)
{
    k_scene_primary<<<grid_of(ns, 256), 256, 0, st>>>(sc, where, ns, rays, u_shadow, valid);
    return launch_check("k_scene_primary");
}

// One chunk of ns samples of the Lambert frame, in the workspace W lays out: the camera step, the primary march, the shade kernel
// and the shadow march, on 32-byte records (W.compact: a ray record carries its mask and the shadow jitter) or on full records; in
// both the shadow ray is written over the primary ray it came from.  `camera` is the driver's camera step: it is called with the
// arrays of the body that runs — (SceneRay *) or (gpis_ray_in *, shadow jitters, mask) — launches and returns its launch_check
// (scene_primary).  `out`: what the driver's own sums read, per sample.
// Each of the three allocations is made (a handle's first frame only; W's sizes are exact) right before the first kernel that
// needs it, i.e. while the kernels launched so far run; a driver that has sized the slots already finds them as they are.
template <typename Camera>
static int lambert_chunk(gpis_medium *m, const SceneConst &sc, const LambertWs &W, size_t ns, hipStream_t st, Camera camera, AdaptiveLambert &out)
{
    int rc = GPIS_OK;
    if ((rc = ensure_stage(m, 3, W.b_prim, true))) return rc;
    char *ws3 = (char *)m->stage[3].p;
    SceneRay *cray = (SceneRay *)(ws3 + W.o_prim);
    gpis_ray_in *prim = (gpis_ray_in *)(ws3 + W.o_prim);
    float *us = (float *)(ws3 + W.o_us);
    uint8_t *v1 = (uint8_t *)(ws3 + W.o_v1);
    if ((rc = W.compact ? camera(cray) : camera(prim, us, v1))) return rc;
    if ((rc = ensure_stage(m, 5, W.b_seg, true))) return rc;
    SceneHit *chit = (SceneHit *)m->stage[5].p;
    gpis_seg_out *seg = (gpis_seg_out *)m->stage[5].p;
    // k_scene_shade reads only ok / exited of a segment that exits: its lastVal and gradient are not evaluated (GPIS_OPT_SCENE_EXIT_STATE)
    if ((rc = W.compact ? scene_sample_distance_compact(m, ns, cray, chit, sc.s.cam_pos, st)
                        : sample_distance_impl(m, ns, prim, seg, nullptr, v1, st, MARCH_COHERENT, m->opt[GPIS_OPT_SCENE_EXIT_STATE] != 0)))
        return rc;
    if ((rc = ensure_stage(m, 6, W.b_shadow, true))) return rc;
    char *ws6 = (char *)m->stage[6].p;
    float *cosl = (float *)(ws6 + W.o_cos);
    uint8_t *v2 = (uint8_t *)(ws6 + W.o_v2), *vis = (uint8_t *)(ws6 + W.o_vis), *hit = (uint8_t *)(ws6 + W.o_hit);
    if (W.compact) {
        k_scene_shade_c<<<grid_of(ns, 256), 256, 0, st>>>(sc, ns, cray, chit, cosl, v2, hit);
        if ((rc = launch_check("k_scene_shade_c"))) return rc;
        if ((rc = scene_transmittance_compact(m, ns, cray, sc.light, vis, st))) return rc;
    } else {
        k_scene_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, ns, prim, seg, us, v1, prim, cosl, v2, hit);
        if ((rc = launch_check("k_scene_shade"))) return rc;
        if ((rc = transmittance_impl(m, ns, prim, vis, v2, st))) return rc;
    }
    out = AdaptiveLambert{cosl, v2, vis, hit};
    return GPIS_OK;
}

extern "C" int gpis_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum, uint32_t *hit_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && radiance_sum);
    CHECK_ARGS(scene_args_ok(s));
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    LambertWs W;
    if (int rc0 = lambert_ws_plan(m, s, total_pixels, W, m->guide.enabled != 0, m->lambert_calls == 0)) return rc0;
    ++m->lambert_calls;
    int rc = GPIS_OK;
    if ((rc = ws_acquire(m, 0, st))) return rc;
    const size_t chunk_pixels = W.chunk_pixels;
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        size_t ns = np * s->spp_count;
        AdaptiveLambert a;
        if ((rc = lambert_chunk(m, sc, W, ns, st, [&](auto... arrays) { return scene_primary(sc, p0, ns, st, arrays...); }, a))) return rc;
        k_scene_accumulate<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, a.cosl, a.valid2, a.vis, a.hit, radiance_sum, hit_count);
        if ((rc = launch_check("k_scene_accumulate"))) return rc;
    }
    return ws_release(m, 0, st);
}

// What the pass loop of the adaptive frame drivers (gpis_adaptive_host.hpp) takes of a sparse-convolution handle: its lock and device,
// chunks of 2^l samples (GPIS_OPT_CHUNK_LOG2, else the driver's default_log2), the workspace slot 0 around the passes, and nothing
// of its own at a pass's synchronisation.
namespace {
struct MediumPasses {
    gpis_medium *m;
    int default_log2;
    std::mutex &mu() const { return m->mu; }
    int device() const { return m->device; }
    int chunk_log2() const { return ::chunk_log2(m, default_log2); }
    int acquire(hipStream_t st) const { return ws_acquire(m, 0, st); }
    int release(hipStream_t st) const { return ws_release(m, 0, st); }
    int before_sync(hipStream_t) const { return GPIS_OK; }
    int after_sync(hipStream_t) const { return GPIS_OK; }
};
}

// gpis_render_scene_s under the reference's adaptive sample schedule: per chunk of whole records the stages of gpis_render_scene_s
// (lambert_chunk, seeded through the variable-count layout), the pixel sum of that layout and the tile statistics.
extern "C" int gpis_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, float *radiance_sum, uint32_t *sample_count,
                                            uint32_t *hit_count, gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && radiance_sum && sample_count);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    LambertWs W;
    return adaptive_passes(
        MediumPasses{m, 27}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            W.compact = lambert_compact(m, m->guide.enabled != 0);
            return lambert_ws_carve(m, W, n, fits);
        },
        [&]() {
            if (int rc = ensure_stage(m, 3, W.b_prim, true)) return rc;
            if (int rc = ensure_stage(m, 5, W.b_seg, true)) return rc;
            return ensure_stage(m, 6, W.b_shadow, true);
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            int rc = GPIS_OK;
            AdaptiveLambert arrays;
            if ((rc = lambert_chunk(m, sc, W, ns, st, [&](auto... rays) { return scene_primary(sc, ch, ns, st, rays...); }, arrays))) return rc;
            k_adaptive_accumulate<0><<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(sc, ch, arrays, radiance_sum, sample_count,
                                                                                                                   hit_count);
            if ((rc = launch_check("k_adaptive_accumulate"))) return rc;
            k_adaptive_stats<0><<<grid_of(ch.nrec, 256), 256, 0, st>>>(sc, ch, arrays, d_records);
            return launch_check("k_adaptive_stats");
        });
}

// The frame loop of the function-space scene-S drivers: per chunk of samples one fused launch over the resident set of the
// function-space workspace (`march`: scene constants, grid, first pixel, samples) and the per-pixel sum of its records (`sum`:
// scene constants, first pixel, pixels); each launches and returns its launch_check.  Samples per chunk: GPIS_OPT_CHUNK_LOG2,
// else 2^22 as the weight-space frame drivers' (rec_bytes per sample: 32 MB at 8 B).  The entry has checked its arguments (its
// CHECK_ARGS name it and quote its own condition); `entry` names it in the message of the 2^32 guard.
template <typename March, typename Sum>
static int fs_frame(gpis_medium *m, const gpis_scene_s *s, size_t rec_bytes, const char *entry, hipStream_t st, March march, Sum sum)
{
    if (int rc = fs_check(m)) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    if (total_pixels == 0) return GPIS_OK;
    const size_t chunk_pixels = chunk_pixels_of(chunk_log2(m, 22), s->spp_count, total_pixels);
    const size_t ns_max = chunk_pixels * s->spp_count;
    unsigned cap = 0;
    if (int rc = fs_workspace(m, cap, ns_max * rec_bytes)) return rc;
    // the work counter runs to at most n_samples + grid
    if (ns_max + cap >= ((size_t)1 << 32)) return set_err(GPIS_ERR_UNSUPPORTED, "%s: spp_count %u", entry, s->spp_count);
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        HIP_TRY(hipMemsetAsync(m->fs_scene_next.p, 0, sizeof(uint32_t), st));
        if (int rc = march(sc, (unsigned)(ns < cap ? ns : cap), p0, (uint32_t)ns)) return rc;
        if (int rc = sum(sc, p0, np)) return rc;
    }
    return GPIS_OK;
}

// Scene S through the function-space medium (gpis_fs_scene.hpp).
extern "C" int gpis_fs_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum, uint32_t *hit_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && radiance_sum);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    return fs_frame(m, s, launch::fs_scene_rec_bytes(), __func__, st,
                    [&](const SceneConst &sc, unsigned grid, size_t p0, uint32_t ns) {
                        launch::fs_scene(grid, m->d_model.p, sc, p0, ns, m->fs_scene_next.p, m->fs_scene_recs.p, m->fs_ws.p, m->fs_slots, st);
                        return launch_check("k_fs_scene");
                    },
                    [&](const SceneConst &sc, size_t p0, size_t np) {
                        launch::fs_scene_sum(sc, p0, np, m->fs_scene_recs.p, radiance_sum, hit_count, st);
                        return launch_check("k_fs_scene_sum");
                    });
}

// Multi-bounce paths on scene S through the function-space medium (gpis_fs_paths.hpp): the second bank of state slots holds the
// shadow segments' copies.
extern "C" int gpis_fs_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo, float *radiance_sum,
                                            uint32_t *seg_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && radiance_sum && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    return fs_frame(m, s, launch::fs_paths_rec_bytes(), __func__, st,
                    [&](const SceneConst &sc, unsigned grid, size_t p0, uint32_t ns) {
                        launch::fs_paths(grid, m->d_model.p, sc, p0, ns, max_path_bounces, albedo, m->fs_scene_next.p, m->fs_scene_recs.p, m->fs_ws.p, m->fs_slots,
                                         m->fs_slots + m->fs_ws_blocks, st);
                        return launch_check("k_fs_paths");
                    },
                    [&](const SceneConst &sc, size_t p0, size_t np) {
                        launch::fs_paths_sum(sc, p0, np, m->fs_scene_recs.p, radiance_sum, seg_count, st);
                        return launch_check("k_fs_paths_sum");
                    });
}

// The frame loop of the two Lambert path drivers (gpis_render_scene_s_paths, gpis_render_scene_s_paths_rgb): chunks of samples, per
// bounce the regrouping of the secondary segments, the march, the driver's shade kernel, the shadow march and the driver's NEE add.
// The loop owns the arrays the marches read and write (PathsFrame); the driver carves its own path state into the same workspace
// (`state`, called before the allocation with the carving function and the chunk's samples) and takes its pointers from it
// (`bind`).  Segments 0 .. n_marched - 1 are marched; next-event estimation follows the first n_nee of them.  Every callback
// launches and returns its launch_check.  The workspace layout (lambert_paths_carve, lambert_paths_bind) and the body of one chunk
// (lambert_paths_chunk) are functions of their own: the pass loop of gpis_render_scene_s_paths_rgb_adaptive runs the same code.
struct PathsFrame {
    char *ws;                          // stage[3]: the driver's arrays lie at the offsets its `state` carved
    gpis_ray_in *rays, *shadow;        // current segment of every path; the shadow segments of the bounce (by batch slot)
    gpis_seg_out *seg;
    uint8_t *alive, *nee, *vis;
};
// The layout of stage[3] for chunks of up to ns_max samples: the frame's arrays, the driver's own (carved by `state` between them)
// and, when the secondary segments are regrouped, the sort's.
struct PathsWs {
    size_t bytes;
    size_t o_rays, o_seg, o_sh, o_alive, o_nee, o_vis;
    bool regroup, presort;
    size_t sort_temp_bytes;
    size_t o_keys, o_vals, o_keys2, o_order, o_rsorted, o_live, o_temp, o_order2, o_live2;
};
template <typename State>
static int lambert_paths_carve(gpis_medium *m, int n_marched, size_t ns_max, hipStream_t st, State state, PathsWs &W)
{
    size_t off = 0;
    auto carve = [&](size_t bytes) { return ws_carve(off, bytes); };
    W.o_rays = carve(ns_max * sizeof(gpis_ray_in)); W.o_seg = carve(ns_max * sizeof(gpis_seg_out)); W.o_sh = carve(ns_max * sizeof(gpis_ray_in));
    state(carve, ns_max);
    W.o_alive = carve(ns_max); W.o_nee = carve(ns_max); W.o_vis = carve(ns_max);
    // regrouping of secondary segments (GPIS_PATHS_SORT=0 keeps the sample order: results are identical)
    W.regroup = m->opt[GPIS_OPT_PATHS_SORT] != 0 && n_marched > 1;
    W.presort = m->opt[GPIS_OPT_PATHS_PRESORT] != 0;
    W.sort_temp_bytes = 0;
    W.o_keys = W.o_vals = W.o_keys2 = W.o_order = W.o_rsorted = W.o_live = W.o_temp = W.o_order2 = W.o_live2 = 0;
    if (W.regroup) {
        if (sort_pairs_u32(nullptr, W.sort_temp_bytes, nullptr, nullptr, nullptr, nullptr, ns_max, st) != hipSuccess)
            return set_err(GPIS_ERR_DEVICE, "radix sort scratch query failed");
        W.o_keys = carve(ns_max * 4); W.o_vals = carve(ns_max * 4); W.o_keys2 = carve(ns_max * 4); W.o_order = carve(ns_max * 4);
        W.o_rsorted = carve(ns_max * sizeof(gpis_ray_in)); W.o_live = carve(ns_max); W.o_temp = carve(W.sort_temp_bytes);
        W.o_order2 = carve(ns_max * 4); W.o_live2 = carve(ns_max);
    }
    W.bytes = off;
    return GPIS_OK;
}
// the frame's arrays in stage[3], which holds W.bytes
static PathsFrame lambert_paths_bind(gpis_medium *m, const PathsWs &W)
{
    char *ws = (char *)m->stage[3].p;
    PathsFrame f;
    f.ws = ws;
    f.rays = (gpis_ray_in *)(ws + W.o_rays); f.seg = (gpis_seg_out *)(ws + W.o_seg); f.shadow = (gpis_ray_in *)(ws + W.o_sh);
    f.alive = (uint8_t *)(ws + W.o_alive); f.nee = (uint8_t *)(ws + W.o_nee); f.vis = (uint8_t *)(ws + W.o_vis);
    return f;
}
// One chunk of ns samples: `begin` (the driver's camera step), the bounce loop, `finish` (its sums).
template <typename Begin, typename Shade, typename NeeAdd, typename Finish>
static int lambert_paths_chunk(gpis_medium *m, const PathsWs &W, const PathsFrame &f, size_t ns, int n_marched, int n_nee, hipStream_t st, Begin begin,
                               Shade shade, NeeAdd nee_add, Finish finish)
{
    char *ws = f.ws;
    uint32_t *keys = (uint32_t *)(ws + W.o_keys), *vals = (uint32_t *)(ws + W.o_vals), *keys2 = (uint32_t *)(ws + W.o_keys2), *order = (uint32_t *)(ws + W.o_order);
    gpis_ray_in *rays_sorted = (gpis_ray_in *)(ws + W.o_rsorted);
    uint8_t *live_sorted = (uint8_t *)(ws + W.o_live), *live2 = (uint8_t *)(ws + W.o_live2);
    uint32_t *order2 = (uint32_t *)(ws + W.o_order2);
    const DevModel &H = m->host_model;
    const float cell_size = H.iso3d ? (H.radius_iso > 0.f ? H.radius_iso : H.kernel_scale) : (H.radius_world > 0.f ? H.radius_world : 0.1f);
    const bool regroup = W.regroup, presort = W.presort;
    const size_t sort_temp_bytes = W.sort_temp_bytes, o_temp = W.o_temp;
    int rc = GPIS_OK;
    if ((rc = begin())) return rc;
    for (int bounce = 0; bounce < n_marched; ++bounce) {
        // primary segments are coherent as generated (consecutive spp of a pixel); later ones are regrouped
        // Secondary segments are regrouped here by start cell (compaction + locality of the guide steps;
        // GPIS_PATHS_PRESORT=0 skips it when the wavefront march runs, which regroups the exact work
        // itself).  Measured at 4 bounces, C1 1080p x16: sample order + resident march 22.1 M paths/s,
        // regrouped + resident 40.4, wavefront march alone 56.7, regrouped + wavefront 61.3.
        const bool wave = bounce > 0 && m->guide.enabled && wave_march_selected(m, MARCH_SCATTERED);
        const bool sorted = regroup && bounce > 0 && (!wave || presort);
        const int hint = bounce > 0 ? MARCH_SCATTERED : MARCH_COHERENT;
        // src rays + mask -> order, regrouped copy, live flags of the regrouped slots
        auto regroup_batch = [&](const gpis_ray_in *src, const uint8_t *mask, uint32_t *ord, gpis_ray_in *dst, uint8_t *live_out) -> int {
            k_paths_keys<<<grid_of(ns, 256), 256, 0, st>>>(m->d_model.p, cell_size, ns, src, mask, keys, vals);
            int r = launch_check("k_paths_keys");
            if (r) return r;
            size_t tb = sort_temp_bytes;
            if (sort_pairs_u32(ws + o_temp, tb, keys, keys2, vals, ord, ns, st) != hipSuccess)
                return set_err(GPIS_ERR_DEVICE, "radix sort failed");
            k_paths_gather<<<grid_of(ns, 256), 256, 0, st>>>(ns, keys2, ord, src, dst, live_out);
            return launch_check("k_paths_gather");
        };
        if (sorted && (rc = regroup_batch(f.rays, f.alive, order, rays_sorted, live_sorted))) return rc;
        const gpis_ray_in *rays_in = sorted ? rays_sorted : f.rays;
        const uint8_t *live = sorted ? live_sorted : f.alive;
        if ((rc = sample_distance_impl(m, ns, rays_in, f.seg, nullptr, live, st, hint))) return rc;
        if ((rc = shade(bounce, ns, sorted ? order : nullptr, rays_in, sorted ? live_sorted : nullptr))) return rc;
        if (bounce >= n_nee)
            continue;
        if (sorted) {
            // the shadow segments share one direction but start where the bounce segments ended: regroup
            // them by their own lattice cells (the bounce batch's copy of the rays is free again)
            if ((rc = regroup_batch(f.shadow, f.nee, order2, rays_sorted, live2))) return rc;
            if ((rc = transmittance_impl(m, ns, rays_sorted, f.vis, live2, st, hint))) return rc;
            if ((rc = nee_add(ns, order, order2, live2))) return rc;
        } else {
            if ((rc = transmittance_impl(m, ns, f.shadow, f.vis, f.nee, st, hint))) return rc;
            if ((rc = nee_add(ns, nullptr, nullptr, nullptr))) return rc;
        }
    }
    return finish();
}
template <typename State, typename Bind, typename Begin, typename Shade, typename NeeAdd, typename Finish>
static int lambert_paths_frames(gpis_medium *m, const gpis_scene_s *s, int n_marched, int n_nee, hipStream_t st, State state, Bind bind, Begin begin,
                                Shade shade, NeeAdd nee_add, Finish finish)
{
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    const size_t total_pixels = scene_rows(*s) * s->width;
    const size_t chunk_pixels = chunk_pixels_of(chunk_log2(m, 25), s->spp_count, total_pixels);
    PathsWs W;
    int rc = lambert_paths_carve(m, n_marched, chunk_pixels * s->spp_count, st, state, W);
    if (rc) return rc;
    if ((rc = ensure_stage(m, 3, W.bytes))) return rc;
    if ((rc = ws_acquire(m, 0, st))) return rc;
    const PathsFrame f = lambert_paths_bind(m, W);
    bind(f);
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        size_t ns = np * s->spp_count;
        if ((rc = lambert_paths_chunk(m, W, f, ns, n_marched, n_nee, st, [&] { return begin(p0, ns); }, shade, nee_add, [&] { return finish(p0, np); })))
            return rc;
    }
    return ws_release(m, 0, st);
}

namespace {
struct PathsMonoState {                // the path state of the mono Lambert path drivers inside the frame's workspace
    size_t o_rng = 0, o_thr = 0, o_em = 0, o_con = 0;
    PathArrays a;
    template <typename Carve>
    void carve(Carve &carve, size_t ns_max)
    {
        o_rng = carve(ns_max * 8); o_thr = carve(ns_max * 4); o_em = carve(ns_max * 4); o_con = carve(ns_max * 4);
    }
    void bind(const PathsFrame &f)
    {
        a.rays = f.rays; a.seg = f.seg; a.shadow = f.shadow;
        a.rng = (uint64_t *)(f.ws + o_rng);
        a.throughput = (float *)(f.ws + o_thr); a.emission = (float *)(f.ws + o_em); a.contrib = (float *)(f.ws + o_con);
        a.alive = f.alive; a.nee = f.nee; a.vis = f.vis;
    }
};
}
extern "C" int gpis_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo, float *radiance_sum, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && radiance_sum && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    PathsMonoState state;
    const PathArrays &a = state.a;
    // the segment of bounce max-1 cannot contribute (no NEE there, TraceBase.cpp:546, and the
    // light is a Dirac delta), so it is not traced
    return lambert_paths_frames(
        m, s, max_path_bounces - 1, max_path_bounces - 1, st,
        [&](auto &carve, size_t ns_max) { state.carve(carve, ns_max); },
        [&](const PathsFrame &f) { state.bind(f); },
        [&](size_t p0, size_t ns) {
            k_paths_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, p0, ns, a);
            return launch_check("k_paths_begin");
        },
        [&](int bounce, size_t ns, const uint32_t *order, const gpis_ray_in *rays_in, const uint8_t *live) {
            k_paths_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, ns, bounce, max_path_bounces, albedo, a, order, rays_in, live);
            return launch_check("k_paths_shade");
        },
        [&](size_t ns, const uint32_t *order, const uint32_t *order2, const uint8_t *live2) {
            k_paths_nee_add<<<grid_of(ns, 256), 256, 0, st>>>(ns, a, order, order2, live2, a.vis);
            return launch_check("k_paths_nee_add");
        },
        [&](size_t p0, size_t np) {
            k_paths_accumulate<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, a.emission, radiance_sum);
            return launch_check("k_paths_accumulate");
        });
}

// The end of a chunk of records of the mono path drivers under the adaptive schedule: per pixel the sum of the clamped E (and of
// `segs`, where the driver counts segments and the caller wants them), per record the tile statistics.
static int paths_adaptive_finish(const SceneConst &sc, const AdaptiveChunk &ch, hipStream_t st, const float *emission, const uint32_t *segs, float *radiance_sum,
                                 uint32_t *sample_count, uint32_t *seg_count, gpis_adaptive_record *d_records)
{
    k_paths_adaptive_sum<0><<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(sc, ch, emission, seg_count ? segs : nullptr, radiance_sum,
                                                                                                          sample_count, seg_count);
    if (int rc = launch_check("k_paths_adaptive_sum")) return rc;
    k_paths_adaptive_tile_stats<0><<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, emission, d_records);
    return launch_check("k_paths_adaptive_tile_stats");
}

// gpis_render_scene_s_paths under the adaptive sample schedule: the pass loop of gpis_render_scene_s_adaptive around the chunk body
// of the Lambert path drivers, as gpis_render_scene_s_paths_rgb_adaptive below.  A chunk of records is seeded through scene_sample of
// its AdaptiveChunk, runs the bounce loop of gpis_render_scene_s_paths, and ends with the pixel sums and the tile statistics on the
// clamped E of every sample.
extern "C" int gpis_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int max_path_bounces, float albedo,
                                                  float *radiance_sum, uint32_t *sample_count, gpis_adaptive_record *records, gpis_adaptive_info *info,
                                                  void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && radiance_sum && sample_count && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    const int n_marched = max_path_bounces - 1;
    PathsMonoState state;
    const PathArrays &arr = state.a;
    PathsWs W;
    PathsFrame f;
    return adaptive_passes(
        MediumPasses{m, 25}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            const int rc = lambert_paths_carve(m, n_marched, n, st, [&](auto &carve, size_t ns_max) { state.carve(carve, ns_max); }, W);
            if (rc) return rc;
            fits = try_stage(m, 3, W.bytes);
            return (int)GPIS_OK;
        },
        [&]() {
            f = lambert_paths_bind(m, W);
            state.bind(f);
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            return lambert_paths_chunk(
                m, W, f, ns, n_marched, n_marched, st,
                [&] {
                    k_paths_adaptive_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, ch, ns, arr);
                    return launch_check("k_paths_adaptive_begin");
                },
                [&](int bounce, size_t n, const uint32_t *order, const gpis_ray_in *rays_in, const uint8_t *live) {
                    k_paths_shade<<<grid_of(n, 256), 256, 0, st>>>(sc, n, bounce, max_path_bounces, albedo, arr, order, rays_in, live);
                    return launch_check("k_paths_shade");
                },
                [&](size_t n, const uint32_t *order, const uint32_t *order2, const uint8_t *live2) {
                    k_paths_nee_add<<<grid_of(n, 256), 256, 0, st>>>(n, arr, order, order2, live2, arr.vis);
                    return launch_check("k_paths_nee_add");
                },
                [&] { return paths_adaptive_finish(sc, ch, st, arr.emission, nullptr, radiance_sum, sample_count, nullptr, d_records); });
        });
}

// gpis_render_scene_s_paths in RGB with the medium's emission (gpis_paths_rgb.hpp): three planes of throughput / emission / contrib
// and a per-sample segment count.  With mean_emission enabled the segment max_path_bounces - 1 is marched too: its hit emits, and
// neither next-event estimation nor a bounce follows it.
namespace {
struct PathsRgbState {                 // the path state of the RGB drivers inside the frame's workspace
    size_t o_rng = 0, o_thr = 0, o_em = 0, o_con = 0, o_segs = 0;
    PathsRgbArrays a;
    template <typename Carve>
    void carve(Carve &carve, size_t ns_max)
    {
        o_rng = carve(ns_max * 8); o_thr = carve(ns_max * 12); o_em = carve(ns_max * 12); o_con = carve(ns_max * 12); o_segs = carve(ns_max * 4);
        a.plane = ns_max;
    }
    void bind(const PathsFrame &f)
    {
        a.rays = f.rays; a.seg = f.seg; a.shadow = f.shadow;
        a.rng = (uint64_t *)(f.ws + o_rng);
        a.throughput = (float *)(f.ws + o_thr); a.emission = (float *)(f.ws + o_em); a.contrib = (float *)(f.ws + o_con);
        a.segs = (uint32_t *)(f.ws + o_segs);
        a.alive = f.alive; a.nee = f.nee; a.vis = f.vis;
    }
};
}
extern "C" int gpis_render_scene_s_paths_rgb(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, const float albedo[3], float *radiance_sum3,
                                             uint32_t *seg_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && albedo && radiance_sum3 && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    const bool emissive = m->host_model.emission.enabled != 0;
    PathsRgbState state;
    PathsRgbArrays &a = state.a;
    return lambert_paths_frames(
        m, s, emissive ? max_path_bounces : max_path_bounces - 1, max_path_bounces - 1, st,
        [&](auto &carve, size_t ns_max) { state.carve(carve, ns_max); },
        [&](const PathsFrame &f) { state.bind(f); },
        [&](size_t p0, size_t ns) {
            k_paths_rgb_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, p0, ns, a);
            return launch_check("k_paths_rgb_begin");
        },
        [&](int bounce, size_t ns, const uint32_t *order, const gpis_ray_in *rays_in, const uint8_t *live) {
            k_paths_rgb_shade<0><<<grid_of(ns, 256), 256, 0, st>>>(m->d_model.p, sc, ns, bounce, max_path_bounces, emissive ? 1 : 0, albedo[0], albedo[1],
                                                                   albedo[2], a, order, rays_in, live);
            return launch_check("k_paths_rgb_shade");
        },
        [&](size_t ns, const uint32_t *order, const uint32_t *order2, const uint8_t *live2) {
            k_paths_rgb_nee_add<0><<<grid_of(ns, 256), 256, 0, st>>>(ns, a, order, order2, live2, a.vis);
            return launch_check("k_paths_rgb_nee_add");
        },
        [&](size_t p0, size_t np) {
            k_paths_rgb_accumulate<0><<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, a.plane, a.emission, radiance_sum3);
            if (int rc = launch_check("k_paths_rgb_accumulate")) return rc;
            if (!seg_count) return (int)GPIS_OK;
            k_scene_sum_u32<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, a.segs, seg_count);
            return launch_check("k_scene_sum_u32");
        });
}

// gpis_render_scene_s_paths_rgb under the adaptive sample schedule (gpis_adaptive.hpp): the pass loop of
// gpis_render_scene_s_adaptive around the chunk body of the Lambert path drivers.  A chunk of records is seeded through
// scene_sample of its AdaptiveChunk, runs the bounce loop of gpis_render_scene_s_paths_rgb, and ends with the clamped luminance and the clamp
// flag of every sample (4 + 1 bytes per sample behind the path state), the tile statistics on the luminances and the pixel sums.
extern "C" int gpis_render_scene_s_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int max_path_bounces,
                                                      const float albedo[3], float *radiance_sum3, uint32_t *sample_count, uint32_t *seg_count,
                                                      gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && albedo && radiance_sum3 && sample_count && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    const bool emissive = m->host_model.emission.enabled != 0;
    const int n_marched = emissive ? max_path_bounces : max_path_bounces - 1, n_nee = max_path_bounces - 1;
    PathsRgbState state;
    const PathsRgbArrays &arr = state.a;
    size_t o_lum = 0, o_clamped = 0;
    PathsWs W;
    PathsFrame f;
    float *lum = nullptr;
    uint8_t *clamped = nullptr;
    return adaptive_passes(
        MediumPasses{m, 25}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            const int rc = lambert_paths_carve(m, n_marched, n, st,
                                               [&](auto &carve, size_t ns_max) {
                                                   state.carve(carve, ns_max);
                                                   o_lum = carve(ns_max * 4); o_clamped = carve(ns_max);
                                               }, W);
            if (rc) return rc;
            fits = try_stage(m, 3, W.bytes);
            return (int)GPIS_OK;
        },
        [&]() {
            f = lambert_paths_bind(m, W);
            state.bind(f);
            lum = (float *)(f.ws + o_lum); clamped = (uint8_t *)(f.ws + o_clamped);
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            return lambert_paths_chunk(
                m, W, f, ns, n_marched, n_nee, st,
                [&] {
                    k_paths_rgb_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, ch, ns, arr);
                    return launch_check("k_paths_rgb_begin");
                },
                [&](int bounce, size_t n, const uint32_t *order, const gpis_ray_in *rays_in, const uint8_t *live) {
                    k_paths_rgb_shade<0><<<grid_of(n, 256), 256, 0, st>>>(m->d_model.p, sc, n, bounce, max_path_bounces, emissive ? 1 : 0, albedo[0], albedo[1],
                                                                          albedo[2], arr, order, rays_in, live);
                    return launch_check("k_paths_rgb_shade");
                },
                [&](size_t n, const uint32_t *order, const uint32_t *order2, const uint8_t *live2) {
                    k_paths_rgb_nee_add<0><<<grid_of(n, 256), 256, 0, st>>>(n, arr, order, order2, live2, arr.vis);
                    return launch_check("k_paths_rgb_nee_add");
                },
                [&] {
                    k_rgb_adaptive_value<0><<<grid_of(ns, 256), 256, 0, st>>>(ns, arr.plane, arr.emission, lum, clamped);
                    if (int rc = launch_check("k_rgb_adaptive_value")) return rc;
                    k_rgb_adaptive_accumulate<0><<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(
                        sc, ch, arr.plane, arr.emission, clamped, arr.segs, radiance_sum3, sample_count, seg_count);
                    if (int rc = launch_check("k_rgb_adaptive_accumulate")) return rc;
                    k_rgb_adaptive_stats<0><<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, lum, d_records);
                    return launch_check("k_rgb_adaptive_stats");
                });
        });
}

// The two conductor NEE / MIS drivers and the path driver's adaptive form.  max_path_bounces == 0: the single-interaction estimator
// of gpis_render_scene_s_nee; otherwise the bounce loop of gpis_render_scene_s_nee_paths over the same stages.  The workspace layout
// (nee_carve, nee_bind) and the body of one chunk (nee_chunk) are functions of their own, as the Lambert path drivers': the frame
// loop of the uniform entries (nee_frames) and the pass loop of gpis_render_scene_s_nee_paths_adaptive run the same code.
// ≈ 800 B per sample (rays, results, the two query records, two shadow rays, masks; the path driver adds 8 B).
struct NeeWs {
    size_t bytes;                      // of stage[3]
    size_t o_rays, o_seg, o_rng, o_thr, o_em, o_alive, o_coeff, o_qh, o_qn, o_aux, o_shl, o_shp;
    size_t o_ph, o_gh, o_pn, o_cl, o_cp, o_f[7], o_th, o_segs;
    PathArrays a;
    NeeArrays b;
    NeePathArrays c;
};
// the layout of stage[3] for chunks of up to ns_max samples
static void nee_carve(NeeWs &W, size_t ns_max, bool paths, size_t aux_bytes = sizeof(NeeAux))
{
    size_t off = 0;
    auto carve = [&](size_t bytes) { return ws_carve(off, bytes); };
    W.o_rays = carve(ns_max * sizeof(gpis_ray_in)); W.o_seg = carve(ns_max * sizeof(gpis_seg_out));
    W.o_rng = carve(ns_max * 8); W.o_thr = carve(ns_max * 4); W.o_em = carve(ns_max * 4); W.o_alive = carve(ns_max);
    W.o_coeff = carve(ns_max * sizeof(gpis_cond_coeff)); W.o_qh = carve(ns_max * sizeof(gpis_nee_query)); W.o_qn = carve(ns_max * sizeof(gpis_nee_query));
    W.o_aux = carve(ns_max * aux_bytes); W.o_shl = carve(ns_max * sizeof(gpis_ray_in)); W.o_shp = carve(ns_max * sizeof(gpis_ray_in));
    W.o_ph = carve(ns_max * 4); W.o_gh = carve(ns_max * 12); W.o_pn = carve(ns_max * 4); W.o_cl = carve(ns_max * 4); W.o_cp = carve(ns_max * 4);
    for (int k = 0; k < 7; ++k) W.o_f[k] = carve(ns_max);
    W.o_th = W.o_segs = 0;
    if (paths) { W.o_th = carve(ns_max * 4); W.o_segs = carve(ns_max * 4); }
    W.bytes = off;
}
// the arrays in stage[3], which holds W.bytes
static void nee_bind(gpis_medium *m, NeeWs &W)
{
    char *ws = (char *)m->stage[3].p;
    PathArrays &a = W.a;
    NeeArrays &b = W.b;
    NeePathArrays &c = W.c;
    a.rays = (gpis_ray_in *)(ws + W.o_rays); a.seg = (gpis_seg_out *)(ws + W.o_seg); a.shadow = nullptr;
    a.rng = (uint64_t *)(ws + W.o_rng); a.throughput = (float *)(ws + W.o_thr); a.emission = (float *)(ws + W.o_em); a.contrib = nullptr;
    a.alive = (uint8_t *)(ws + W.o_alive); a.nee = nullptr; a.vis = nullptr;
    b.coeff = (gpis_cond_coeff *)(ws + W.o_coeff); b.q_half = (gpis_nee_query *)(ws + W.o_qh); b.q_normal = (gpis_nee_query *)(ws + W.o_qn);
    b.aux = (NeeAux *)(ws + W.o_aux); b.shadow_light = (gpis_ray_in *)(ws + W.o_shl); b.shadow_phase = (gpis_ray_in *)(ws + W.o_shp);
    b.pdf_half = (float *)(ws + W.o_ph); b.grad_half = (float *)(ws + W.o_gh); b.pdf_normal = (float *)(ws + W.o_pn);
    b.contrib_light = (float *)(ws + W.o_cl); b.contrib_phase = (float *)(ws + W.o_cp);
    b.want_light = (uint8_t *)(ws + W.o_f[0]); b.want_phase = (uint8_t *)(ws + W.o_f[1]); b.want_pdf_normal = (uint8_t *)(ws + W.o_f[2]);
    b.go_light = (uint8_t *)(ws + W.o_f[3]); b.go_phase = (uint8_t *)(ws + W.o_f[4]); b.vis_light = (uint8_t *)(ws + W.o_f[5]); b.vis_phase = (uint8_t *)(ws + W.o_f[6]);
    c.thr_hit = (float *)(ws + W.o_th); c.segs = (uint32_t *)(ws + W.o_segs);
}
// the light and the phase estimator of the hits of one march: neePDF / neeGrad between set-up and shade, then the shadow marches
static int nee_queries(gpis_medium *m, const NeeArrays &b, size_t ns, hipStream_t st)
{
    ProfScope prof(m, 2, st);
    launch::nee(nee_instance(m->host_model), m->d_model.p, ns, b.q_half, b.pdf_half, b.grad_half, m->d_counters.p, b.want_light, st);
    if (int r = launch_check("k_nee")) return r;
    launch::nee(nee_instance(m->host_model), m->d_model.p, ns, b.q_normal, b.pdf_normal, nullptr, m->d_counters.p, b.want_pdf_normal, st);
    return launch_check("k_nee");
}
static int nee_shadow_marches(gpis_medium *m, const NeeArrays &b, size_t ns, hipStream_t st, int hint)
{
    if (int r = transmittance_impl(m, ns, b.shadow_light, b.vis_light, b.go_light, st, hint)) return r;
    return transmittance_impl(m, ns, b.shadow_phase, b.vis_phase, b.go_phase, st, hint);
}
// One chunk of ns samples: `begin` (the driver's camera step), the estimator of one hit or the bounce loop, `finish` (its sums).
// Each callback launches and returns its launch_check.
template <typename Begin, typename Finish>
static int nee_chunk(gpis_medium *m, const SceneConst &sc, const gpis_surface_s *surf, const NeeWs &W, size_t ns, int max_path_bounces, hipStream_t st,
                     Begin begin, Finish finish)
{
    const bool paths = max_path_bounces > 0;
    const PathArrays &a = W.a;
    const NeeArrays &b = W.b;
    const NeePathArrays &c = W.c;
    int rc = GPIS_OK;
    if ((rc = begin())) return rc;
    if (!paths) {
        if ((rc = sample_distance_impl(m, ns, a.rays, a.seg, b.coeff, a.alive, st))) return rc;
        k_nee_setup<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, a, b);
        if ((rc = launch_check("k_nee_setup"))) return rc;
        if ((rc = nee_queries(m, b, ns, st))) return rc;
        k_nee_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, a, b);
        if ((rc = launch_check("k_nee_shade"))) return rc;
        if ((rc = nee_shadow_marches(m, b, ns, st, MARCH_COHERENT))) return rc;
        k_nee_gather<<<grid_of(ns, 256), 256, 0, st>>>(surf->cap_radiance, ns, a, b);
        if ((rc = launch_check("k_nee_gather"))) return rc;
    } else {
        HIP_TRY(hipMemsetAsync(c.segs, 0, ns * sizeof(uint32_t), st));
        // the segment of bounce max-1 cannot contribute (no direct lighting there, TraceBase.cpp:546, and the light seen directly is
        // never added), so it is not marched.  Dead paths stay masked in sample order; the segments after the first are scattered.
        for (int bounce = 0; bounce + 1 < max_path_bounces; ++bounce) {
            const int hint = bounce > 0 ? MARCH_SCATTERED : MARCH_COHERENT;
            if ((rc = sample_distance_impl(m, ns, a.rays, a.seg, b.coeff, a.alive, st, hint))) return rc;
            k_nee_paths_setup<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, a, b, c);
            if ((rc = launch_check("k_nee_paths_setup"))) return rc;
            if ((rc = nee_queries(m, b, ns, st))) return rc;
            k_nee_paths_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, bounce, max_path_bounces, a, b, c);
            if ((rc = launch_check("k_nee_paths_shade"))) return rc;
            if ((rc = nee_shadow_marches(m, b, ns, st, hint))) return rc;
            k_nee_paths_gather<<<grid_of(ns, 256), 256, 0, st>>>(surf->cap_radiance, ns, a, b, c);
            if ((rc = launch_check("k_nee_paths_gather"))) return rc;
        }
    }
    return finish();
}
// The frames of the two uniform entries: the largest chunk the device can hold, starting from the whole frame (2^27 samples ≈ 106 GB
// for C2's 1920x1080x64) — every launch ends in a tail of half-empty waves.
static int nee_frames(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_s *surf, int max_path_bounces, float *radiance_sum, uint32_t *seg_count,
                      hipStream_t st)
{
    const bool paths = max_path_bounces > 0;
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    NeeWs W;
    size_t chunk_pixels = 0;
    int rc = GPIS_OK;
    for (int l = chunk_log2(m, 27);; --l) {
        chunk_pixels = chunk_pixels_of(l, s->spp_count, total_pixels);
        nee_carve(W, chunk_pixels * s->spp_count, paths);
        if (try_stage(m, 3, W.bytes))
            break;
        if (l <= 20) return set_err(GPIS_ERR_DEVICE, "NEE driver: no memory for a 1 Mi-sample workspace");
    }
    if ((rc = ws_acquire(m, 0, st))) return rc;
    nee_bind(m, W);
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        size_t ns = np * s->spp_count;
        rc = nee_chunk(
            m, sc, surf, W, ns, max_path_bounces, st,
            [&] {
                k_paths_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, p0, ns, W.a);
                return launch_check("k_paths_begin");
            },
            [&] {
                if (paths && seg_count) {
                    k_scene_sum_u32<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.c.segs, seg_count);
                    if (int r = launch_check("k_scene_sum_u32")) return r;
                }
                k_paths_accumulate<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.a.emission, radiance_sum);
                return launch_check("k_paths_accumulate");
            });
        if (rc) return rc;
    }
    return ws_release(m, 0, st);
}

extern "C" int gpis_render_scene_s_nee(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_s *surf, float *radiance_sum, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && surf && radiance_sum);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(surf->cap_cos < 1.0f && surf->cap_cos > -1.0f);
    return nee_frames(m, s, surf, 0, radiance_sum, nullptr, (hipStream_t)stream);
}

extern "C" int gpis_render_scene_s_nee_paths(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_s *surf, int max_path_bounces, float *radiance_sum,
                                             uint32_t *seg_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && surf && radiance_sum && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(surf->cap_cos < 1.0f && surf->cap_cos > -1.0f);
    return nee_frames(m, s, surf, max_path_bounces, radiance_sum, seg_count, (hipStream_t)stream);
}

// gpis_render_scene_s_nee_paths under the adaptive sample schedule: the pass loop of gpis_render_scene_s_adaptive around nee_chunk.
// A chunk of records is seeded through scene_sample of its AdaptiveChunk, runs the bounce loop of gpis_render_scene_s_nee_paths, and
// ends with the pixel sums and the tile statistics on the clamped E of every sample.
extern "C" int gpis_render_scene_s_nee_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, const gpis_surface_s *surf,
                                                      int max_path_bounces, float *radiance_sum, uint32_t *sample_count, uint32_t *seg_count,
                                                      gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && surf && radiance_sum && sample_count && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(surf->cap_cos < 1.0f && surf->cap_cos > -1.0f);
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    NeeWs W;
    return adaptive_passes(
        MediumPasses{m, 27}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            nee_carve(W, n, true);
            fits = try_stage(m, 3, W.bytes);
            return (int)GPIS_OK;
        },
        [&]() {
            nee_bind(m, W);
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            return nee_chunk(
                m, sc, surf, W, ns, max_path_bounces, st,
                [&] {
                    k_paths_adaptive_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, ch, ns, W.a);
                    return launch_check("k_paths_adaptive_begin");
                },
                [&] { return paths_adaptive_finish(sc, ch, st, W.a.emission, W.c.segs, radiance_sum, sample_count, seg_count, d_records); });
        });
}

// ---- the conductor NEE / MIS path driver in RGB and its adaptive form.  The workspace is NeeWs's layout (its aux slots sized for
// NeeAuxN<3>) followed by the colour planes of thr, thr_hit, em, contrib_light and contrib_phase (60 B per sample), on an emissive
// medium the points, values and mask of the emission (37 B) and, for the adaptive entry, the clamped luminance and the clamp flag
// of gpis_render_scene_s_paths_rgb_adaptive; the chunk body mirrors the path branch of nee_chunk around the kernels of
// gpis_cond_rgb.hpp.
struct CondRgbWs {
    NeeWs nee;
    size_t bytes;                      // of stage[3]
    size_t o_thr, o_th, o_em, o_cl, o_cp, o_points, o_e3, o_emit, o_lum, o_clamped;
    CondRgbArrays r;
    float *lum;                        // adaptive entry only
    uint8_t *clamped;
};
static void cond_rgb_carve(CondRgbWs &W, size_t ns_max, bool emissive, bool adaptive, size_t aux_bytes = sizeof(NeeAuxN<3>))
{
    nee_carve(W.nee, ns_max, true, aux_bytes);
    size_t off = W.nee.bytes;
    auto carve = [&](size_t bytes) { return ws_carve(off, bytes); };
    W.o_thr = carve(ns_max * 12); W.o_th = carve(ns_max * 12); W.o_em = carve(ns_max * 12); W.o_cl = carve(ns_max * 12); W.o_cp = carve(ns_max * 12);
    W.o_points = W.o_e3 = W.o_emit = W.o_lum = W.o_clamped = 0;
    if (emissive) { W.o_points = carve(ns_max * 24); W.o_e3 = carve(ns_max * 12); W.o_emit = carve(ns_max); }
    if (adaptive) { W.o_lum = carve(ns_max * 4); W.o_clamped = carve(ns_max); }
    W.r.plane = ns_max;
    W.bytes = off;
}
static void cond_rgb_bind(gpis_medium *m, CondRgbWs &W)
{
    nee_bind(m, W.nee);
    char *ws = (char *)m->stage[3].p;
    CondRgbArrays &r = W.r;
    r.thr = (float *)(ws + W.o_thr); r.thr_hit = (float *)(ws + W.o_th); r.em = (float *)(ws + W.o_em);
    r.contrib_light = (float *)(ws + W.o_cl); r.contrib_phase = (float *)(ws + W.o_cp);
    r.aux = (NeeAuxN<3> *)(ws + W.nee.o_aux);
    r.points = (double *)(ws + W.o_points); r.e3 = (float *)(ws + W.o_e3); r.emit = (uint8_t *)(ws + W.o_emit);
    W.lum = (float *)(ws + W.o_lum); W.clamped = (uint8_t *)(ws + W.o_clamped);
}
// One chunk of ns samples: `begin` (the camera step on W.nee.a), the bounce loop, `finish` (the driver's sums over W.r.em and
// W.nee.c.segs).  On an emissive medium the segment of bounce max-1 is marched too: its hit can only emit.
template <typename Begin, typename Finish>
static int cond_rgb_chunk(gpis_medium *m, const SceneConst &sc, const gpis_surface_rgb_s *surf, const CondRgbWs &W, size_t ns, int max_path_bounces,
                          hipStream_t st, Begin begin, Finish finish)
{
    const PathArrays &a = W.nee.a;
    const NeeArrays &b = W.nee.b;
    const NeePathArrays &c = W.nee.c;
    const CondRgbArrays &r = W.r;
    const int emissive = m->host_model.emission.enabled != 0 ? 1 : 0;
    const int n_marched = emissive ? max_path_bounces : max_path_bounces - 1;
    int rc = GPIS_OK;
    if ((rc = begin())) return rc;
    HIP_TRY(hipMemsetAsync(c.segs, 0, ns * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(r.em, 0, 3 * r.plane * sizeof(float), st));
    for (int bounce = 0; bounce < n_marched; ++bounce) {
        const int hint = bounce > 0 ? MARCH_SCATTERED : MARCH_COHERENT;
        if ((rc = sample_distance_impl(m, ns, a.rays, a.seg, b.coeff, a.alive, st, hint))) return rc;
        k_cond_rgb_setup<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, bounce, max_path_bounces, emissive, a, b, c, r);
        if ((rc = launch_check("k_cond_rgb_setup"))) return rc;
        if (emissive) {
            if ((rc = gpis_mean_color_emission_batch(m, ns, r.points, nullptr, r.e3, st))) return rc;
            k_cond_rgb_emit<<<grid_of(ns, 256), 256, 0, st>>>(ns, bounce, r);
            if ((rc = launch_check("k_cond_rgb_emit"))) return rc;
        }
        if (bounce + 1 >= max_path_bounces) break;      // the extra last segment: no estimator and no bounce follow it
        if ((rc = nee_queries(m, b, ns, st))) return rc;
        k_cond_rgb_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, *surf, ns, bounce, n_marched, a, b, c, r);
        if ((rc = launch_check("k_cond_rgb_shade"))) return rc;
        if ((rc = nee_shadow_marches(m, b, ns, st, hint))) return rc;
        k_cond_rgb_gather<<<grid_of(ns, 256), 256, 0, st>>>(surf->cap_radiance[0], surf->cap_radiance[1], surf->cap_radiance[2], ns, b, r);
        if ((rc = launch_check("k_cond_rgb_gather"))) return rc;
    }
    return finish();
}

extern "C" void gpis_default_surface_rgb(gpis_surface_rgb_s *surf)
{
    memset(surf, 0, sizeof *surf);
    const float eta[3] = {0.200438f, 0.924033f, 1.10221f}, k[3] = {3.91295f, 2.45285f, 2.14219f};     // ConductorBsdf.cpp:24-28: "Cu"
    for (int c = 0; c < 3; ++c) {
        surf->eta[c] = eta[c]; surf->k[c] = k[c];
        surf->albedo[c] = 1.0f; surf->cap_radiance[c] = 1.0f;
    }
    surf->cap_cos = 0.9781476f;
}

extern "C" int gpis_render_scene_s_nee_paths_rgb(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_rgb_s *surf, int max_path_bounces,
                                                 float *radiance_sum3, uint32_t *seg_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && surf && radiance_sum3 && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(surf->cap_cos < 1.0f && surf->cap_cos > -1.0f);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    const SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    CondRgbWs W;
    size_t chunk_pixels = 0;
    int rc = GPIS_OK;
    for (int l = chunk_log2(m, 27);; --l) {        // the chunks of gpis_render_scene_s_nee_paths (nee_frames)
        chunk_pixels = chunk_pixels_of(l, s->spp_count, total_pixels);
        cond_rgb_carve(W, chunk_pixels * s->spp_count, m->host_model.emission.enabled != 0, false);
        if (try_stage(m, 3, W.bytes))
            break;
        if (l <= 20) return set_err(GPIS_ERR_DEVICE, "NEE driver: no memory for a 1 Mi-sample workspace");
    }
    if ((rc = ws_acquire(m, 0, st))) return rc;
    cond_rgb_bind(m, W);
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        rc = cond_rgb_chunk(
            m, sc, surf, W, ns, max_path_bounces, st,
            [&] {
                k_paths_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, p0, ns, W.nee.a);
                return launch_check("k_paths_begin");
            },
            [&] {
                if (seg_count) {
                    k_scene_sum_u32<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.nee.c.segs, seg_count);
                    if (int r = launch_check("k_scene_sum_u32")) return r;
                }
                k_paths_rgb_accumulate<0><<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.r.plane, W.r.em, radiance_sum3);
                return launch_check("k_paths_rgb_accumulate");
            });
        if (rc) return rc;
    }
    return ws_release(m, 0, st);
}

extern "C" int gpis_render_scene_s_nee_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, const gpis_surface_rgb_s *surf,
                                                          int max_path_bounces, float *radiance_sum3, uint32_t *sample_count, uint32_t *seg_count,
                                                          gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && surf && radiance_sum3 && sample_count && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(surf->cap_cos < 1.0f && surf->cap_cos > -1.0f);
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    CondRgbWs W;
    return adaptive_passes(
        MediumPasses{m, 27}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            cond_rgb_carve(W, n, m->host_model.emission.enabled != 0, true);
            fits = try_stage(m, 3, W.bytes);
            return (int)GPIS_OK;
        },
        [&]() {
            cond_rgb_bind(m, W);
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            return cond_rgb_chunk(
                m, sc, surf, W, ns, max_path_bounces, st,
                [&] {
                    k_paths_adaptive_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, ch, ns, W.nee.a);
                    return launch_check("k_paths_adaptive_begin");
                },
                [&] {
                    k_rgb_adaptive_value<0><<<grid_of(ns, 256), 256, 0, st>>>(ns, W.r.plane, W.r.em, W.lum, W.clamped);
                    if (int rc = launch_check("k_rgb_adaptive_value")) return rc;
                    k_rgb_adaptive_accumulate<0><<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(
                        sc, ch, W.r.plane, W.r.em, W.clamped, W.nee.c.segs, radiance_sum3, sample_count, seg_count);
                    if (int rc = launch_check("k_rgb_adaptive_accumulate")) return rc;
                    k_rgb_adaptive_stats<0><<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, W.lum, d_records);
                    return launch_check("k_rgb_adaptive_stats");
                });
        });
}

// ---- materials chosen by GP id: the RGB conductor driver's workspace (its aux slots sized for MatAux) and its chunk body around
// k_mat_rgb_setup / k_mat_rgb_shade; the emission add and the gather are the conductor driver's kernels.
static void mat_rgb_carve(CondRgbWs &W, size_t ns_max, bool emissive, bool adaptive)
{
    cond_rgb_carve(W, ns_max, emissive, adaptive, sizeof(MatAux));
}
template <typename Begin, typename Finish>
static int mat_rgb_chunk(gpis_medium *m, const SceneConst &sc, const gpis_materials_s *mats, const CondRgbWs &W, size_t ns, int max_path_bounces,
                         hipStream_t st, Begin begin, Finish finish)
{
    const PathArrays &a = W.nee.a;
    const NeeArrays &b = W.nee.b;
    const NeePathArrays &c = W.nee.c;
    const CondRgbArrays &r = W.r;
    MatAux *aux = (MatAux *)r.aux;
    const int emissive = m->host_model.emission.enabled != 0 ? 1 : 0;
    const int n_marched = emissive ? max_path_bounces : max_path_bounces - 1;
    int rc = GPIS_OK;
    if ((rc = begin())) return rc;
    HIP_TRY(hipMemsetAsync(c.segs, 0, ns * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(r.em, 0, 3 * r.plane * sizeof(float), st));
    for (int bounce = 0; bounce < n_marched; ++bounce) {
        const int hint = bounce > 0 ? MARCH_SCATTERED : MARCH_COHERENT;
        if ((rc = sample_distance_impl(m, ns, a.rays, a.seg, b.coeff, a.alive, st, hint))) return rc;
        k_mat_rgb_setup<<<grid_of(ns, 256), 256, 0, st>>>(sc, *mats, ns, bounce, max_path_bounces, emissive, a, b, c, r, aux);
        if ((rc = launch_check("k_mat_rgb_setup"))) return rc;
        if (emissive) {
            if ((rc = gpis_mean_color_emission_batch(m, ns, r.points, nullptr, r.e3, st))) return rc;
            k_cond_rgb_emit<<<grid_of(ns, 256), 256, 0, st>>>(ns, bounce, r);
            if ((rc = launch_check("k_cond_rgb_emit"))) return rc;
        }
        if (bounce + 1 >= max_path_bounces) break;      // the extra last segment: no estimator and no bounce follow it
        if ((rc = nee_queries(m, b, ns, st))) return rc;
        k_mat_rgb_shade<<<grid_of(ns, 256), 256, 0, st>>>(sc, *mats, ns, bounce, n_marched, a, b, c, r, aux);
        if ((rc = launch_check("k_mat_rgb_shade"))) return rc;
        if ((rc = nee_shadow_marches(m, b, ns, st, hint))) return rc;
        k_cond_rgb_gather<<<grid_of(ns, 256), 256, 0, st>>>(mats->cap_radiance[0], mats->cap_radiance[1], mats->cap_radiance[2], ns, b, r);
        if ((rc = launch_check("k_cond_rgb_gather"))) return rc;
    }
    return finish();
}

extern "C" void gpis_default_materials(gpis_materials_s *mats)
{
    memset(mats, 0, sizeof *mats);
    gpis_surface_rgb_s cu;
    gpis_default_surface_rgb(&cu);
    mats->n_materials = 2;
    mats->cap_cos = cu.cap_cos;
    mats->material[0].type = GPIS_MATERIAL_CONDUCTOR;
    mats->material[1].type = GPIS_MATERIAL_LAMBERT;
    for (int c = 0; c < 3; ++c) {
        mats->cap_radiance[c] = cu.cap_radiance[c];
        mats->material[0].eta[c] = cu.eta[c]; mats->material[0].k[c] = cu.k[c]; mats->material[0].albedo[c] = cu.albedo[c];
        mats->material[1].albedo[c] = 0.8f;
    }
}

static bool materials_ok(const gpis_materials_s *mats)
{
    if (!mats || mats->n_materials < 1 || mats->n_materials > GPIS_MAX_MATERIALS) return false;
    for (uint32_t k = 0; k < mats->n_materials; ++k)
        if (mats->material[k].type != GPIS_MATERIAL_CONDUCTOR && mats->material[k].type != GPIS_MATERIAL_LAMBERT) return false;
    return mats->cap_cos < 1.0f && mats->cap_cos > -1.0f;
}

extern "C" int gpis_render_scene_s_material_paths_rgb(gpis_medium *m, const gpis_scene_s *s, const gpis_materials_s *mats, int max_path_bounces,
                                                      float *radiance_sum3, uint32_t *seg_count, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && radiance_sum3 && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(materials_ok(mats));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    const SceneConst sc = make_scene_const(s);
    const size_t total_pixels = scene_rows(*s) * s->width;
    CondRgbWs W;
    size_t chunk_pixels = 0;
    int rc = GPIS_OK;
    for (int l = chunk_log2(m, 27);; --l) {        // the chunks of gpis_render_scene_s_nee_paths_rgb
        chunk_pixels = chunk_pixels_of(l, s->spp_count, total_pixels);
        mat_rgb_carve(W, chunk_pixels * s->spp_count, m->host_model.emission.enabled != 0, false);
        if (try_stage(m, 3, W.bytes))
            break;
        if (l <= 20) return set_err(GPIS_ERR_DEVICE, "material driver: no memory for a 1 Mi-sample workspace");
    }
    if ((rc = ws_acquire(m, 0, st))) return rc;
    cond_rgb_bind(m, W);
    for (size_t p0 = 0; p0 < total_pixels; p0 += chunk_pixels) {
        const size_t np = total_pixels - p0 < chunk_pixels ? total_pixels - p0 : chunk_pixels;
        const size_t ns = np * s->spp_count;
        rc = mat_rgb_chunk(
            m, sc, mats, W, ns, max_path_bounces, st,
            [&] {
                k_paths_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, p0, ns, W.nee.a);
                return launch_check("k_paths_begin");
            },
            [&] {
                if (seg_count) {
                    k_scene_sum_u32<<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.nee.c.segs, seg_count);
                    if (int r = launch_check("k_scene_sum_u32")) return r;
                }
                k_paths_rgb_accumulate<0><<<grid_of(np, 256), 256, 0, st>>>(sc, p0, np, W.r.plane, W.r.em, radiance_sum3);
                return launch_check("k_paths_rgb_accumulate");
            });
        if (rc) return rc;
    }
    return ws_release(m, 0, st);
}

extern "C" int gpis_render_scene_s_material_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                               const gpis_materials_s *mats, int max_path_bounces, float *radiance_sum3,
                                                               uint32_t *sample_count, uint32_t *seg_count, gpis_adaptive_record *records,
                                                               gpis_adaptive_info *info, void *stream)
{
    CHECK_ARGS(std_handle(m) && s && a && radiance_sum3 && sample_count && max_path_bounces >= 1);
    CHECK_ARGS(scene_args_ok(s));
    CHECK_ARGS(materials_ok(mats));
    hipStream_t st = (hipStream_t)stream;
    const SceneConst sc = make_scene_const(s);
    CondRgbWs W;
    return adaptive_passes(
        MediumPasses{m, 27}, s, a, __func__, st, records, info,
        [&](size_t n, bool &fits) {
            mat_rgb_carve(W, n, m->host_model.emission.enabled != 0, true);
            fits = try_stage(m, 3, W.bytes);
            return (int)GPIS_OK;
        },
        [&]() {
            cond_rgb_bind(m, W);
            return (int)GPIS_OK;
        },
        [&](const AdaptiveChunk &ch, size_t ns, gpis_adaptive_record *d_records) {
            return mat_rgb_chunk(
                m, sc, mats, W, ns, max_path_bounces, st,
                [&] {
                    k_paths_adaptive_begin<<<grid_of(ns, 256), 256, 0, st>>>(sc, ch, ns, W.nee.a);
                    return launch_check("k_paths_adaptive_begin");
                },
                [&] {
                    k_rgb_adaptive_value<0><<<grid_of(ns, 256), 256, 0, st>>>(ns, W.r.plane, W.r.em, W.lum, W.clamped);
                    if (int rc = launch_check("k_rgb_adaptive_value")) return rc;
                    k_rgb_adaptive_accumulate<0><<<grid_of((size_t)ch.nrec * (kVarianceTile * kVarianceTile), 256), 256, 0, st>>>(
                        sc, ch, W.r.plane, W.r.em, W.clamped, W.nee.c.segs, radiance_sum3, sample_count, seg_count);
                    if (int rc = launch_check("k_rgb_adaptive_accumulate")) return rc;
                    k_rgb_adaptive_stats<0><<<grid_of(ch.nrec, 256), 256, 0, st>>>(ch, W.lum, d_records);
                    return launch_check("k_rgb_adaptive_stats");
                });
        });
}
