// gpis_paths_rgb.hpp — the per-bounce kernels of gpis_render_scene_s_paths_rgb: the Lambert multi-bounce estimator of
// gpis_render_scene_s_paths (tu_scene.hip, which instantiates these kernels too: k_paths_begin, k_paths_shade, k_paths_nee_add, k_paths_accumulate) carried in RGB, with
// the medium's emission (MediumSample.emission, GPM.cpp:317; PathTracer.cpp:72-73: emission += throughput * sample.emission, then
// throughput *= sample.weight).
//
// The march kernels, the regrouping (k_paths_keys, k_paths_gather) and the host loop are the mono driver's; only the small
// kernels between the medium's launches are new.  One thread per sample (per pixel in the sum), 256 threads per workgroup,
// no LDS.  Path state is SoA: throughput, emission and contrib are THREE PLANES each of `plane` floats (channel c of sample i at
// [c * plane + i]), so that a wave's 64 lanes read and write 256 contiguous bytes per channel exactly as the mono driver's single
// plane does; interleaved float3 would make every access a 12-byte stride.
//
// Per bounce the order of additions into a sample's emission is: the hit's own emission (thr BEFORE the segment's weight, the
// product rounded to float on its own: contraction is off in this file), then, after the shadow march, the NEE term.  The fp64 fbm
// behind field_vec (sandstone / rust emission) is reached only by the lanes that hit: dead slots, !ok and exited segments return
// before it.
#pragma once
#include "gpis_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

struct PathsRgbArrays {                // path state of one chunk, SoA; `plane` floats per channel plane
    gpis_ray_in *rays;                 // current segment of every path (rewritten in place at each bounce)
    gpis_seg_out *seg;
    gpis_ray_in *shadow;
    uint64_t *rng;                     // PCG32 state of the sample's stream
    float *throughput, *emission;      // 3 planes each, indexed by path
    float *contrib;                    // 3 planes, indexed by batch slot
    uint32_t *segs;                    // segments marched for the sample, path plus shadow (per pixel: k_scene_sum_u32)
    uint8_t *alive, *nee, *vis;
    size_t plane;
};

// The camera step: the path state of slot i.  `where` is the sample layout scene_sample takes: size_t, the first pixel of a chunk
// with spp_count samples per pixel, or AdaptiveChunk (gpis_adaptive.hpp).
template <typename Where>
__global__ void __launch_bounds__(256) k_paths_rgb_begin(SceneConst sc, Where where, size_t n_samples, PathsRgbArrays a)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint32_t x, y, spp;
    Pcg32 g = scene_sample(sc, where, i, x, y, spp);
    float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
    float u0 = normalized_uint(g.next_i());
    gpis_ray_in r;
    bool hit = scene_camera_ray(sc, x, y, spp, jx, jy, r);
    r.u_jitter = u0;
    a.rays[i] = r;
    a.rng[i] = g.state;
    for (int c = 0; c < 3; ++c) {
        a.throughput[c * a.plane + i] = 1.f;
        a.emission[c * a.plane + i] = 0.f;
    }
    a.segs[i] = 0;
    a.alive[i] = hit ? 1 : 0;
}

// After sampleDistance of segment `bounce`: the hit's emission, the throughput, and for bounce < max_bounces - 1 the next-event
// set-up and the bounce of k_paths_shade (same conditions, draws and order of draws).  `emissive`: the medium's mean_emission is
// enabled; the host then marches the segment max_bounces - 1 too, which ends here after its emission term.
// Slot j of the batch (seg, shadow, nee, contrib, and rays_in) belongs to path i = order[j] (identity when order is null); the
// path state (rng, throughput, emission, segs, alive, next ray) is indexed by i.
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_paths_rgb_shade(const DevModel *__restrict__ Mp, SceneConst sc, size_t n_samples, int bounce,
                                                                        int max_bounces, int emissive, float alb0, float alb1, float alb2,
                                                                        PathsRgbArrays a, const uint32_t *__restrict__ order,
                                                                        const gpis_ray_in *__restrict__ rays_in, const uint8_t *__restrict__ live)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_samples) return;
    uint8_t nee = 0;
    if (live ? !live[j] : !a.alive[j]) { a.nee[j] = 0; return; }
    const size_t i = order ? (size_t)order[j] : j;
    a.segs[i] += 1;
    const gpis_seg_out o = a.seg[j];
    if (!o.ok) { a.alive[i] = 0; a.nee[j] = 0; return; }
    const float albedo[3] = {alb0, alb1, alb2};
    float thr[3];
    for (int c = 0; c < 3; ++c) thr[c] = a.throughput[c * a.plane + i];
    if (o.exited) {
        a.alive[i] = 0; a.nee[j] = 0;
        for (int c = 0; c < 3; ++c) a.throughput[c * a.plane + i] = thr[c] * o.weight[c];
        return;
    }
    const gpis_ray_in ray = rays_in[j];
    const V3 dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
    if (emissive) {
        // emission(ro + rd * t): the point of GPM.cpp:317 and of gpis_mean_color_emission_*
        V3d rd = to_d(dir);
        { double inv = 1.0 / length_d(rd); rd.x *= inv; rd.y *= inv; rd.z *= inv; }
        double e[3] = {0., 0., 0.};
        field_vec(Mp->emission, ray_at(to_d(v3(ray.pos[0], ray.pos[1], ray.pos[2])), rd, o.t), true, e);
        for (int c = 0; c < 3; ++c) {
            const float prod = thr[c] * (float)e[c];
            a.emission[c * a.plane + i] = a.emission[c * a.plane + i] + prod;
        }
    }
    for (int c = 0; c < 3; ++c) thr[c] = thr[c] * o.weight[c];
    if (bounce >= max_bounces - 1) {         // the extra last segment of an emissive medium: no NEE and no bounce follow it
        a.alive[i] = 0; a.nee[j] = 0;
        for (int c = 0; c < 3; ++c) a.throughput[c * a.plane + i] = thr[c];
        return;
    }
    Pcg32 g;
    g.state = a.rng[i];
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    const V3 n = hit_normal(o);
    const Frame fr = frame_from_normal(n);
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
    const V3 wo = normalized(to_local(fr, l));
    if (wi.z > 0.0f && wo.z > 0.0f) {
        float t0, t1;
        if (sphere_chord(p, l, sc.s.bound_radius, t0, t1)) {
            gpis_ray_in sh = next;
            sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
            sh.far_t = t1;
            sh.segment = (uint32_t)bounce + 1;
            sh.u_jitter = normalized_uint(g.next_i());
            a.shadow[j] = sh;
            for (int c = 0; c < 3; ++c) {
                const float f = albedo[c] * (1.0f / 3.1415926536f) * wo.z;
                a.contrib[c * a.plane + j] = thr[c] * (f * sc.s.light_radiance);
            }
            a.segs[i] += 1;
            nee = 1;
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
        for (int c = 0; c < 3; ++c) thr[c] *= albedo[c];
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
    for (int c = 0; c < 3; ++c) a.throughput[c * a.plane + i] = thr[c];
    a.rng[i] = g.state;
}

// slot k of the (possibly regrouped) shadow batch -> slot j of the bounce batch -> path i
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_paths_rgb_nee_add(size_t n_samples, PathsRgbArrays a, const uint32_t *__restrict__ order,
                                                                          const uint32_t *__restrict__ shadow_order,
                                                                          const uint8_t *__restrict__ shadow_live, const uint8_t *__restrict__ vis)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_samples) return;
    if (shadow_order ? !shadow_live[k] : !a.nee[k]) return;
    const size_t j = shadow_order ? (size_t)shadow_order[k] : k;
    const size_t i = order ? (size_t)order[j] : j;
    const bool v = vis[k] != 0;
    for (int c = 0; c < 3; ++c)
        a.emission[c * a.plane + i] += v ? a.contrib[c * a.plane + j] : 0.f;
}

// one lane per pixel: per channel the sequential sum over its samples' emissions, in sample order (k_paths_accumulate's sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_paths_rgb_accumulate(SceneConst sc, size_t first_pixel, size_t n_pixels, size_t plane,
                                                                             const float *__restrict__ emission, float *__restrict__ radiance_sum3)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pixels) return;
    const uint32_t spp = sc.s.spp_count;
    float acc[3] = {0.f, 0.f, 0.f};
    for (uint32_t k = 0; k < spp; ++k)
        for (int c = 0; c < 3; ++c)
            acc[c] += emission[c * plane + j * spp + k];
    const size_t pix = scene_pixel(sc.s, first_pixel + j);
    for (int c = 0; c < 3; ++c)
        radiance_sum3[3 * pix + c] += acc[c];
}

}   // namespace gpis
