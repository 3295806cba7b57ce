// gpis_fs_scene.hpp — scene S rendered through the function-space GP medium: one fused kernel, one wave per sample.
//
// The estimator is gpis_render_scene_s's (gpis_hip.hip: k_scene_primary, k_scene_shade, k_scene_accumulate) and the frame has
// the shape of the weight-space one (gpis_ws_scene.hpp): camera ray, bounding-sphere chord, a primary sampleDistance, Lambert
// shading against the directional light, one shadow transmittance per lit hit, one 8-byte record per sample and a per-pixel sum
// of the records in sample order, so the image depends neither on the order in which workgroups finish nor on how a frame is cut
// into calls.  What is this medium's own:
//   one sampler — the path's PCG32 stream gives jx, jy and then EVERY variate of the medium (the reference's medium draws from
//       the path's PathSampleGenerator); no u_march / u_shadow is drawn, and the shadow segment continues the stream where the
//       primary segment stopped;
//   one state — a gpis_fs_state is 2 424 B, so a staged frame moves 2.4 KB per sample through device memory and needs a copy
//       of it for the shadow segment.  Here the state lives in ONE slot per resident workgroup, next to its FsGlob: the primary
//       segment starts it empty (has_context = 0), and the shadow segment continues in place from what the primary left —
//       context (points, derivs, values, sampled_grad, is_intersect) and sampler.  Nothing follows the shadow segment in this
//       estimator, so running in place equals running on a copy (where the path goes on after it, the copy is real: k_fs_paths,
//       gpis_fs_paths.hpp, keeps a second slot per workgroup for it);
//   dynamic work fetch — a sample costs nothing (a miss of the bounding sphere) up to tens of eigen-solves (a grazing chord
//       with fs_step_size > 0 and its shadow segment); workgroups take the next sample index from a global counter (one atomic
//       per workgroup per sample) instead of k_fs_march's static stride.
// The march itself is k_fs_march's: fs_sample_distance_one / fs_transmittance_one (gpis_fs.hpp), the same code for both kernels.
#pragma once
#include "gpis_fs.hpp"
#include "gpis_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one sample's contribution: cos(normal, light) * visible, and bit 0 = the primary segment hit the surface (ok && !exited),
// bit 1 = lit (a shadow segment was marched; cv takes part in the pixel's sum)
struct FsSceneRec { float cv; uint32_t flags; };

// grid = the resident set of the function-space workspace (four one-wave workgroups per CU): workspace[blockIdx.x] and
// slots[blockIdx.x] are this workgroup's for the whole launch.  Every value that steers control flow is computed identically by
// all 64 lanes (the sample index is broadcast from lane 0), so every branch around an FS_SYNC is wave-uniform.
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_fs_scene(const DevModel *__restrict__ Mp, SceneConst sc, size_t first_pixel, uint32_t n_samples,
                                                                uint32_t *__restrict__ next, FsSceneRec *__restrict__ recs,
                                                                FsGlob *__restrict__ workspace, gpis_fs_state *__restrict__ slots)
{
    __shared__ FsLds L;
    FsGlob &G = workspace[blockIdx.x];
    gpis_fs_state *st = slots + blockIdx.x;
    const DevModel &M = *Mp;
    const gpis_scene_s &s = sc.s;
    const int lane = (int)threadIdx.x;
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(next, 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_samples) break;
        // ---- k_scene_primary, with the path's sampler in place of the four per-sample draws
        const size_t pix = scene_pixel(s, first_pixel + i / s.spp_count);
        const uint32_t x = (uint32_t)(pix % s.width), y = (uint32_t)(pix / s.width);
        const uint32_t spp = s.spp_begin + i % s.spp_count;
        Pcg32 g;
        g.set_state((uint64_t)(uint32_t)(xxhash32_4(x, y, spp, s.scene_seed) + 1u));
        const float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
        const V3 local = normalized(v3(-1.0f + ((float)x + jx) * 2.0f * sc.psx, sc.ratio - ((float)y + jy) * 2.0f * sc.psx, sc.plane_dist));
        const V3 d = v3(local.x, local.y, -local.z);
        const V3 o = v3(s.cam_pos[0], s.cam_pos[1], s.cam_pos[2]);
        FsSceneRec rec{0.f, 0u};
        float t0 = 0.f, t1 = 0.f;
        if (sphere_chord(o, d, s.bound_radius, t0, t1)) {
            gpis_ray_in ray{};
            ray.pos[0] = o.x; ray.pos[1] = o.y; ray.pos[2] = o.z;
            ray.dir[0] = d.x; ray.dir[1] = d.y; ray.dir[2] = d.z;
            ray.near_t = t0; ray.far_t = t1;
            ray.pixel[0] = x; ray.pixel[1] = y; ray.spp = spp; ray.segment = 0;
            ray.scene_seed = s.scene_seed; ray.info_t = 0.f;
            ray.first_scatter = 1;
            // the empty state of a path's first segment; the slot still holds the previous sample's context
            FS_SYNC();
            if (lane == 0) {
                st->has_context = 0; st->is_intersect = 0; st->n_points = 0; st->n_values = 0;
                st->sampled_grad[0] = 0.; st->sampled_grad[1] = 0.; st->sampled_grad[2] = 0.;
            }
            __threadfence_block();
            FsState state;
            state.first_scatter = ray.first_scatter != 0;
            state.last_gp_id = ray.last_gp_id;
            state.last_aniso = V3d{ray.last_aniso[0], ray.last_aniso[1], ray.last_aniso[2]};
            FS_SYNC();
            const gpis_seg_out r = fs_sample_distance_one(M, L, G, g, &ray, st, state, lane);
            // ---- k_scene_shade
            if (r.ok && !r.exited) {
                rec.flags = 1u;
                const double ax = r.aniso[0], ay = r.aniso[1], az = r.aniso[2];
                const double len = sqrt(ax * ax + ay * ay + az * az);
                const V3 nn = v3((float)(ax / len), (float)(ay / len), (float)(az / len));
                const float c = dot(nn, l);
                float s0, s1;
                if (c > 0.f && sphere_chord(v3(r.p[0], r.p[1], r.p[2]), l, s.bound_radius, s0, s1)) {
                    gpis_ray_in sh{};
                    sh.pos[0] = r.p[0]; sh.pos[1] = r.p[1]; sh.pos[2] = r.p[2];
                    sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                    sh.near_t = 0.f; sh.far_t = s1;
                    sh.pixel[0] = x; sh.pixel[1] = y; sh.spp = spp;
                    sh.segment = ray.segment + 1;
                    sh.scene_seed = ray.scene_seed;
                    sh.info_t = ray.info_t + r.sample_t;
                    sh.first_scatter = 0;
                    sh.bounce = ray.bounce + 1;
                    sh.last_val = r.last_val;
                    sh.last_gp_id = r.gp_id;
                    sh.last_aniso[0] = r.aniso[0]; sh.last_aniso[1] = r.aniso[1]; sh.last_aniso[2] = r.aniso[2];
                    // the shadow segment: in place on the state (context and sampler) the primary segment left
                    FsState shadow;
                    shadow.first_scatter = sh.first_scatter != 0;
                    shadow.last_gp_id = sh.last_gp_id;
                    shadow.last_aniso = V3d{sh.last_aniso[0], sh.last_aniso[1], sh.last_aniso[2]};
                    FS_SYNC();
                    const bool vis = fs_transmittance_one(M, L, G, g, &sh, st, shadow, lane);
                    rec.cv = c * (vis ? 1.f : 0.f);
                    rec.flags = 3u;
                }
            }
        }
        if (lane == 0) recs[i] = rec;
    }
}

// one lane per pixel: sequential sum over its samples, in sample order (k_scene_accumulate's sum, as k_ws_scene_sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_fs_scene_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, const FsSceneRec *__restrict__ recs,
                                                                     float *__restrict__ radiance_sum, uint32_t *__restrict__ hit_count)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pixels) return;
    const uint32_t spp = sc.s.spp_count;
    float acc = 0.f;
    uint32_t hits = 0;
    for (uint32_t k = 0; k < spp; ++k) {
        const FsSceneRec r = recs[j * spp + k];
        hits += r.flags & 1u;
        if (r.flags & 2u)
            acc += r.cv * sc.s.light_radiance;
    }
    const size_t pix = scene_pixel(sc.s, first_pixel + j);
    radiance_sum[pix] += acc;
    if (hit_count) hit_count[pix] += hits;
}

}   // namespace gpis
