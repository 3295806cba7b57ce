// gpis_fs_paths.hpp — multi-bounce paths on scene S through the function-space GP medium: one fused kernel, one wave per sample.
//
// The estimator is gpis_render_scene_s_paths's and gpis_ws_render_scene_s_paths's (gpis_ws_paths.hpp), operation for operation:
// camera ray, bounding-sphere chord, then per bounce a sampleDistance with segment word = bounce, next-event estimation of the
// directional light through one shadow transmittance with segment + 1, and a cosine bounce drawn by unit-disk rejection.  The
// segment of bounce max - 1 is marched and counted although nothing after it can reach the image, and the driver stops there.
// The frame has the shape of k_fs_scene (gpis_fs_scene.hpp): grid = the resident set of the function-space workspace, samples
// fetched from a global counter, FsLds + FsGlob as there, one 8-byte record per sample and a per-pixel sum in sample order.
// What is this medium's own:
//   one sampler — the sample's PCG32 stream gives jx, jy and then every variate of the medium AND of the bounce, in program
//       order: path segment b, [shadow segment of bounce b], the disk pairs of bounce b, path segment b + 1, ...  No u_march /
//       u_shadow is drawn.  The sampler is never forked: the shadow segment draws where the path segment stopped, and the path
//       goes on where the shadow segment stopped;
//   the state is a VALUE (include/gpis.h, gpis_fs_state) — the path goes on after a shadow segment here, so the shadow segment
//       must not alter the path's context.  A workgroup owns TWO state slots: `path` holds the context the path segments leave,
//       and before every shadow segment the 64 lanes copy it into `shadow`, on which fs_transmittance_one then runs.  Segment
//       b + 1 of the path is conditioned on what segment b left in `path`, untouched by the shadow segment.  The whole 2 424-byte
//       record is copied (303 eight-byte words, five rounds of the wave) whatever n_points and has_context say: simple, at a
//       cost per shadow segment that has not been measured.
// The march itself is k_fs_march's: fs_sample_distance_one / fs_transmittance_one (gpis_fs.hpp), the same code for three kernels.
//
// Wave-uniform control flow.  A workgroup is one wave and FS_SYNC is a barrier, so every branch around one must be taken by all
// 64 lanes alike.  Every value that steers control flow is computed by every lane from the same inputs: the sample index is
// broadcast from lane 0 (readfirstlane); x, y, spp, the Pcg32, the ray, the FsState, throughput and emission derive from it and
// from kernel arguments; fs_sample_distance_one and fs_transmittance_one return wave-uniform results (gpis_fs.hpp).  The
// sample's pixel and stream and the hit normal are gpis_scene.hpp's helpers (scene_sample, hit_normal): they hold no barrier and
// no branch on the lane and read only their arguments, so on uniform arguments their results are uniform.  Of the medium's own
// helpers, fs_state_of is arithmetic on the ray; fs_reset_state holds an FS_SYNC and a lane-0 store, and is called by all 64
// lanes from a uniform branch.  The loop exits:
//   the fetch loop ends when i >= n_samples — i is the broadcast value;
//   the bounce loop ends on its trip count (a kernel argument), on !r.ok / r.exited (fields of the uniform segment record), on
//       !(wi.z > 0) (float arithmetic on the uniform ray and record) and on a missing chord (sphere_chord on uniform p, w);
//   the rejection loop ends when d2 < 1 — dx, dy are draws of the uniform Pcg32, so its trip count is the same in every lane;
//   the copy loop runs w = lane, lane + 64, ... < 303: a per-lane trip count, but it holds no barrier; the FS_SYNCs sit outside.
//
// The camera ray and the shade step (Duff frame, wi / wo, next-event estimation, disk rejection, next-ray fill) are stated here
// in full, the shade step as in k_ws_paths and k_paths_shade: as functions around the marches they made this kernel slower
// (gpis_scene.hpp).  The tests pin all three against the same C (tests/native/ws_paths_shade.c, tests/native/fs_paths_shade.c).
#pragma once
#include "gpis_frame_sum.hpp"
#include "gpis_fs.hpp"
#include "gpis_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one sample: its emission (the sum of its NEE contributions in bounce order; 0 for a sample that misses the bound) and the
// segments marched for it, path plus shadow
struct FsPathsRec { float emission; uint32_t segs; };
// what the sums and the tile statistics read of it (gpis_frame_sum.hpp): a mono estimator's scalar emission — raw as the uniform entry
// adds it, value after renderTile's clamp as the adaptive entry adds and accounts it; the count is the sample's segments, path plus
// shadow, whether or not the clamp took its value
struct FsPathsValues {
    const FsPathsRec *recs;
    GPIS_DEV float raw(size_t i) const { return recs[i].emission; }
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(raw(i)); }
    GPIS_DEV uint32_t count(size_t i) const { return recs[i].segs; }
};

static_assert(sizeof(gpis_fs_state) % sizeof(unsigned long long) == 0 && alignof(gpis_fs_state) == alignof(unsigned long long), "the state copies as whole 8-byte words");

// grid = the resident set of the function-space workspace: workspace[blockIdx.x], path_slots[blockIdx.x] and
// shadow_slots[blockIdx.x] are this workgroup's for the whole launch.
// The body of the fused kernel, a template on the sample step `where` (scene_sample's second argument), as ws_paths_samples is
// (gpis_ws_paths.hpp): size_t, the first pixel of a chunk with spp_count samples per pixel, for k_fs_paths; AdaptiveChunk, the
// records of an adaptive pass (gpis_adaptive.hpp), for k_fs_paths_adaptive.  Sample i of the chunk leaves recs[i] either way.  The
// arguments are the kernels' own, by value and without a second __restrict__ (the kernels' parameters carry it): k_fs_paths's
// registers are pinned.  (k_fs_scene shares its body as included text instead, gpis_fs_scene_body.inc: the template form cost it
// frame time, this kernel none; as included text this kernel would lose five of its accumulation registers against the pin.)
template <typename Where>
GPIS_DEV void fs_paths_samples(const DevModel *Mp, SceneConst sc, Where where, uint32_t n_samples, int max_bounces, float albedo, uint32_t *next,
                               FsPathsRec *recs, FsGlob *workspace, gpis_fs_state *path_slots, gpis_fs_state *shadow_slots)
{
    __shared__ FsLds L;
    FsGlob &G = workspace[blockIdx.x];
    gpis_fs_state *st = path_slots + blockIdx.x;
    gpis_fs_state *st_shadow = shadow_slots + blockIdx.x;
    const DevModel &M = *Mp;
    const gpis_scene_s &s = sc.s;
    const int lane = (int)threadIdx.x;
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(next, 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_samples) break;
        // ---- the camera step of k_fs_scene: the path's sampler gives jx, jy and is then the medium's and the bounce's
        uint32_t x, y, spp;
        Pcg32 g = scene_sample(sc, where, i, x, y, spp);
        const float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
        const V3 local = normalized(v3(-1.0f + ((float)x + jx) * 2.0f * sc.psx, sc.ratio - ((float)y + jy) * 2.0f * sc.psx, sc.plane_dist));
        const V3 d0 = v3(local.x, local.y, -local.z);
        const V3 o0 = v3(s.cam_pos[0], s.cam_pos[1], s.cam_pos[2]);
        FsPathsRec rec{0.f, 0u};
        float c0 = 0.f, c1 = 0.f;
        if (sphere_chord(o0, d0, s.bound_radius, c0, c1)) {
            gpis_ray_in ray{};
            ray.pos[0] = o0.x; ray.pos[1] = o0.y; ray.pos[2] = o0.z;
            ray.dir[0] = d0.x; ray.dir[1] = d0.y; ray.dir[2] = d0.z;
            ray.near_t = c0; ray.far_t = c1;
            ray.pixel[0] = x; ray.pixel[1] = y; ray.spp = spp; ray.segment = 0;
            ray.scene_seed = s.scene_seed; ray.info_t = 0.f;
            ray.first_scatter = 1;
            fs_reset_state(st, lane);            // the slot still holds the previous sample's context
            float thr = 1.f;
            for (int bounce = 0; bounce < max_bounces; ++bounce) {
                FsState state = fs_state_of(ray);
                rec.segs++;
                FS_SYNC();
                const gpis_seg_out r = fs_sample_distance_one(M, L, G, g, &ray, st, state, lane);
                // ---- k_paths_shade
                if (!r.ok) break;
                thr = thr * r.weight[0];
                if (r.exited) break;
                if (bounce + 1 >= max_bounces) break;        // no NEE at the last bounce, and the bounce itself cannot be seen
                const V3 n = hit_normal(r);
                const Frame fr = frame_from_normal(n);
                const V3 dir = v3(ray.dir[0], ray.dir[1], ray.dir[2]);
                const V3 wi = normalized(to_local(fr, v3(-dir.x, -dir.y, -dir.z)));
                const V3 p = v3(r.p[0], r.p[1], r.p[2]);
                gpis_ray_in nx{};
                nx.pos[0] = p.x; nx.pos[1] = p.y; nx.pos[2] = p.z;
                nx.near_t = 0.f;
                nx.pixel[0] = x; nx.pixel[1] = y; nx.spp = spp;
                nx.scene_seed = ray.scene_seed;
                nx.info_t = ray.info_t + r.sample_t;
                nx.first_scatter = 0;
                nx.bounce = ray.bounce + 1;
                nx.last_val = r.last_val;
                nx.last_gp_id = r.gp_id;
                nx.last_aniso[0] = r.aniso[0]; nx.last_aniso[1] = r.aniso[1]; nx.last_aniso[2] = r.aniso[2];
                nx.segment = (uint32_t)bounce + 1;
                {
                    const V3 wo = normalized(to_local(fr, l));
                    if (wi.z > 0.0f && wo.z > 0.0f) {
                        const float f = albedo * (1.0f / 3.1415926536f) * wo.z;
                        float t0, t1;
                        if (sphere_chord(p, l, s.bound_radius, t0, t1)) {
                            gpis_ray_in sh = nx;
                            sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                            sh.far_t = t1;
                            const float contrib = thr * (f * s.light_radiance);
                            // the shadow segment works on a copy of the path's state and on the path's sampler
                            FS_SYNC();
                            {
                                const char *src = (const char *)__builtin_assume_aligned((const void *)st, 8);
                                char *dst = (char *)__builtin_assume_aligned((void *)st_shadow, 8);
                                for (int w = lane; w < (int)(sizeof(gpis_fs_state) / 8); w += 64)
                                    __builtin_memcpy(dst + 8 * w, src + 8 * w, 8);       // an 8-byte load and store: no lvalue of another type
                            }
                            __threadfence_block();
                            FsState shadow = fs_state_of(sh);
                            rec.segs++;
                            FS_SYNC();
                            const bool vis = fs_transmittance_one(M, L, G, g, &sh, st_shadow, shadow, lane);
                            rec.emission += vis ? contrib : 0.f;
                        }
                    }
                }
                if (!(wi.z > 0.0f)) break;
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
                if (!sphere_chord(p, w, s.bound_radius, t0, t1)) break;
                nx.dir[0] = w.x; nx.dir[1] = w.y; nx.dir[2] = w.z;
                nx.far_t = t1;
                ray = nx;
            }
        }
        if (lane == 0) recs[i] = rec;
    }
}

GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_fs_paths(const DevModel *__restrict__ Mp, SceneConst sc, size_t first_pixel, uint32_t n_samples,
                                                                int max_bounces, float albedo, uint32_t *__restrict__ next, FsPathsRec *__restrict__ recs,
                                                                FsGlob *__restrict__ workspace, gpis_fs_state *__restrict__ path_slots,
                                                                gpis_fs_state *__restrict__ shadow_slots)
{
    fs_paths_samples(Mp, sc, first_pixel, n_samples, max_bounces, albedo, next, recs, workspace, path_slots, shadow_slots);
}

// the same samples under the adaptive schedule (gpis_fs_render_scene_s_paths_adaptive): sample i of the chunk `ch` of records
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_fs_paths_adaptive(const DevModel *__restrict__ Mp, SceneConst sc, AdaptiveChunk ch, uint32_t n_samples,
                                                                         int max_bounces, float albedo, uint32_t *__restrict__ next,
                                                                         FsPathsRec *__restrict__ recs, FsGlob *__restrict__ workspace,
                                                                         gpis_fs_state *__restrict__ path_slots, gpis_fs_state *__restrict__ shadow_slots)
{
    fs_paths_samples(Mp, sc, ch, n_samples, max_bounces, albedo, next, recs, workspace, path_slots, shadow_slots);
}

// one lane per pixel: sequential sum over its samples' emissions, in sample order (k_paths_accumulate's sum, as k_fs_scene_sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_fs_paths_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, const FsPathsRec *__restrict__ recs,
                                                                     float *__restrict__ radiance_sum, uint32_t *__restrict__ seg_count)
{
    frame_values_sum(sc, first_pixel, n_pixels, FsPathsValues{recs}, radiance_sum, seg_count);
}

}   // namespace gpis
