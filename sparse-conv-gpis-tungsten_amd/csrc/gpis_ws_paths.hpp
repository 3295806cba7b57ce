// gpis_ws_paths.hpp — multi-bounce paths on scene S through the weight-space GP medium: one fused kernel, one wave per sample.
//
// The estimator is gpis_render_scene_s_paths's (tu_scene.hip: k_paths_begin, k_paths_shade, k_paths_nee_add, k_paths_accumulate),
// operation for operation: the camera ray and its three draws, the bounding-sphere chord, then per bounce a sampleDistance with
// segment word = bounce, next-event estimation of the directional light through a state copy with segment + 1 (one shadow
// transmittance), and a cosine bounce drawn by unit-disk rejection.  The draw order of the
// sample's PCG32 stream is jx, jy, u_march, then per bounce [u_shadow when NEE runs], the disk pairs, [u_march of the next
// segment when the path lives on].  The segment of bounce max - 1 is marched as the reference marches it (it counts in n_eval and
// n_seg) although nothing after it can reach the image: no NEE runs there and the light is a Dirac delta.
//
// The whole path stays in the wave: ray, carried state (last_aniso, last_gp_id, last_val, info_t, bounce), PCG state, throughput
// and emission are wave-uniform, and no gpis_ray_in / gpis_seg_out record goes to HBM.  A sample ends in one 4-byte record (its
// emission); k_ws_paths_sum adds a pixel's records in sample order, so the image depends neither on the order in which waves
// finish nor on how a frame is cut into calls.  Work fetch is k_ws_scene's: the next sample index comes from a global counter.
//
// Realization reuse, which a staged composition of gpis_ws_sample_distance_batch + gpis_ws_transmittance_batch cannot do (every
// batch entry rebuilds the realization of every ray):
//   single_realization — the handle's basis serves everything;
//   context GLOBAL — pss.w = 0 for every segment (ws_pss), so one realization is built per sample and serves the whole path;
//   the other contexts — the shadow segment of bounce b and the path segment of bounce b + 1 carry the SAME segment word b + 1,
//       so one ws_build serves both: the shadow segment and the next path segment are marched from the same basis.  A path of k
//       hits builds k + 1 realizations where the staged form builds up to 2k + 1.
// One realization per wave at a time is enough: the workspace is the handle's one [6][N] slice per workgroup.
//
// The camera step and the hit normal are gpis_scene.hpp's helpers, the counter flush is gpis_ws.hpp's.  The shade step (Duff
// frame, wi / wo, next-event estimation, disk rejection, next-ray fill) is stated here in full, as in k_paths_shade and
// k_fs_paths: shared as functions around the marches it made this kernel slower (gpis_scene.hpp).
// k_ws_paths_adaptive is the same body on the variable-count sample layout of an adaptive pass (gpis_adaptive.hpp: scene_sample of an
// AdaptiveChunk); gpis_ws_adaptive.hpp sums and accounts its records.
#pragma once
#include "gpis_frame_sum.hpp"
#include "gpis_scene.hpp"
#include "gpis_ws.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one sample's emission: the sum of its NEE contributions in bounce order (0 for a sample that misses the bound)
struct WsPathsRec { float emission; };
// what the sums and the tile statistics read of it (gpis_frame_sum.hpp): a mono estimator's scalar emission — raw as the uniform entry
// adds it, value after renderTile's clamp as the adaptive entry adds and accounts it; the driver counts nothing per pixel
struct WsPathsValues {
    const WsPathsRec *recs;
    GPIS_DEV float raw(size_t i) const { return recs[i].emission; }
    GPIS_DEV float value(size_t i) const { return adaptive_clamp(raw(i)); }
    GPIS_DEV uint32_t count(size_t) const { return 0u; }
};

// The body of the fused kernel, a template on the sample step `where` (scene_sample's second argument): size_t, the first pixel of
// a chunk with spp_count samples per pixel (k_ws_paths), or AdaptiveChunk, the records of an adaptive pass (k_ws_paths_adaptive;
// gpis_adaptive.hpp).  Sample i of the chunk leaves recs[i] either way; nothing else depends on the layout.  The arguments are the
// kernels' own, by value and without a second __restrict__ (the kernels' parameters carry it): restated here it changed the register
// allocation of k_ws_paths, which is pinned.  The one WsLds of a kernel is the body's.
template <typename Where>
GPIS_DEV void ws_paths_samples(const WsModel *Wp, SceneConst sc, Where where, uint32_t n_samples,
                               int max_bounces, float albedo, uint32_t *next_sample, WsPathsRec *recs,
                               double *workspace, WsCounters *counters)
{
    __shared__ WsLds L;
    const WsModel &W = *Wp;
    const gpis_scene_s &s = sc.s;
    const int lane = (int)threadIdx.x;
    double *own = workspace ? workspace + (size_t)blockIdx.x * 6 * (size_t)W.n : nullptr;
    const bool per_path = !W.single;
    const bool whole_path = W.ctx == GPIS_CTX_GLOBAL;             // per-path realizations: one for all segments of a sample
    const double *B = per_path ? own : W.basis;
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    WsTally tally{0, 0};
    bool overflow = false;
    unsigned long long segs = 0;
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(next_sample, 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_samples) break;
        // ---- k_paths_begin
        uint32_t x, y, spp;
        Pcg32 g = scene_sample(sc, where, i, x, y, spp);
        const float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
        const float u0 = normalized_uint(g.next_i());
        float emission = 0.f;
        gpis_ray_in ray;
        if (scene_camera_ray(sc, x, y, spp, jx, jy, ray)) {
            ray.u_jitter = u0;
            float thr = 1.f;
            int built = -1;                  // segment word of the realization in `own` (any word under GLOBAL once built)
            for (int bounce = 0; bounce < max_bounces; ++bounce) {
                if (per_path && (whole_path ? built < 0 : built != bounce)) {
                    uint32_t pss[4];
                    ws_pss(W, x, y, spp, (uint32_t)bounce, pss);
                    ws_build(W, pss, own, W.n, lane);        // each lane reads back only the functions it wrote
                    built = bounce;
                }
                segs++;
                __syncthreads();
                const gpis_seg_out r = ws_sample_distance(W, L, B, ray, lane, overflow, tally);
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
                            sh.u_jitter = normalized_uint(g.next_i());
                            const float contrib = thr * (f * s.light_radiance);
                            if (per_path && !whole_path) {   // segment word bounce + 1: also the next path segment's realization
                                uint32_t pss[4];
                                ws_pss(W, x, y, spp, sh.segment, pss);
                                ws_build(W, pss, own, W.n, lane);
                                built = bounce + 1;
                            }
                            segs++;
                            bool first_scatter = false;
                            int last_gp_id = sh.last_gp_id;
                            V3d last_aniso{sh.last_aniso[0], sh.last_aniso[1], sh.last_aniso[2]};
                            __syncthreads();
                            const bool vis = ws_transmittance_one(W, L, B, sh, first_scatter, last_gp_id, last_aniso, lane, overflow, tally);
                            emission += vis ? contrib : 0.f;
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
                nx.u_jitter = normalized_uint(g.next_i());
                ray = nx;
            }
        }
        if (lane == 0) recs[i] = WsPathsRec{emission};
    }
    ws_flush_counters(counters, tally, segs, overflow, lane);
}

GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_ws_paths(const WsModel *__restrict__ Wp, SceneConst sc, size_t first_pixel, uint32_t n_samples,
                                                                int max_bounces, float albedo, uint32_t *__restrict__ next_sample,
                                                                WsPathsRec *__restrict__ recs, double *__restrict__ workspace,
                                                                WsCounters *__restrict__ counters)
{
    ws_paths_samples(Wp, sc, first_pixel, n_samples, max_bounces, albedo, next_sample, recs, workspace, counters);
}

// the same samples under the adaptive schedule (gpis_ws_render_scene_s_paths_adaptive): sample i of the chunk `ch` of records
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_ws_paths_adaptive(const WsModel *__restrict__ Wp, SceneConst sc, AdaptiveChunk ch, uint32_t n_samples,
                                                                         int max_bounces, float albedo, uint32_t *__restrict__ next_sample,
                                                                         WsPathsRec *__restrict__ recs, double *__restrict__ workspace,
                                                                         WsCounters *__restrict__ counters)
{
    ws_paths_samples(Wp, sc, ch, n_samples, max_bounces, albedo, next_sample, recs, workspace, counters);
}

// one lane per pixel: sequential sum over its samples' emissions, in sample order (k_paths_accumulate's sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_ws_paths_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, const WsPathsRec *__restrict__ recs,
                                                                     float *__restrict__ radiance_sum)
{
    frame_values_sum(sc, first_pixel, n_pixels, WsPathsValues{recs}, radiance_sum, nullptr);
}

}   // namespace gpis
