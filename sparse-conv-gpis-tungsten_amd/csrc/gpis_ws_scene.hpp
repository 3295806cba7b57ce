// gpis_ws_scene.hpp — scene S rendered through the weight-space GP medium: one fused kernel, one wave per sample.
//
// The estimator is gpis_render_scene_s's (tu_scene.hip: k_scene_primary, k_scene_shade, k_scene_accumulate), bit for bit: the
// camera ray and its four draws, the bounding-sphere chord, a primary sampleDistance, Lambert shading against the directional
// light and one shadow transmittance per lit hit.  What differs is where the intermediate records live.  The staged drivers keep
// a gpis_ray_in and a gpis_seg_out per sample in HBM between five launches; here a wave carries its sample from the camera to one
// 8-byte record (WsSceneRec), and k_ws_scene_sum adds a pixel's records in sample order, so the image depends neither on the
// order in which waves finish nor on how a frame is cut into calls.
//
// Two things the staged composition of gpis_ws_sample_distance_batch + gpis_ws_transmittance_batch cannot do:
//   realization reuse — under single_realization or context GLOBAL the shadow segment's pixelSampleSegment is the primary's
//       (ws_pss: w = 0), so the realization built for the primary march serves the shadow march; the other contexts rebuild for
//       segment + 1, as the batch entries do;
//   dynamic work fetch — a sample costs nothing (a miss), a few batches (a hit near the chord's start) or the whole chord and
//       a shadow march; waves take the next sample index from a global counter (one atomic per wave per sample) instead of
//       k_ws_march's static stride, so no wave idles behind a neighbour's long samples at the end of a launch.
// k_ws_scene_adaptive is the same body on the variable-count sample layout of an adaptive pass (gpis_adaptive.hpp: scene_sample of an
// AdaptiveChunk); gpis_ws_adaptive.hpp sums and accounts its records.
#pragma once
#include "gpis_frame_sum.hpp"
#include "gpis_scene.hpp"
#include "gpis_ws.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one sample's contribution: cos(normal, light) * visible, and bit 0 = the primary segment hit the surface,
// bit 1 = lit (a shadow segment was marched; cv takes part in the pixel's sum)
struct WsSceneRec { float cv; uint32_t flags; };
// what the sums and the tile statistics read of it (gpis_frame_sum.hpp); count: whether the primary segment hit
struct WsSceneValues : SceneRecValues<WsSceneRec> {};

// The body of the fused kernel, a template on the sample step `where` (scene_sample's second argument): size_t, the first pixel of
// a chunk with spp_count samples per pixel (k_ws_scene), or AdaptiveChunk, the records of an adaptive pass (k_ws_scene_adaptive;
// gpis_adaptive.hpp).  Sample i of the chunk leaves recs[i] either way; nothing else depends on the layout.  The arguments are the
// kernels' own, by value and without a second __restrict__ (the kernels' parameters carry it): restated here it changed the register
// allocation of k_ws_scene, which is pinned.  The one WsLds of a kernel is the body's.
template <typename Where>
GPIS_DEV void ws_scene_samples(const WsModel *Wp, SceneConst sc, Where where, uint32_t n_samples,
                               uint32_t *next, WsSceneRec *recs, double *workspace,
                               WsCounters *counters)
{
    __shared__ WsLds L;
    const WsModel &W = *Wp;
    const gpis_scene_s &s = sc.s;
    const int lane = (int)threadIdx.x;
    double *own = workspace ? workspace + (size_t)blockIdx.x * 6 * (size_t)W.n : nullptr;
    const bool reuse = W.single || W.ctx == GPIS_CTX_GLOBAL;      // the shadow segment's realization is the primary's
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    WsTally tally{0, 0};
    bool overflow = false;
    unsigned long long segs = 0;
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(next, 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_samples) break;
        // ---- k_scene_primary
        uint32_t x, y, spp;
        Pcg32 g = scene_sample(sc, where, i, x, y, spp);
        const float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
        const float u0 = normalized_uint(g.next_i()), u1 = normalized_uint(g.next_i());
        WsSceneRec rec{0.f, 0u};
        gpis_ray_in ray;
        if (scene_camera_ray(sc, x, y, spp, jx, jy, ray)) {
            ray.u_jitter = u0;
            const double *B = W.basis;
            if (!W.single) {
                uint32_t pss[4];
                ws_pss(W, x, y, spp, ray.segment, pss);
                ws_build(W, pss, own, W.n, lane);        // each lane reads back only the functions it wrote
                B = own;
            }
            segs++;
            __syncthreads();
            const gpis_seg_out r = ws_sample_distance(W, L, B, ray, lane, overflow, tally);
            // ---- k_scene_shade
            if (r.ok && !r.exited) {
                rec.flags = 1u;
                const float c = dot(hit_normal(r), l);
                float s0, s1;
                if (c > 0.f && sphere_chord(v3(r.p[0], r.p[1], r.p[2]), l, s.bound_radius, s0, s1)) {
                    gpis_ray_in sh = scene_next_ray(ray, r);
                    sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                    sh.far_t = s1;
                    sh.u_jitter = u1;
                    if (!reuse) {
                        uint32_t pss[4];
                        ws_pss(W, x, y, spp, sh.segment, pss);
                        ws_build(W, pss, own, W.n, lane);
                    }
                    segs++;
                    bool first_scatter = false;
                    int last_gp_id = sh.last_gp_id;
                    V3d last_aniso{sh.last_aniso[0], sh.last_aniso[1], sh.last_aniso[2]};
                    __syncthreads();
                    const bool vis = ws_transmittance_one(W, L, B, sh, first_scatter, last_gp_id, last_aniso, lane, overflow, tally);
                    rec.cv = c * (vis ? 1.f : 0.f);
                    rec.flags = 3u;
                }
            }
        }
        if (lane == 0) recs[i] = rec;
    }
    ws_flush_counters(counters, tally, segs, overflow, lane);
}

GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_ws_scene(const WsModel *__restrict__ Wp, SceneConst sc, size_t first_pixel, uint32_t n_samples,
                                                                uint32_t *__restrict__ next, WsSceneRec *__restrict__ recs,
                                                                double *__restrict__ workspace, WsCounters *__restrict__ counters)
{
    ws_scene_samples(Wp, sc, first_pixel, n_samples, next, recs, workspace, counters);
}

// the same samples under the adaptive schedule (gpis_ws_render_scene_s_adaptive): sample i of the chunk `ch` of records
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_ws_scene_adaptive(const WsModel *__restrict__ Wp, SceneConst sc, AdaptiveChunk ch, uint32_t n_samples,
                                                                         uint32_t *__restrict__ next, WsSceneRec *__restrict__ recs,
                                                                         double *__restrict__ workspace, WsCounters *__restrict__ counters)
{
    ws_scene_samples(Wp, sc, ch, n_samples, next, recs, workspace, counters);
}

// one lane per pixel: sequential sum over its samples, in sample order (k_scene_accumulate's sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_ws_scene_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, const WsSceneRec *__restrict__ recs,
                                                                     float *__restrict__ radiance_sum, uint32_t *__restrict__ hit_count)
{
    frame_values_sum(sc, first_pixel, n_pixels, WsSceneValues{recs, sc.s.light_radiance}, radiance_sum, hit_count);
}

}   // namespace gpis
