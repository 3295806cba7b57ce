// gpis_fs_scene.hpp — scene S rendered through the function-space GP medium: one fused kernel, one wave per sample.
//
// The estimator is gpis_render_scene_s's (tu_scene.hip: k_scene_primary, k_scene_shade, k_scene_accumulate) and the frame has
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
// k_fs_scene_adaptive is the same body (gpis_fs_scene_body.inc) on the variable-count sample layout of an adaptive pass
// (gpis_adaptive.hpp: scene_sample of an AdaptiveChunk); gpis_fs_adaptive.hpp sums and accounts its records.
#pragma once
#include "gpis_frame_sum.hpp"
#include "gpis_fs.hpp"
#include "gpis_scene.hpp"

#pragma clang fp contract(off)

namespace gpis {

// one sample's contribution: cos(normal, light) * visible, and bit 0 = the primary segment hit the surface (ok && !exited),
// bit 1 = lit (a shadow segment was marched; cv takes part in the pixel's sum)
struct FsSceneRec { float cv; uint32_t flags; };
// what the sums and the tile statistics read of it (gpis_frame_sum.hpp); count: whether the primary segment hit
struct FsSceneValues : SceneRecValues<FsSceneRec> {};

// grid = the resident set of the function-space workspace (four one-wave workgroups per CU): workspace[blockIdx.x] and
// slots[blockIdx.x] are this workgroup's for the whole launch.  Every value that steers control flow is computed identically by
// all 64 lanes (the sample index is broadcast from lane 0), so every branch around an FS_SYNC is wave-uniform.  The body is
// gpis_fs_scene_body.inc, shared with k_fs_scene_adaptive.
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_fs_scene(const DevModel *__restrict__ Mp, SceneConst sc, size_t first_pixel, uint32_t n_samples,
                                                                uint32_t *__restrict__ next, FsSceneRec *__restrict__ recs,
                                                                FsGlob *__restrict__ workspace, gpis_fs_state *__restrict__ slots)
{
#define GPIS_FS_SAMPLE_WHERE first_pixel
#include "gpis_fs_scene_body.inc"
#undef GPIS_FS_SAMPLE_WHERE
}

// the same samples under the adaptive schedule (gpis_fs_render_scene_s_adaptive): sample i of the chunk `ch` of records.  The sample
// index is wave-uniform, so the search of the chunk's offset table is scalar work.
GPIS_TU_KERNEL __global__ void __launch_bounds__(64) k_fs_scene_adaptive(const DevModel *__restrict__ Mp, SceneConst sc, AdaptiveChunk ch, uint32_t n_samples,
                                                                         uint32_t *__restrict__ next, FsSceneRec *__restrict__ recs,
                                                                         FsGlob *__restrict__ workspace, gpis_fs_state *__restrict__ slots)
{
#define GPIS_FS_SAMPLE_WHERE ch
#include "gpis_fs_scene_body.inc"
#undef GPIS_FS_SAMPLE_WHERE
}

// one lane per pixel: sequential sum over its samples, in sample order (k_scene_accumulate's sum, as k_ws_scene_sum)
GPIS_TU_KERNEL __global__ void __launch_bounds__(256) k_fs_scene_sum(SceneConst sc, size_t first_pixel, size_t n_pixels, const FsSceneRec *__restrict__ recs,
                                                                     float *__restrict__ radiance_sum, uint32_t *__restrict__ hit_count)
{
    frame_values_sum(sc, first_pixel, n_pixels, FsSceneValues{recs, sc.s.light_radiance}, radiance_sum, hit_count);
}

}   // namespace gpis
