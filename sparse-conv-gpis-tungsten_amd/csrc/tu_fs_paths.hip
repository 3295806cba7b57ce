// tu_fs_paths.hip — the multi-bounce path frame of the function-space medium (gpis_fs_render_scene_s_paths in tu_scene.hip;
// gpis_fs_paths.hpp, gpis_launch.hpp): the fused kernel of one chunk of samples, on the uniform and on the adaptive sample layout
// (gpis_fs_render_scene_s_paths_adaptive in tu_fs_adaptive.hip), and the per-pixel sum of the uniform layout's records.
#include "gpis_fs_paths.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

size_t fs_paths_rec_bytes() { return sizeof(FsPathsRec); }
void fs_paths(unsigned grid, const DevModel *d_model, const SceneConst &sc, size_t first_pixel, uint32_t n_samples, int max_bounces, float albedo,
              uint32_t *next, void *recs, void *workspace, gpis_fs_state *path_slots, gpis_fs_state *shadow_slots, hipStream_t s)
{
    k_fs_paths<0><<<grid, 64, 0, s>>>(d_model, sc, first_pixel, n_samples, max_bounces, albedo, next, (FsPathsRec *)recs, (FsGlob *)workspace, path_slots,
                                      shadow_slots);
}
void fs_paths_adaptive(unsigned grid, const DevModel *d_model, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t n_samples, int max_bounces, float albedo,
                       uint32_t *next, void *recs, void *workspace, gpis_fs_state *path_slots, gpis_fs_state *shadow_slots, hipStream_t s)
{
    k_fs_paths_adaptive<0><<<grid, 64, 0, s>>>(d_model, sc, ch, n_samples, max_bounces, albedo, next, (FsPathsRec *)recs, (FsGlob *)workspace, path_slots,
                                               shadow_slots);
}
void fs_paths_sum(const SceneConst &sc, size_t first_pixel, size_t n_pixels, const void *recs, float *radiance_sum, uint32_t *seg_count, hipStream_t s)
{
    k_fs_paths_sum<0><<<grid_of(n_pixels, 256), 256, 0, s>>>(sc, first_pixel, n_pixels, (const FsPathsRec *)recs, radiance_sum, seg_count);
}

}}   // namespace gpis::launch
