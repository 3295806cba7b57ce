// tu_fs_scene.hip — the scene-S frame of the function-space medium (gpis_fs_render_scene_s in tu_scene.hip; gpis_fs_scene.hpp,
// gpis_launch.hpp): the fused kernel of one chunk of samples, on the uniform and on the adaptive sample layout
// (gpis_fs_render_scene_s_adaptive in tu_fs_adaptive.hip), and the per-pixel sum of the uniform layout's records.
#include "gpis_fs_scene.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

size_t fs_scene_rec_bytes() { return sizeof(FsSceneRec); }
void fs_scene(unsigned grid, const DevModel *d_model, const SceneConst &sc, size_t first_pixel, uint32_t n_samples, uint32_t *next, void *recs,
              void *workspace, gpis_fs_state *slots, hipStream_t s)
{
    k_fs_scene<0><<<grid, 64, 0, s>>>(d_model, sc, first_pixel, n_samples, next, (FsSceneRec *)recs, (FsGlob *)workspace, slots);
}
void fs_scene_adaptive(unsigned grid, const DevModel *d_model, const SceneConst &sc, const AdaptiveChunk &ch, uint32_t n_samples, uint32_t *next, void *recs,
                       void *workspace, gpis_fs_state *slots, hipStream_t s)
{
    k_fs_scene_adaptive<0><<<grid, 64, 0, s>>>(d_model, sc, ch, n_samples, next, (FsSceneRec *)recs, (FsGlob *)workspace, slots);
}
void fs_scene_sum(const SceneConst &sc, size_t first_pixel, size_t n_pixels, const void *recs, float *radiance_sum, uint32_t *hit_count, hipStream_t s)
{
    k_fs_scene_sum<0><<<grid_of(n_pixels, 256), 256, 0, s>>>(sc, first_pixel, n_pixels, (const FsSceneRec *)recs, radiance_sum, hit_count);
}

}}   // namespace gpis::launch
