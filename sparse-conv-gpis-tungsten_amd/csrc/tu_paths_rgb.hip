// tu_paths_rgb.hip — the per-bounce kernels of the RGB multi-bounce path driver of the sparse-convolution medium
// (gpis_render_scene_s_paths_rgb in gpis_hip.hip; gpis_paths_rgb.hpp, gpis_launch.hpp).
#include "gpis_paths_rgb.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

void paths_rgb_begin(const SceneConst &sc, size_t first_pixel, size_t n_samples, const PathsRgbArrays &a, hipStream_t s)
{
    k_paths_rgb_begin<0><<<grid_of(n_samples, 256), 256, 0, s>>>(sc, first_pixel, n_samples, a);
}
void paths_rgb_shade(const DevModel *d_model, const SceneConst &sc, size_t n_samples, int bounce, int max_bounces, bool emissive, const float albedo[3],
                     const PathsRgbArrays &a, const uint32_t *order, const gpis_ray_in *rays_in, const uint8_t *live, hipStream_t s)
{
    k_paths_rgb_shade<0><<<grid_of(n_samples, 256), 256, 0, s>>>(d_model, sc, n_samples, bounce, max_bounces, emissive ? 1 : 0, albedo[0], albedo[1],
                                                                 albedo[2], a, order, rays_in, live);
}
void paths_rgb_nee_add(size_t n_samples, const PathsRgbArrays &a, const uint32_t *order, const uint32_t *shadow_order, const uint8_t *shadow_live,
                       hipStream_t s)
{
    k_paths_rgb_nee_add<0><<<grid_of(n_samples, 256), 256, 0, s>>>(n_samples, a, order, shadow_order, shadow_live, a.vis);
}
void paths_rgb_accumulate(const SceneConst &sc, size_t first_pixel, size_t n_pixels, const PathsRgbArrays &a, float *radiance_sum3, hipStream_t s)
{
    k_paths_rgb_accumulate<0><<<grid_of(n_pixels, 256), 256, 0, s>>>(sc, first_pixel, n_pixels, a.plane, a.emission, radiance_sum3);
}
void paths_rgb_segs(const SceneConst &sc, size_t first_pixel, size_t n_pixels, const PathsRgbArrays &a, uint32_t *seg_count, hipStream_t s)
{
    k_paths_rgb_segs<0><<<grid_of(n_pixels, 256), 256, 0, s>>>(sc, first_pixel, n_pixels, a.segs, seg_count);
}

}}   // namespace gpis::launch
