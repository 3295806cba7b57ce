// tu_guided_tr.hip — resident guided march, transmittance (gpis_guide.hpp, gpis_launch.hpp).
#include "gpis_guide.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

void guided_transmittance(bool small_arg, bool lean, const DevModel *d_model, const FastTable &T, const GuideField *d_guide, size_t n, const gpis_ray_in *rays,
                          uint8_t *visible, const uint8_t *mask, Counters *cnt, unsigned long long *guide_cnt, hipStream_t s)
{
    if (lean) {
        if (small_arg) k_shadow_lean<true><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, visible, mask, cnt, guide_cnt);
        else k_shadow_lean<false><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, visible, mask, cnt, guide_cnt);
        return;
    }
    if (small_arg) k_guided_transmittance<true><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, visible, mask, cnt, guide_cnt);
    else k_guided_transmittance<false><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, visible, mask, cnt, guide_cnt);
}
void guided_transmittance_scene(bool small_arg, bool lean, const DevModel *d_model, const FastTable &T, const GuideField *d_guide, size_t n, const SceneRay *rays,
                                const float light[3], uint8_t *visible, Counters *cnt, unsigned long long *guide_cnt, hipStream_t s)
{
    if (lean) {
        if (small_arg) k_shadow_lean_scene<true><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, light[0], light[1], light[2], visible, cnt, guide_cnt);
        else k_shadow_lean_scene<false><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, light[0], light[1], light[2], visible, cnt, guide_cnt);
        return;
    }
    if (small_arg) k_guided_transmittance_scene<true><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, light[0], light[1], light[2], visible, cnt, guide_cnt);
    else k_guided_transmittance_scene<false><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, d_guide, n, rays, light[0], light[1], light[2], visible, cnt, guide_cnt);
}
int fast_stats_read_tr(unsigned long long *out32)
{
#ifdef GPIS_FAST_STATS
    // diagnostic build only: this TU's copy of the work counters (the guided transmittance kernels), read and cleared
    unsigned long long h[32];
    if (hipDeviceSynchronize() != hipSuccess) return GPIS_ERR_DEVICE;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(gpis::g_fast_stats), sizeof h) != hipSuccess) return GPIS_ERR_DEVICE;
    for (int i = 0; i < 32; ++i) out32[i] = h[i];
    for (int i = 0; i < 32; ++i) h[i] = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(gpis::g_fast_stats), h, sizeof h) != hipSuccess) return GPIS_ERR_DEVICE;
    return GPIS_OK;
#else
    (void)out32;
    return GPIS_ERR_UNSUPPORTED;
#endif
}

}}   // namespace gpis::launch
