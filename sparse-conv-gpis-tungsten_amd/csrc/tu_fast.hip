// tu_fast.hip — wave-cooperative march for single-realization media and its cell table (gpis_fast.hpp, gpis_launch.hpp).
#include <cstdlib>

#include "gpis_fast.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

int fast_table_build(const DevModel &M, FastTable *t)
{
    t->cells = nullptr;
    t->half = 0;
    t->stride = 0;
    t->enabled = fast_supported(M) && !getenv("GPIS_DISABLE_FAST");
    if (!t->enabled || getenv("GPIS_DISABLE_TABLE"))
        return GPIS_OK;
    int half = 16;   // covers |p| < 16 cells: scene S spans 14.2 cells (1.5 world units / cell size 0.106)
    if (const char *e = getenv("GPIS_TABLE_HALF_EXTENT")) half = atoi(e);
    if (half < 2) return GPIS_OK;
    if (half > 40) half = 40;
    const int stride = M.n_impulses <= 32 ? 32 : 64;
    const size_t ncell = (size_t)(2 * half) * (2 * half) * (2 * half);
    if (hipMalloc(&t->cells, ncell * stride * sizeof(float4)) != hipSuccess) {
        t->cells = nullptr;   // no table: fall back to per-wave generation
        (void)hipGetLastError();
        return GPIS_OK;
    }
    k_fast_build_table<0><<<(unsigned)ncell, 64>>>(M.seed, half, stride, t->cells);
    if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(t->cells);
        t->cells = nullptr;
        return GPIS_ERR_DEVICE;
    }
    t->half = half;
    t->stride = stride;
    return GPIS_OK;
}
void fast_sample_distance(const DevModel *d_model, const FastTable &T, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, gpis_cond_coeff *coeff,
                          const uint8_t *mask, Counters *cnt, hipStream_t s)
{
    k_fast_sample_distance<0><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, n, rays, out, coeff, mask, cnt);
}
void fast_transmittance(const DevModel *d_model, const FastTable &T, size_t n, const gpis_ray_in *rays, uint8_t *visible, const uint8_t *mask,
                        Counters *cnt, hipStream_t s)
{
    k_fast_transmittance<0><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, n, rays, visible, mask, cnt);
}

}}   // namespace gpis::launch
