// tu_guide_build.hip — tabulation of the certified guide field and its two self-checks (gpis_guide.hpp, gpis_launch.hpp).
#include "gpis_guide.hpp"
#include "gpis_launch.hpp"

#pragma clang fp contract(off)

namespace gpis { namespace launch {

// Builds the guide field for the grid space of medium M (world space or isotropic-ray space).  `sparse`: tabulate only the bricks
// level 1 of the certificate can be asked about (a 4x coarser field, built first, bounds |N| per brick); otherwise every brick.
int guide_build(const DevModel &M, const DevModel *d_model, const FastTable &T, int half, int ppc, GuideField *F, bool sparse)
{
    guide_free(F);
    if (!fast_supported(M) || half < 2 || half > 64 || (ppc != 8 && ppc != 16 && ppc != 32 && ppc != 64))
        return GPIS_ERR_UNSUPPORTED;
    F->half = half; F->ppc = ppc; F->side = 2 * half * ppc;
    if (!M.iso3d) {
        F->R = M.radius_world;
        for (int a = 0; a < 3; ++a) F->alpha[a] = (M.invcov_world[4 * a] * 0.5f) * F->R * F->R;
    } else {
        F->R = M.radius_iso;
        for (int a = 0; a < 3; ++a) F->alpha[a] = 0.5f * F->R * F->R;
    }
    const size_t nblk = ((size_t)F->side / 4) * (F->side / 4) * (F->side / 4);
    const uint32_t nbricks = (uint32_t)(nblk / 64);
    const unsigned bgrid = (nbricks + 255u) / 256u;
    uint8_t *need = nullptr;
    uint32_t *slot_of = nullptr, *list = nullptr, *counters = nullptr;
    GuideField C{};
    auto fail = [&](int code) {
        (void)hipGetLastError();
        if (need) (void)hipFree(need);
        if (slot_of) (void)hipFree(slot_of);
        if (list) (void)hipFree(list);
        if (counters) (void)hipFree(counters);
        guide_free(&C);
        guide_free(F);
        return code;
    };
    if (hipMalloc(&F->blk, nblk * sizeof(uint64_t)) != hipSuccess) { F->blk = nullptr; return fail(GPIS_ERR_DEVICE); }
    if (hipMalloc(&need, nbricks) != hipSuccess || hipMalloc(&slot_of, (size_t)nbricks * 4) != hipSuccess || hipMalloc(&list, (size_t)nbricks * 4) != hipSuccess ||
        hipMalloc(&counters, 8) != hipSuccess || hipMemset(counters, 0, 8) != hipSuccess)
        return fail(GPIS_ERR_DEVICE);
    // 1. which bricks does level 1 need?  (a-priori bound on |N| per brick from the field at ppc / 4: its 4-point block = this brick)
    if (sparse && ppc >= 32) {
        const int st = guide_build(M, d_model, T, half, ppc / 4, &C, false);
        if (st != GPIS_OK) return fail(st);
    }
    k_guide_need<0><<<bgrid, 256>>>(d_model, *F, C.blk, need);
    k_guide_slots<0><<<bgrid, 256>>>(*F, need, slot_of, list, counters);
    uint32_t cnt[2] = {0, 0};
    if (hipMemcpy(cnt, counters, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(GPIS_ERR_DEVICE);
    guide_free(&C);
    F->n_alloc = cnt[0]; F->n_usable = cnt[1];
    // 2. the samples of the allocated bricks (at least one brick exists: the lookup table points unused bricks at slot 0)
    const size_t pool = (size_t)(cnt[0] ? cnt[0] : 1u) * kBrickFloats;
    if (hipMalloc(&F->G, pool * sizeof(float)) != hipSuccess) { F->G = nullptr; return fail(GPIS_ERR_DEVICE); }
    if (!cnt[0] && hipMemset(F->G, 0, pool * sizeof(float)) != hipSuccess) return fail(GPIS_ERR_DEVICE);
    const size_t n_items = (size_t)cnt[0] * 64, per_launch = (size_t)1 << 22;   // slabs of 4 Mi blocks
    for (size_t i0 = 0; i0 < n_items; i0 += per_launch)
        k_guide_build<0><<<(unsigned)(n_items - i0 < per_launch ? n_items - i0 : per_launch), 64>>>(d_model, T, *F, i0, list, slot_of, need);
    // 3. the blocks' bounds on |N| (reads the samples incl. the shared layers) and their bricks' slots
    for (size_t i0 = 0; i0 < n_items; i0 += (size_t)1 << 30)
        k_guide_amax<0><<<(unsigned)(((n_items - i0 < ((size_t)1 << 30) ? n_items - i0 : ((size_t)1 << 30)) + 255) / 256), 256>>>(*F, i0, n_items, list, need);
    if (hipDeviceSynchronize() != hipSuccess) return fail(GPIS_ERR_DEVICE);
    (void)hipFree(need); (void)hipFree(slot_of); (void)hipFree(list); (void)hipFree(counters);
    F->enabled = 1;
    return GPIS_OK;
}
void guide_selfcheck(const DevModel *d_model, const FastTable &T, const GuideField &F, size_t n, const float *points3, unsigned long long *stats,
                     float *max_ratio, float *sum_bound, hipStream_t s)
{
    k_guide_selfcheck<0><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, F, n, points3, stats, max_ratio, sum_bound);
}
void guide_raycheck(const DevModel *d_model, const FastTable &T, const GuideField &F, size_t n, const gpis_ray_in *rays, uint32_t steps,
                    unsigned long long *stats, hipStream_t s)
{
    k_guide_raycheck<0><<<grid_of(n, kFastBlock), kFastBlock, 0, s>>>(d_model, T, F, n, rays, steps, stats);
}

}}   // namespace gpis::launch
