// gpis_tables.hpp — the two device tables of a single-realization medium as the host sees them: the records that cross the
// host/device boundary (a handle owns them, a launcher passes them to a kernel by value) and their release.  No device function
// and no kernel lives here: the code that reads the tables is gpis_fast.hpp / gpis_guide.hpp, the code that fills them is
// launch::fast_table_build (tu_fast.hip) and launch::guide_build (tu_guide_build.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpis.h"
#include "gpis_device.hpp"    // DevModel

namespace gpis {

// Cell table in HBM (served from L2 / Infinity Cache): the impulses of every cell (i, j, k) with
// -H <= i, j, k < H, as float4 (x, y, z, w=+-1) in generation order, `stride` slots per cell.  A wave
// reads a cell with ONE coalesced 512-B / 1-KiB load; cells outside the table are generated on the
// fly, so the table is a cache and never a correctness bound.
struct FastTable {
    float4 *cells;   // nullptr = every cell is generated per wave
    int half;        // H
    int stride;      // 32 or 64 slots per cell
    int enabled;
};

inline bool fast_supported(const DevModel &M)
{
    return M.single_realization && !M.sampling_1d && !M.nonstationary && !M.use_aniso_mtx && !M.absorption_only && !M.color.enabled && !M.sdf_mean && M.kernel_type == GPIS_KERNEL_SQUARED_EXPONENTIAL &&
           M.n_impulses >= 1 && M.n_impulses <= 64;
}
inline void fast_table_free(FastTable *t)
{
    if (t->cells) (void)hipFree(t->cells);
    t->cells = nullptr;
    t->enabled = 0;
}

// Storage of the guide field: the samples live in BRICKS of 16^3 grid points (+ one layer shared with the +neighbours: 17^3 floats, so the eight taps of
// a lookup never leave their brick), and only the bricks a march can need at level 1 are tabulated: a brick is needed when, over the
// world points that can map into it, |mean| can come below sigma * amax / norm, amax = an a-priori bound on |N| over the brick
// from a field 4x coarser (1/64 of the work).  Everywhere else level 0 (guide_sign_at) decides every step by the mean alone, and
// the block records say so: Err = +inf there, so level 1 can certify nothing and the exact evaluation takes over — the need
// analysis decides speed, never results.  Scene S: 8 % of the bricks (2.8 of 34 GB at 16:64).
constexpr int kBrick = 16;                         // grid points per brick edge = 4 blocks
constexpr uint32_t kBrickRow = 17, kBrickFloats = 17u * 17u * 17u;
constexpr uint32_t kNoBrick = 0xFFFFFFFFu;
struct GuideField {
    float *G;            // pool of tabulated bricks: slot * 17^3 + (lx * 17 + ly) * 17 + lz
    uint64_t *blk;       // (side/4)^3 block records, dense, 8 bytes = one load per march step: slot << 32 | fp16 Err << 16 | fp16 amax (both
                         // rounded UP; Err = the bound of the block, +inf where the brick is not tabulated; amax = a bound on |N| anywhere in
                         // the block's cells; slot = the block's brick in the pool, 0 where not tabulated: Err = +inf makes its taps irrelevant)
    int half;            // extent in cells: u in [-half, half)
    int ppc;             // grid points per cell (h = 1/ppc)
    int side;            // 2*half*ppc
    float alpha[3];      // A_a * R^2
    float R;             // kernelRadius of the grid space
    int enabled;
    uint32_t n_alloc, n_usable;   // bricks in the pool / bricks level 1 may use
};

inline void guide_free(GuideField *F)
{
    if (F->G) (void)hipFree(F->G);
    if (F->blk) (void)hipFree(F->blk);
    F->G = nullptr; F->blk = nullptr; F->enabled = 0; F->n_alloc = 0; F->n_usable = 0;
}

}   // namespace gpis
