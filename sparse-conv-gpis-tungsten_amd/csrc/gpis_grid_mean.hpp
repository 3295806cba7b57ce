// gpis_grid_mean.hpp — a dense voxel grid read as VdbGrid::density reads its tree (VdbGrid.cpp:405-431), and TabulatedMean over it
// (GPF.hpp:1007-1025, GPF.cpp:165-190).  grid_density is the lookup GridNonstationaryCovariance and TabulatedMean share: the
// narrowing to Vec3f, the rows of invNaturalTransform, the clamp to [bounds_min + 2, bounds_max - 3] (always: no emission grid is
// built), then OpenVDB's PointSampler / BoxSampler restated from tools/Interpolation.h over a dense array whose outside reads the
// background 0 of an empty tree (absent dependency: parity unpinned for the lookup; same code as the oracle's).
//
// Included by gpis_device.hpp only, outside any namespace, at the one place that fits: everything this header uses must be declared
// above the include — GPIS_DEV, DevGrid, DevModel (mean, mean_grid, mean_volume), V3d and, from gpis_libm.hpp, log_glibc — and
// grid_unscaled_variance, which calls grid_density, below it.  One lane looks up its own point: the eight corners of the Box sampler are per-lane
// gathers (32 per gradient), no LDS, no cross-lane traffic; the descriptor is wave-uniform.  tabulated_mean / tabulated_mean_grad are
// reached from sdf::mean_weight_space / sdf::mean_grad only (gpis_sdf.hpp: the all-features path instance and k_mean).
#pragma once

#pragma clang fp contract(off)

namespace gpis {

// _grid->density(invNaturalTransform * Vec3f(x, y, z)); G.vox must be set
GPIS_DEV float grid_density(const DevGrid &G, float x, float y, float z)
{
    float q[3] = {G.T[0] * x + G.T[1] * y + G.T[2] * z + G.T[3], G.T[4] * x + G.T[5] * y + G.T[6] * z + G.T[7], G.T[8] * x + G.T[9] * y + G.T[10] * z + G.T[11]};
    for (int c = 0; c < 3; ++c) {
        const float v = q[c] < G.lo[c] ? G.lo[c] : q[c];
        q[c] = v < G.hi[c] ? v : G.hi[c];
    }
    auto voxel = [&](long i, long j, long k) -> float {
        i -= G.origin[0]; j -= G.origin[1]; k -= G.origin[2];
        if (i < 0 || j < 0 || k < 0 || i >= G.dims[0] || j >= G.dims[1] || k >= G.dims[2]) return 0.f;
        return G.vox[(size_t)i + (size_t)G.dims[0] * ((size_t)j + (size_t)G.dims[1] * (size_t)k)];
    };
    auto lerp = [](float a, float b, double w) -> float { const double temp = (double)(b - a) * w; return a + (float)temp; };
    const double xd = q[0], yd = q[1], zd = q[2];
    if (G.interpolate == 0)
        return voxel((long)floor(xd + 0.5), (long)floor(yd + 0.5), (long)floor(zd + 0.5));
    const double fx = floor(xd), fy = floor(yd), fz = floor(zd);
    const long i = (long)fx, j = (long)fy, k = (long)fz;
    const double u = xd - fx, v = yd - fy, w = zd - fz;
    return lerp(lerp(lerp(voxel(i, j, k), voxel(i, j, k + 1), w), lerp(voxel(i, j + 1, k), voxel(i, j + 1, k + 1), w), v),
                lerp(lerp(voxel(i + 1, j, k), voxel(i + 1, j, k + 1), w), lerp(voxel(i + 1, j + 1, k), voxel(i + 1, j + 1, k + 1), w), v), u);
}

// TabulatedMean::mean, GPF.cpp:165-172: the float density widened, -log(max(0.0001, res)) in double for a "volume" grid, then
// (res + offset) * scale in double.  Without a grid (gpis_set_mean_grid not called yet) the density is the background 0.
GPIS_DEV double tabulated_mean(const DevModel &M, int w, V3d a)
{
    const DevGrid &G = M.mean_grid[w];
    double res = G.vox ? (double)grid_density(G, (float)a.x, (float)a.y, (float)a.z) : 0.0;
    if (M.mean_volume[w])
        res = -log_glibc(0.0001 > res ? 0.0001 : res);            // max of MathUtil.hpp:26-29 on two doubles
    return (res + (double)M.mean[w].offset) * (double)M.mean[w].scale;
}
// TabulatedMean::dmean_da, GPF.cpp:179-190: eps = 0.001 (a double), the order +x, +y, +z, a
GPIS_DEV V3d tabulated_mean_grad(const DevModel &M, int w, V3d a)
{
    const double eps = 0.001;
    double v0 = 0., v1 = 0., v2 = 0., v3 = 0.;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {     // one body, four trips: the lookup's code is emitted once
        const V3d q{a.x + (k == 0 ? eps : 0.), a.y + (k == 1 ? eps : 0.), a.z + (k == 2 ? eps : 0.)};
        const double v = tabulated_mean(M, w, k == 3 ? a : q);
        v0 = k == 0 ? v : v0; v1 = k == 1 ? v : v1; v2 = k == 2 ? v : v2; v3 = k == 3 ? v : v3;
    }
    return V3d{(v0 - v3) / eps, (v1 - v3) / eps, (v2 - v3) / eps};
}

}   // namespace gpis
