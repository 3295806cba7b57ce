// gpis_nn_mean.hpp — the reference's NeuralMean (GPF.cpp:197-248 over GPNeuralNetwork.hpp's mean network), evaluated EXACTLY: an
// fp64 MLP with sine activations in the arithmetic the reference's build performs (Eigen 3.4.90, -O3 -msse4.2, no FMA; the
// host's sin), bit for bit.  Included by gpis_hip.hip only: no path instance sees it.  The march never evaluates the network; it
// reads the voxels gpis_bake_mean_network wrote through the tabulated mean (gpis_grid_mean.hpp).
//
// The three summation orders of `weights * in + biases` (Eigen::MatrixXd, column-major, times a dynamic vector):
//   rows > 1, cols < 128:   c = 0; c = c + W(i, j) x[j], j ascending; then + bias
//   rows > 1, cols >= 128:  GeneralMatrixVector.h switches to blocks of 16 columns (the last one shorter):
//                           res = 0; per block c0 = the sequential sum from 0, res = c0 * 1.0 + res; then + bias
//   rows == 1:              an unvectorised dot: W(0, 0) x[0], then += over ALL columns, never blocked; then + bias
// Every multiply-add is a multiply and an add (fp contract off).  The sine is sin_glibc (gpis_libm.hpp), out of line.
//
// One lane evaluates one point.  A layer's activations live in two buffers (input, output) addressed [j][lane]: in LDS for
// networks up to LDSW = 32 or 64 wide (32 / 64 KiB per one-wave workgroup; consecutive lanes are consecutive doubles, which
// ds_read_b64 serves without bank conflicts), in a launch-owned global workspace above that (the same layout over all lanes of
// the launch: coalesced).  The rows of a layer are blocked by kRows: kRows accumulators per lane, one activation read per column.
// The weights are column-major, so rows i .. i + 7 of a column are 64 contiguous bytes at a wave-uniform address: the compiler
// reads them with scalar loads (the blob and the workspace are __restrict__).  Lanes never exchange data: no barrier.
#pragma once

#include "gpis_device.hpp"

#pragma clang fp contract(off)

namespace gpis {
namespace nn {

constexpr int kRows = 8;
constexpr int kLanes = 64;             // one wave per workgroup

// the network as the kernels take it (a kernel argument: wave-uniform)
struct Net {
    int32_t n_layers, max_width;
    int32_t dims[GPIS_NN_MAX_LAYERS][2];
    uint32_t w_off[GPIS_NN_MAX_LAYERS];      // first double of layer k in the blob: out x in weights, then out biases
    double bmin[3], bmax[3];
    float offset, scale;
    float inv[12];                           // rows 0..2 of the inverted transform
};
// the lattice of a bake: voxel v = i + dims[0] (j + dims[1] k) sits at A . (origin + (i, j, k), 1)
struct Lattice {
    int32_t dims[3], origin[3];
    float A[12];
};

__device__ __noinline__ double sine(double x) { return sin_glibc(x); }

// rows i0 .. i0 + kRows - 1 of one layer with more than one row.  FULL: all of them exist; otherwise the rows past out - 1 read
// row out - 1 again (in bounds) and are not stored.
template <bool FULL>
GPIS_DEV void row_block(const double *__restrict__ w, const double *__restrict__ b, int in, int out, int i0, int block, bool sin_after,
                        const double *src, double *dst, size_t stride)
{
    int row[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) row[r] = FULL ? i0 + r : (i0 + r < out ? i0 + r : out - 1);
    double res[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) res[r] = 0.0;
    for (int j0 = 0; j0 < in; j0 += block) {
        const int jend = j0 + block < in ? j0 + block : in;
        double c[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) c[r] = 0.0;
#pragma unroll 4          // four columns' scalar loads and activation reads in flight; each accumulator's chain keeps its order
        for (int j = j0; j < jend; ++j) {
            const double xj = src[(size_t)j * stride];
            const double *col = w + (size_t)j * (size_t)out;
#pragma unroll
            for (int r = 0; r < kRows; ++r) c[r] = c[r] + col[row[r]] * xj;
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) res[r] = c[r] * 1.0 + res[r];
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r)
        if (FULL || i0 + r < out) {
            double v = res[r] + b[row[r]];
            if (sin_after) v = sine(v);
            dst[(size_t)row[r] * stride] = v;
        }
}

// GPNeuralNetwork::MLP::infer(p)(0).  act: this lane's first activation; buffer t, element j is act[t * buf + j * stride]
GPIS_DEV double infer(const Net &N, const double *__restrict__ W, double *act, size_t stride, size_t buf, double x, double y, double z)
{
    act[0] = x;
    act[stride] = y;
    act[2 * stride] = z;
    int cur = 0;
    double result = 0.0;
    for (int L = 0; L < N.n_layers; ++L) {
        const int in = N.dims[L][0], out = N.dims[L][1];
        const double *w = W + N.w_off[L], *b = w + (size_t)in * (size_t)out;
        const double *src = act + (size_t)cur * buf;
        double *dst = act + (size_t)(cur ^ 1) * buf;
        const bool last = L == N.n_layers - 1, sin_after = L > 0 && !last;      // no activation behind the input and output layers
        if (out == 1) {
            double c = w[0] * src[0];
            for (int j = 1; j < in; ++j) c = c + w[j] * src[(size_t)j * stride];
            c = c + b[0];
            if (sin_after) c = sine(c);
            dst[0] = c;
            result = c;
        } else {
            const int block = in < 128 ? in : 16;
            int i0 = 0;
            for (; i0 + kRows <= out; i0 += kRows) row_block<true>(w, b, in, out, i0, block, sin_after, src, dst, stride);
            if (i0 < out) row_block<false>(w, b, in, out, i0, block, sin_after, src, dst, stride);
        }
        cur ^= 1;
    }
    return result;         // the last layer has one row (gpis_mean_network's rule)
}

// NeuralMean::mean: mult(Mat4f, Vec3d) promotes the float entries and sums left to right; GPNeuralNetwork::mean clamps the point
// (cwiseMin(max), then cwiseMax(min)) only when Box::contains fails
GPIS_DEV double network_mean(const Net &N, const double *__restrict__ W, double *act, size_t stride, size_t buf, double ax, double ay, double az)
{
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        q[r] = (double)N.inv[4 * r] * ax + (double)N.inv[4 * r + 1] * ay + (double)N.inv[4 * r + 2] * az + (double)N.inv[4 * r + 3];
    bool outside = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) outside = outside || q[r] < N.bmin[r] || q[r] > N.bmax[r];
    if (outside) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            q[r] = N.bmax[r] < q[r] ? N.bmax[r] : q[r];
            q[r] = q[r] < N.bmin[r] ? N.bmin[r] : q[r];
        }
    }
    return (infer(N, W, act, stride, buf, q[0], q[1], q[2]) + (double)N.offset) * (double)N.scale;
}

// this lane's activation column: LDS for LDSW > 0 (the network is at most LDSW wide), the launch's workspace for LDSW == 0
template <int LDSW>
GPIS_DEV double *act_base(double *__restrict__ ws, const Net &N, size_t &stride, size_t &buf)
{
    if constexpr (LDSW > 0) {
        __shared__ double lds[2 * LDSW * kLanes];
        stride = kLanes;
        buf = (size_t)LDSW * kLanes;
        return lds + threadIdx.x;
    } else {
        stride = (size_t)gridDim.x * kLanes;
        buf = (size_t)N.max_width * stride;
        return ws + (size_t)blockIdx.x * kLanes + threadIdx.x;
    }
}

}   // namespace nn
}   // namespace gpis

// "the mean at n points", for a network: NeuralMean::mean and dmean_da (either may be null)
template <int LDSW>
__global__ void __launch_bounds__(gpis::nn::kLanes) k_mean(gpis::nn::Net N, const double *__restrict__ W, size_t n, const double *__restrict__ p3,
                                                          double *__restrict__ value, double *__restrict__ grad3, double *__restrict__ ws)
{
    using namespace gpis::nn;
    size_t stride, buf;
    double *act = act_base<LDSW>(ws, N, stride, buf);
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    const double ax = p3[3 * i], ay = p3[3 * i + 1], az = p3[3 * i + 2];
    if (!grad3) {
        value[i] = network_mean(N, W, act, stride, buf, ax, ay, az);
        return;
    }
    const double eps = 0.001;
    double vals[4];
    for (int k = 0; k < 4; ++k)          // a + Vec3d(eps, 0.f, 0.f), ..., a
        vals[k] = network_mean(N, W, act, stride, buf, ax + (k == 0 ? eps : 0.0), ay + (k == 1 ? eps : 0.0), az + (k == 2 ? eps : 0.0));
    if (value) value[i] = vals[3];
    for (int k = 0; k < 3; ++k) grad3[3 * i + k] = (vals[k] - vals[3]) / eps;
}

// the mean at voxels [first, first + n) of a lattice, narrowed to float
template <int LDSW>
__global__ void __launch_bounds__(gpis::nn::kLanes) k_mean(gpis::nn::Net N, const double *__restrict__ W, gpis::nn::Lattice G, size_t first, size_t n,
                                                          float *__restrict__ voxels, double *__restrict__ ws)
{
    using namespace gpis::nn;
    size_t stride, buf;
    double *act = act_base<LDSW>(ws, N, stride, buf);
    const size_t t = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (t >= n) return;
    const size_t v = first + t;
    const size_t dx = (size_t)G.dims[0], dy = (size_t)G.dims[1];
    const double ci = (double)(G.origin[0] + (int32_t)(v % dx)), cj = (double)(G.origin[1] + (int32_t)((v / dx) % dy)),
                 ck = (double)(G.origin[2] + (int32_t)(v / (dx * dy)));
    double x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = (double)G.A[4 * r] * ci + (double)G.A[4 * r + 1] * cj + (double)G.A[4 * r + 2] * ck + (double)G.A[4 * r + 3];
    voxels[v] = (float)network_mean(N, W, act, stride, buf, x[0], x[1], x[2]);
}
