/* TEST INFRASTRUCTURE: a plain-C restatement of the reference's NeuralMean (GPFunctions.cpp:197-248) over GPNeuralNetwork's mean
 * network (GPNeuralNetwork.hpp), the tests' reference for csrc/gpis_nn_mean.hpp and an independent second writing of it.
 *
 * Built with the oracle's flags (-msse4.2 -mno-fma -ffp-contract=off) against the host libm: the sine is the host's sin().
 *
 * `weights * in + biases` on a column-major Eigen::MatrixXd and a dynamic vector (Eigen 3.4.90, no FMA) sums in one of three orders,
 * pinned bit for bit by tests/golden/nn_mean_pins.npz (recorded through the reference's own compiled Eigen):
 *   rows > 1, cols < 128    c = 0; c += W(i, j) x[j], j ascending                                       then + bias
 *   rows > 1, cols >= 128   blocks of 16 columns: res = 0; per block c0 = sum from 0; res = c0 * 1 + res  then + bias
 *   rows == 1               W(0, 0) x[0], then += over all columns, never blocked                        then + bias
 * PARITY UNPINNED: the clamp, the transform, the sine's use and offset / scale are restated from the source text alone. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define NN_MAX_LAYERS 16
#define NN_MAX_WIDTH 256

typedef struct nn_ref_net {
    int32_t n_layers;
    int32_t _pad;
    int32_t dims[NN_MAX_LAYERS][2];
    double bounds_min[3], bounds_max[3];
    float offset, scale;
    float inv_transform[16];        /* the INVERTED transform (tests/sdf_mean_ref.py: sdf_ref_mat4_invert) */
} nn_ref_net;

size_t nn_ref_net_size(void) { return sizeof(nn_ref_net); }

/* y += W x as Eigen's GEMV accumulates into a destination (W rows x cols column-major): what `dst += W * x` performs.  The
 * network's `W * x + b` evaluates the product into a zeroed temporary and adds b afterwards (nn_ref_gemv); `b + W * x`, the form
 * the pins can record with a non-zero start, accumulates into a destination that already holds b.  The two differ in the last bit
 * once the columns are blocked. */
void nn_ref_gemv_acc(int rows, int cols, const double *W, const double *x, double *y)
{
    if (rows == 1) {
        double c = W[0] * x[0];
        for (int j = 1; j < cols; ++j) c += W[j] * x[j];
        y[0] += 1.0 * c;
        return;
    }
    const int block = cols < 128 ? cols : 16;
    for (int i = 0; i < rows; ++i) {
        double res = y[i];
        for (int j0 = 0; j0 < cols; j0 += block) {
            const int jend = j0 + block < cols ? j0 + block : cols;
            double c0 = 0.0;
            for (int j = j0; j < jend; ++j) c0 = W[(size_t)j * rows + i] * x[j] + c0;
            res = c0 * 1.0 + res;
        }
        y[i] = res;
    }
}
/* y = W x + b */
void nn_ref_gemv(int rows, int cols, const double *W, const double *b, const double *x, double *y)
{
    for (int i = 0; i < rows; ++i) y[i] = 0.0;
    nn_ref_gemv_acc(rows, cols, W, x, y);
    for (int i = 0; i < rows; ++i) y[i] = y[i] + b[i];
}

/* MLP::infer(p)(0); pre (may be null): receives every pre-activation a sine is applied to, returns how many through n_pre */
static double infer(const nn_ref_net *N, const double *w, const double p[3], double *pre, size_t *n_pre)
{
    double a[NN_MAX_WIDTH], t[NN_MAX_WIDTH];
    a[0] = p[0]; a[1] = p[1]; a[2] = p[2];
    for (int L = 0; L < N->n_layers; ++L) {
        const int in = N->dims[L][0], out = N->dims[L][1];
        nn_ref_gemv(out, in, w, w + (size_t)in * out, a, t);
        w += (size_t)out * (in + 1);
        const int sine = L > 0 && L < N->n_layers - 1;
        for (int i = 0; i < out; ++i) {
            if (sine && pre) pre[(*n_pre)++] = t[i];
            a[i] = sine ? sin(t[i]) : t[i];
        }
    }
    return a[0];
}

static double mean_at(const nn_ref_net *N, const double *w, double ax, double ay, double az, double *pre, size_t *n_pre)
{
    const float *T = N->inv_transform;
    double q[3];
    for (int r = 0; r < 3; ++r) q[r] = (double)T[4 * r] * ax + (double)T[4 * r + 1] * ay + (double)T[4 * r + 2] * az + (double)T[4 * r + 3];
    int inside = 1;
    for (int r = 0; r < 3; ++r)
        if (q[r] < N->bounds_min[r] || q[r] > N->bounds_max[r]) inside = 0;
    if (!inside)
        for (int r = 0; r < 3; ++r) {
            q[r] = N->bounds_max[r] < q[r] ? N->bounds_max[r] : q[r];      /* cwiseMin(max) */
            q[r] = q[r] < N->bounds_min[r] ? N->bounds_min[r] : q[r];      /* cwiseMax(min) */
        }
    return (infer(N, w, q, pre, n_pre) + (double)N->offset) * (double)N->scale;
}

/* NeuralMean::mean and dmean_da at n points; value / grad3 may be null */
void nn_ref_mean(const nn_ref_net *N, const double *w, size_t n, const double *p3, double *value, double *grad3)
{
#pragma omp parallel for schedule(static)
    for (ptrdiff_t i = 0; i < (ptrdiff_t)n; ++i) {
        const double ax = p3[3 * i], ay = p3[3 * i + 1], az = p3[3 * i + 2];
        const double m = mean_at(N, w, ax, ay, az, NULL, NULL);
        if (value) value[i] = m;
        if (grad3) {
            const double eps = 0.001;
            const double vx = mean_at(N, w, ax + eps, ay + 0.0, az + 0.0, NULL, NULL), vy = mean_at(N, w, ax + 0.0, ay + eps, az + 0.0, NULL, NULL),
                         vz = mean_at(N, w, ax + 0.0, ay + 0.0, az + eps, NULL, NULL);
            grad3[3 * i] = (vx - m) / eps;
            grad3[3 * i + 1] = (vy - m) / eps;
            grad3[3 * i + 2] = (vz - m) / eps;
        }
    }
}

/* the pre-activations of every sine at the points themselves (no gradient offsets): out holds n * (sum of hidden widths) doubles */
size_t nn_ref_preactivations(const nn_ref_net *N, const double *w, size_t n, const double *p3, double *out)
{
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) (void)mean_at(N, w, p3[3 * i], p3[3 * i + 1], p3[3 * i + 2], out, &k);
    return k;
}

/* the voxels of a bake: voxel (i, j, k) of dims at A . (origin + (i, j, k), 1), A = rows 0..2 of index_to_world in float */
void nn_ref_bake(const nn_ref_net *N, const double *w, const int32_t dims[3], const int32_t origin[3], const float A[12], float *voxels)
{
    const ptrdiff_t n = (ptrdiff_t)dims[0] * dims[1] * dims[2];
#pragma omp parallel for schedule(static)
    for (ptrdiff_t v = 0; v < n; ++v) {
        const double ci = (double)(origin[0] + (int32_t)(v % dims[0])), cj = (double)(origin[1] + (int32_t)((v / dims[0]) % dims[1])),
                     ck = (double)(origin[2] + (int32_t)(v / ((ptrdiff_t)dims[0] * dims[1])));
        double x[3];
        for (int r = 0; r < 3; ++r) x[r] = (double)A[4 * r] * ci + (double)A[4 * r + 1] * cj + (double)A[4 * r + 2] * ck + (double)A[4 * r + 3];
        voxels[v] = (float)mean_at(N, w, x[0], x[1], x[2], NULL, NULL);
    }
}
