/* TEST INFRASTRUCTURE: a plain-C restatement of the reference's TabulatedMean over a dense voxel array
 * (GPFunctions.cpp:165-190 over VdbGrid::density, VdbGrid.cpp:405-431, with OpenVDB's PointSampler / BoxSampler restated from
 * tools/Interpolation.h).  Written independently of csrc/gpis_grid_mean.hpp; compiled with -msse4.2 -mno-fma -ffp-contract=off and
 * linked against the host libm (tests/grid_mean_ref.py). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* the fields of gpis_variance_grid, in its layout (include/gpis.h) */
typedef struct {
    int32_t dims[3];
    int32_t interpolate;
    int32_t origin[3];
    int32_t pad_;
    float bounds_min[3], bounds_max[3];
    float inv_natural_transform[16];
} grid_desc;

typedef struct {
    const grid_desc *desc;      /* NULL: no grid, the density is the background 0 */
    const float *voxels;
    float offset, scale;
    int32_t volume;
} grid_slot;

/* the tree's value at an index-space coordinate: the dense array inside its box, the background outside */
static float tree_value(const grid_desc *g, const float *vox, int64_t ix, int64_t iy, int64_t iz)
{
    const int64_t c[3] = {ix - g->origin[0], iy - g->origin[1], iz - g->origin[2]};
    for (int a = 0; a < 3; ++a)
        if (c[a] < 0 || c[a] >= g->dims[a])
            return 0.0f;
    return vox[c[0] + (int64_t)g->dims[0] * (c[1] + (int64_t)g->dims[1] * c[2])];
}

/* VdbGrid::density at a world-space Vec3f: invNaturalTransform * p (Mat4f * Vec3f, Mat4f.hpp:168-175), the clamp, the sampler */
static float density(const grid_desc *g, const float *vox, float px, float py, float pz)
{
    const float *m = g->inv_natural_transform;
    float q[3];
    for (int r = 0; r < 3; ++r) {
        float acc = m[4 * r + 0] * px;
        acc = acc + m[4 * r + 1] * py;
        acc = acc + m[4 * r + 2] * pz;
        q[r] = acc + m[4 * r + 3];
    }
    for (int a = 0; a < 3; ++a) {                     /* clamp(p, bounds.min + 2, bounds.max - 3): min(max(p, lo), hi) */
        const float lo = g->bounds_min[a] + 2, hi = g->bounds_max[a] - 3;
        float t = q[a] > lo ? q[a] : lo;
        q[a] = t < hi ? t : hi;
    }
    const double d[3] = {(double)q[0], (double)q[1], (double)q[2]};          /* openvdb::Vec3R */
    if (g->interpolate == 0) {                         /* PointSampler: the nearest voxel, round half up */
        return tree_value(g, vox, (int64_t)floor(d[0] + 0.5), (int64_t)floor(d[1] + 0.5), (int64_t)floor(d[2] + 0.5));
    }
    int64_t base[3];
    double uvw[3];
    for (int a = 0; a < 3; ++a) {
        const double fl = floor(d[a]);
        base[a] = (int64_t)fl;
        uvw[a] = d[a] - fl;
    }
    float data[2][2][2];                               /* BoxSampler::getValues */
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy)
            for (int dz = 0; dz < 2; ++dz)
                data[dx][dy][dz] = tree_value(g, vox, base[0] + dx, base[1] + dy, base[2] + dz);
    /* BoxSampler::trilinearInterpolation: _interpolate(a, b, weight) { const auto temp = (b - a) * weight; return a + ValueT(temp); } */
    float along_z[2][2];
    for (int dx = 0; dx < 2; ++dx)
        for (int dy = 0; dy < 2; ++dy) {
            const double temp = (double)(data[dx][dy][1] - data[dx][dy][0]) * uvw[2];
            along_z[dx][dy] = data[dx][dy][0] + (float)temp;
        }
    float along_y[2];
    for (int dx = 0; dx < 2; ++dx) {
        const double temp = (double)(along_z[dx][1] - along_z[dx][0]) * uvw[1];
        along_y[dx] = along_z[dx][0] + (float)temp;
    }
    const double temp = (double)(along_y[1] - along_y[0]) * uvw[0];
    return along_y[0] + (float)temp;
}

void grid_ref_density(const grid_desc *g, const float *vox, size_t n, const double *p3, float *out)
{
    for (size_t i = 0; i < n; ++i)
        out[i] = density(g, vox, (float)p3[3 * i], (float)p3[3 * i + 1], (float)p3[3 * i + 2]);
}

/* TabulatedMean::mean, GPFunctions.cpp:165-172 */
static double tab_mean(const grid_slot *s, double ax, double ay, double az)
{
    double res = s->desc ? (double)density(s->desc, s->voxels, (float)ax, (float)ay, (float)az) : 0.0;
    if (s->volume) {
        const double floor_ = 0.0001;
        res = -log(floor_ > res ? floor_ : res);
    }
    return (res + (double)s->offset) * (double)s->scale;
}

/* value and dmean_da (GPFunctions.cpp:179-190): eps = 0.001 in double; mean(a + (eps, 0, 0)), (0, eps, 0), (0, 0, eps), then mean(a) */
void grid_ref_mean(const grid_slot *s, size_t n, const double *p3, double *value, double *grad3)
{
    const double eps = 0.001;
    for (size_t i = 0; i < n; ++i) {
        const double ax = p3[3 * i], ay = p3[3 * i + 1], az = p3[3 * i + 2];
        double vals[4];
        vals[0] = tab_mean(s, ax + eps, ay + 0.0, az + 0.0);
        vals[1] = tab_mean(s, ax + 0.0, ay + eps, az + 0.0);
        vals[2] = tab_mean(s, ax + 0.0, ay + 0.0, az + eps);
        vals[3] = tab_mean(s, ax, ay, az);
        if (value) value[i] = vals[3];
        if (grad3) {
            grad3[3 * i + 0] = (vals[0] - vals[3]) / eps;
            grad3[3 * i + 1] = (vals[1] - vals[3]) / eps;
            grad3[3 * i + 2] = (vals[2] - vals[3]) / eps;
        }
    }
}

size_t grid_ref_desc_size(void) { return sizeof(grid_desc); }
size_t grid_ref_slot_size(void) { return sizeof(grid_slot); }
