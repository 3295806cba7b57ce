/* ws_oracle.c — TEST INFRASTRUCTURE: a plain-C restatement of the reference's weight-space GP medium, for parity tests of the
 * gpis_ws_* entries (tests/test_gpu_ws.py) and the statistics check (tests/test_ws_cpu.py).  Built on demand by tests/ws_oracle.py.
 *
 * It follows the reference's serial code line by line, independently of the device's formulation (no jump-ahead, no batching):
 *   media/WeightSpaceGaussianProcessMedium.cpp:64-291     (WSM) sampleGradient, intersectGP
 *   math/WeightSpaceGaussianProcess.cpp:26-76, 120-240    (WSG) evaluate, evaluateGradient, basis and weight sampling
 *   media/GaussianProcessMedium.cpp:221-393               (GPM) sampleDistance, transmittance
 *   sampling/Gaussian.cpp:21-34, 104-119                  rand_normal_2, sample_standard_normal
 *   math/MathUtil.hpp:179-224, sampling/UniformSampler.hpp:22-53, math/BitManip.hpp:47-50   xxhash32, PCG32, normalizedUint
 * The Eigen reduction orders are those of the reference's vendored Eigen (csrc/gpis_ws.hpp names them).  The mean's "color" is
 * restated for the ramp noises (the ones gpis_ws_create accepts).
 * Compiled with the restatement flags of oracle/Makefile (SSE4.2, no FMA, no contraction) against the host libm. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "gpis.h"

#define WS_MAX_THREADS 16

typedef struct { double x, y, z; } v3d;
typedef struct { uint64_t state; } pcg32;

/* ---- integer layer ------------------------------------------------------------------------------------------------------- */
static uint32_t rotl17(uint32_t h) { return (h << 17) | (h >> 15); }
static uint32_t xx_final(uint32_t h)
{
    h = 2246822519U * (h ^ (h >> 15));
    h = 3266489917U * (h ^ (h >> 13));
    return h ^ (h >> 16);
}
uint32_t ws_xxhash32_4(const uint32_t p[4])            /* MathUtil::xxhash32(Vec4u) */
{
    const uint32_t P3 = 3266489917U, P4 = 668265263U, P5 = 374761393U;
    uint32_t h = p[3] + P5 + p[0] * P3;
    h = P4 * rotl17(h);
    h += p[1] * P3;
    h = P4 * rotl17(h);
    h += p[2] * P3;
    h = P4 * rotl17(h);
    return xx_final(h);
}
static uint32_t pcg_next(pcg32 *s)
{
    uint64_t old = s->state;
    s->state = old * 6364136223846793005ULL + 1ULL;
    uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((uint32_t)(-(int32_t)rot) & 31));
}
static float next1d(pcg32 *s)
{
    union { uint32_t u; float f; } v;
    v.u = (pcg_next(s) >> 9u) | 0x3F800000u;
    return v.f - 1.0f;
}
static void sampler_init(pcg32 *s, uint64_t seed)      /* UniformSampler(seed): state = seed, then next2D() */
{
    s->state = seed;
    (void)pcg_next(s);
    (void)pcg_next(s);
}
void ws_pcg32_stream(size_t n, const uint64_t *state, uint32_t count, uint32_t *out)   /* set_state + raw draws */
{
    for (size_t i = 0; i < n; ++i) {
        pcg32 s;
        sampler_init(&s, state[i]);
        for (uint32_t k = 0; k < count; ++k) out[i * count + k] = pcg_next(&s);
    }
}

/* ---- libm entries (which one a call reaches is part of the last bit: oracle/gpis_oracle.c explains) ------------------------ */
static __attribute__((noinline)) double libm_sin_alone(double x) { return sin(x); }
static __attribute__((noinline)) double libm_cos_alone(double x) { return cos(x); }
static __attribute__((noinline)) void libm_sin_and_cos(double x, double *sn, double *cs) { *sn = sin(x); *cs = cos(x); }

static const float PI_F = 3.1415926536f;
static void rand_normal_2(pcg32 *s, double *z1, double *z2)
{
    double u1 = next1d(s);
    double u2 = next1d(s);
    double r = sqrt(-2 * log(1. - u1));
    double x, y;
    libm_sin_and_cos(2 * PI_F * u2, &y, &x);
    *z1 = r * x;
    *z2 = r * y;
}
void ws_box_muller(uint64_t state, uint32_t pairs, double *out)
{
    pcg32 s;
    sampler_init(&s, state);
    for (uint32_t d = 0; d < pairs; ++d) rand_normal_2(&s, &out[2 * d], &out[2 * d + 1]);
}
static void sample_standard_normal(int n, pcg32 *s, double *out)
{
    for (int i = 0; i < n / 2; ++i) rand_normal_2(s, &out[2 * i], &out[2 * i + 1]);
    if (n % 2) {
        double y;
        rand_normal_2(s, &out[n - 1], &y);
    }
}

/* ---- model --------------------------------------------------------------------------------------------------------------- */
typedef struct {
    gpis_params P;
    gpis_ws_params S;
    double lin_dir[2][3];
    float sigma_s_over_t[3];
    int absorption_only;
} ws_model;

typedef struct {
    int n;
    double *d;          /* n x 3 */
    double *om, *ph, *w;
} ws_real;

static int model_init(ws_model *m, const gpis_params *P, const gpis_ws_params *S)
{
    if ((P->mean_color.enabled && P->mean_color.type >= GPIS_NOISE_SANDSTONE) || !(P->step_size > 0.f) || S->basis_functions < 0 || S->basis_functions > GPIS_WS_MAX_BASIS ||
        (S->normal_method != GPIS_NORMAL_CONDITIONED_GAUSSIAN && S->normal_method != GPIS_NORMAL_FINITE_DIFFERENCES))
        return -2;
    m->P = *P;
    m->S = *S;
    for (int w = 0; w < 2; ++w) {
        const gpis_mean *mu = w ? &P->mean_additional : &P->mean;
        double l2 = 0.; l2 += mu->dir[0] * mu->dir[0]; l2 += mu->dir[1] * mu->dir[1]; l2 += mu->dir[2] * mu->dir[2];
        double len = sqrt(l2), inv = len > 0 ? 1.0 / len : 0.0;
        for (int k = 0; k < 3; ++k) m->lin_dir[w][k] = mu->dir[k] * inv;
    }
    int all_zero = 1;
    for (int c = 0; c < 3; ++c) {          /* GPM.cpp:152-158 */
        float sa = P->sigma_a[c] * P->density, ss = P->sigma_s[c] * P->density;
        float st = sa + ss;
        m->sigma_s_over_t[c] = ss / st;
        if (ss != 0.0f) all_zero = 0;
    }
    m->absorption_only = all_zero;
    return 0;
}

static double v3d_length(v3d a) { double r = a.x * a.x; r += a.y * a.y; r += a.z * a.z; return sqrt(r); }

static double mean_eval(const ws_model *m, int w, v3d a)       /* GPF.hpp:887-889, 933-935, 992-994 */
{
    const gpis_mean *mu = w ? &m->P.mean_additional : &m->P.mean;
    if (mu->type == GPIS_MEAN_HOMOGENEOUS) return (double)mu->offset;
    if (mu->type == GPIS_MEAN_SPHERICAL) {
        v3d d = {a.x - mu->center[0], a.y - mu->center[1], a.z - mu->center[2]};
        return v3d_length(d) - (double)mu->radius;
    }
    double dx = a.x - mu->center[0], dy = a.y - mu->center[1], dz = a.z - mu->center[2];
    double dt = dx * m->lin_dir[w][0]; dt += dy * m->lin_dir[w][1]; dt += dz * m->lin_dir[w][2];
    double v = dt * (double)mu->scale, mn = (double)mu->min;
    return v > mn ? v : mn;
}
static v3d mean_grad(const ws_model *m, int w, v3d a)           /* dmean_da */
{
    const gpis_mean *mu = w ? &m->P.mean_additional : &m->P.mean;
    v3d z = {0., 0., 0.};
    if (mu->type == GPIS_MEAN_HOMOGENEOUS) return z;
    if (mu->type == GPIS_MEAN_SPHERICAL) {
        v3d d = {a.x - mu->center[0], a.y - mu->center[1], a.z - mu->center[2]};
        double inv = 1.0 / v3d_length(d);
        v3d r = {d.x * inv, d.y * inv, d.z * inv};
        return r;
    }
    double dx = a.x - mu->center[0], dy = a.y - mu->center[1], dz = a.z - mu->center[2];
    double dt = dx * m->lin_dir[w][0]; dt += dy * m->lin_dir[w][1]; dt += dz * m->lin_dir[w][2];
    if (dt * (double)mu->scale < (double)mu->min) return z;
    v3d r = {m->lin_dir[w][0] * (double)mu->scale, m->lin_dir[w][1] * (double)mu->scale, m->lin_dir[w][2] * (double)mu->scale};
    return r;
}
static void mean_weight_space(const ws_model *m, v3d p, double *mean, int *id)   /* GaussianProcess.cpp:379-393 */
{
    *mean = mean_eval(m, 0, p);
    *id = 0;
    if (m->P.has_mean_additional) {
        double add = mean_eval(m, 1, p);
        if (add < *mean) { *mean = add; *id = 1; }
    }
}
/* ProceduralNoise(Vec) of a ramp type, GPF.cpp:57-69, 91-103 (_const = 1, _scale = 1/(end - start), _offset = -start _scale) */
static double ramp_unit(double coord, double start, double end, double mn, double mx)
{
    const double c = 1.;
    double scale = 1.0 / (end - start), offset = -start * scale;
    double lo = mn + c, hi = mx + c;
    double u = coord * scale + offset;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    double a = log(lo * lo), b = log(hi * hi);
    double l = a * (1.0 - u) + b * u;
    return sqrt(exp(l));
}
static double ramp_eval(const gpis_ramp *r, v3d p)
{
    const double c = 1.;
    if (r->type == GPIS_RAMP_BOTTOM_TOP_LEFT_RIGHT) {       /* the two factors are narrowed to float */
        float bottomTop = (float)ramp_unit(p.y, r->start, r->end, r->min, r->max);
        float leftRight = (float)ramp_unit(p.x, r->start2, r->end2, r->min2, r->max2);
        return (double)(bottomTop * leftRight) - c * c;
    }
    double coord = r->type == GPIS_RAMP_BOTTOM_TOP ? p.y : (r->type == GPIS_RAMP_LEFT_RIGHT ? p.x : p.z);
    return ramp_unit(coord, r->start, r->end, r->min, r->max) - c;
}
static double cov_pp(const ws_model *m, v3d p)      /* squared exponential, GP form, at (p, p) */
{
    const double an[3] = {(double)m->P.aniso[0], (double)m->P.aniso[1], (double)m->P.aniso[2]};
    v3d d = {p.x - p.x, p.y - p.y, p.z - p.z};
    v3d ad = {an[0] * d.x, an[1] * d.y, an[2] * d.z};
    double absq = d.x * ad.x; absq += d.y * ad.y; absq += d.z * ad.z;
    const float s2 = m->P.sigma * m->P.sigma, l2 = m->P.length_scale * m->P.length_scale;
    return (double)s2 * exp(-absq / (double)(2 * l2));
}

/* ---- realization (WSG:160-240, serial) ---------------------------------------------------------------------------------------- */
static void pss_of(const ws_model *m, uint32_t px, uint32_t py, uint32_t spp, uint32_t seg, uint32_t pss[4])
{
    if (m->P.single_realization) { pss[0] = pss[1] = pss[2] = pss[3] = 0; return; }
    pss[0] = px; pss[1] = py; pss[2] = spp; pss[3] = m->P.correlation_context == GPIS_CTX_GLOBAL ? 0u : seg;
}
static void real_alloc(ws_real *r, int n)
{
    r->n = n;
    r->d = (double *)malloc(sizeof(double) * 3 * (size_t)(n ? n : 1));
    r->om = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1));
    r->ph = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1));
    r->w = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1));
}
static void real_free(ws_real *r) { free(r->d); free(r->om); free(r->ph); free(r->w); }
static void real_sample(const ws_model *m, const uint32_t pss[4], ws_real *r)
{
    const uint32_t h = ws_xxhash32_4(pss);
    pcg32 s;
    sampler_init(&s, (uint64_t)h);
    const float sa[3] = {sqrtf(m->P.aniso[0]), sqrtf(m->P.aniso[1]), sqrtf(m->P.aniso[2])};
    for (int i = 0; i < r->n; ++i) {
        r->ph[i] = next1d(&s) * (PI_F * 2.0f);
        double g[3];
        sample_standard_normal(3, &s, g);
        double v[3];
        for (int c = 0; c < 3; ++c) v[c] = (g[c] / (double)m->P.length_scale) * (double)sa[c];
        double l2 = v[0] * v[0]; l2 += v[1] * v[1]; l2 += v[2] * v[2];
        double len = sqrt(l2), inv = 1.0 / len;
        for (int c = 0; c < 3; ++c) r->d[3 * i + c] = v[c] * inv;
        r->om[i] = sqrt(l2);
    }
    pcg32 t;
    sampler_init(&t, (uint64_t)(uint32_t)(m->P.seed + h));
    sample_standard_normal(r->n, &t, r->w);
}

/* WeightSpaceRealization::evaluate (WSG:26-33, 120-127) */
static double real_eval(const ws_model *m, const ws_real *r, v3d p, int *id)
{
    double scale = sqrt(cov_pp(m, p));
    double mean;
    mean_weight_space(m, p, &mean, id);
    double basis = 0;
    if (r->n) {
        double result = 0;
        for (int i = 0; i < r->n; ++i) {
            double dot = (r->d[3 * i] * p.x + r->d[3 * i + 1] * p.y) + r->d[3 * i + 2] * p.z;
            result += r->w[i] * libm_cos_alone(dot * r->om[i] + r->ph[i]);
        }
        basis = result * sqrt(2. / r->n);
    }
    return scale * basis + mean;
}
static double det3(const double *m)
{
#define E(i, j) m[3 * (i) + (j)]
    return E(0, 0) * (E(1, 1) * E(2, 2) - E(1, 2) * E(2, 1)) - E(0, 1) * (E(1, 0) * E(2, 2) - E(1, 2) * E(2, 0)) + E(0, 2) * (E(1, 0) * E(2, 1) - E(1, 1) * E(2, 0));
}
static double cof3(const double *m, int i, int j)
{
    int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return E(i1, j1) * E(i2, j2) - E(i1, j2) * E(i2, j1);
#undef E
}
/* WeightSpaceRealization::evaluateGradient (WSG:50-76) */
static v3d real_grad(const ws_model *m, const ws_real *r, v3d p)
{
    double scale = sqrt(cov_pp(m, p));
    double g[3] = {0., 0., 0.};
    if (r->n) {
        for (int i = 0; i < r->n; ++i) {
            double dot = (r->d[3 * i] * p.x + r->d[3 * i + 1] * p.y) + r->d[3 * i + 2] * p.z;
            double s = -libm_sin_alone(dot * r->om[i] + r->ph[i]);
            for (int c = 0; c < 3; ++c) g[c] += ((r->d[3 * i + c] * r->om[i]) * r->w[i]) * s;
        }
        double f = sqrt(2. / r->n);
        for (int c = 0; c < 3; ++c) g[c] = g[c] * f;
    }
    for (int c = 0; c < 3; ++c) g[c] = scale * g[c];
    double eps = 0.0001, jac[9];
    do {
        double e[3][3] = {{p.x + eps, p.y + 0., p.z + 0.}, {p.x + 0., p.y + eps, p.z + 0.}, {p.x + 0., p.y + 0., p.z + eps}};
        for (int i = 0; i < 3; ++i) {
            jac[3 * i] = (e[i][0] - p.x) / eps;
            jac[3 * i + 1] = (e[i][1] - p.y) / eps;
            jac[3 * i + 2] = (e[i][2] - p.z) / eps;
        }
        eps *= 2;
    } while (det3(jac) < 0.0001);
    double c[9], t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = cof3(jac, i, j);
    double det = (c[0] * jac[0] + c[3] * jac[3]) + c[6] * jac[6];
    double invdet = 1.0 / det;
    for (int i = 0; i < 9; ++i) t[i] = c[i] * invdet;             /* inverse().transpose() */
    double bg[3];
    for (int i = 0; i < 3; ++i) bg[i] = (t[3 * i] * g[0] + t[3 * i + 1] * g[1]) + t[3 * i + 2] * g[2];
    double mean;
    int id;
    mean_weight_space(m, p, &mean, &id);
    v3d mg = mean_grad(m, id, p);
    v3d out = {bg[0] + mg.x, bg[1] + mg.y, bg[2] + mg.z};
    return out;
}
/* sampleGradient (WSM:64-156) */
static v3d sample_gradient(const ws_model *m, const ws_real *r, v3d p, uint64_t *n_eval)
{
    if (m->S.normal_method == GPIS_NORMAL_FINITE_DIFFERENCES) {
        float eps = 0.0001f;
        double e = eps;
        v3d ps[6] = {{p.x + e, p.y + 0., p.z + 0.}, {p.x + 0., p.y + e, p.z + 0.}, {p.x + 0., p.y + 0., p.z + e},
                     {p.x - e, p.y - 0., p.z - 0.}, {p.x - 0., p.y - e, p.z - 0.}, {p.x - 0., p.y - 0., p.z - e}};
        double v[6];
        int id;
        for (int i = 0; i < 6; ++i) v[i] = real_eval(m, r, ps[i], &id);
        *n_eval += 6;
        double den = (double)(2 * eps);
        v3d g = {(v[0] - v[3]) / den, (v[1] - v[4]) / den, (v[2] - v[5]) / den};
        return g;
    }
    *n_eval += 1;
    return real_grad(m, r, p);
}

static double lerp_d(double a, double b, double ratio) { return a * (1.0 - ratio) + b * ratio; }
static v3d at(v3d p, v3d rd, double t) { v3d r = {p.x + t * rd.x, p.y + t * rd.y, p.z + t * rd.z}; return r; }

/* intersectGP, step_size > 0 (WSM:236-290) */
static int intersect_gp(const ws_model *m, const ws_real *r, v3d p, v3d rd, float nearT, float farT, float u, int first_scatter,
                        double *t_out, int *last_gp_id, uint64_t *n_eval)
{
    float step_size = (farT - nearT) / (float)m->P.min_step;
    if (m->P.step_size < step_size) step_size = m->P.step_size;
    int gid;
    double t = nearT;
    double f0 = real_eval(m, r, at(p, rd, t), &gid);
    (*n_eval)++;
    int sign0 = f0 < 0 ? -1 : 1;
    double pf = f0;
    t = nearT + step_size * u;
    int step = 0;
    while (t < (double)farT) {
        step++;
        double fc = real_eval(m, r, at(p, rd, t), &gid);
        (*n_eval)++;
        int signc = fc < 0 ? -1 : 1;
        if (!first_scatter && step == 1) {
            sign0 = signc;
        } else if (signc != sign0) {
            double intp = pf / (pf - fc);
            double t_test, t_prev = lerp_d(t - step_size, t, intp);
            int tried = 0;
            for (;;) {
                t_test = lerp_d(t - step_size, t, intp);
                double ft = real_eval(m, r, at(p, rd, t_test), &gid);
                (*n_eval)++;
                if ((ft < 0 ? -1 : 1) == sign0) break;
                intp *= 0.9;
                if (intp <= 0.01 || ++tried >= 4096) {   /* 4096: the device's bound for a NaN factor (csrc/gpis_ws.hpp) */
                    t_prev = t_test = 0;
                    break;
                }
                t_prev = t_test;
            }
            *t_out = t_prev;
            *last_gp_id = gid;
            return 1;
        }
        pf = fc;
        t += step_size;
    }
    *t_out = farT;
    return 0;
}

typedef struct {
    const ws_model *m;
    const gpis_ray_in *rays;
    gpis_seg_out *out;
    uint8_t *visible;
    const gpis_ws_query *q;
    double *value, *grad3;
    int32_t *gp_id;
    const uint32_t *pss4;
    double *basis;
    size_t n, begin, end;
    uint64_t n_eval;
} job;

static void ray_setup(const gpis_ray_in *ray, v3d *ro, v3d *rd, v3d *rdn, float *farT)
{
    ro->x = ray->pos[0]; ro->y = ray->pos[1]; ro->z = ray->pos[2];
    rd->x = ray->dir[0]; rd->y = ray->dir[1]; rd->z = ray->dir[2];
    double l2 = rd->x * rd->x; l2 += rd->y * rd->y; l2 += rd->z * rd->z;
    double inv = 1.0 / sqrt(l2);
    rdn->x = rd->x * inv; rdn->y = rd->y * inv; rdn->z = rd->z * inv;
    *farT = ray->far_t;
    if (!isfinite(*farT)) *farT = (float)((double)ray->near_t + 2000);
}
/* GaussianProcessMedium::transmittance (GPM.cpp:343-393) */
static int transmittance_one(const ws_model *m, const ws_real *r, const gpis_ray_in *ray, int *first_scatter, int *last_gp_id, v3d *last_aniso,
                             uint64_t *n_eval)
{
    v3d ro, rd, rdn;
    float farT;
    ray_setup(ray, &ro, &rd, &rdn, &farT);
    const float maxT = farT;
    double startT = ray->near_t, t = maxT;
    int exited;
    do {
        exited = !intersect_gp(m, r, ro, rd, (float)startT, farT, ray->u_jitter, *first_scatter, &t, last_gp_id, n_eval);
        if (t < (double)maxT) {
            v3d g = sample_gradient(m, r, at(ro, rdn, t), n_eval);
            *last_aniso = g;
            *first_scatter = 0;
            if (!isfinite((g.x + g.y + g.z) / 3.0)) return 0;
        }
        startT = t;
    } while (t < (double)maxT && exited);
    return exited;
}
/* GaussianProcessMedium::sampleDistance (GPM.cpp:221-341) */
static void sample_distance_one(const ws_model *m, const ws_real *r, const gpis_ray_in *ray, gpis_seg_out *o, uint64_t *n_eval)
{
    memset(o, 0, sizeof *o);
    int first_scatter = ray->first_scatter != 0, last_gp_id = ray->last_gp_id;
    v3d last_aniso = {ray->last_aniso[0], ray->last_aniso[1], ray->last_aniso[2]};
    v3d ro, rd, rdn;
    float farT;
    ray_setup(ray, &ro, &rd, &rdn, &farT);
    const float maxT = farT;
    double startT = ray->near_t;
    o->gp_id = last_gp_id;
    o->last_val = ray->last_val;
    v3d aniso = last_aniso;
    int finished = 0;
    if (ray->bounce >= m->P.max_bounces) {
        o->ok = 0;
        finished = 1;
    } else if (maxT == 0.f) {
        o->sample_t = maxT;
        o->weight[0] = o->weight[1] = o->weight[2] = 1.f;
        o->exited = 1;
        for (int c = 0; c < 3; ++c) o->p[c] = ray->pos[c] + o->sample_t * ray->dir[c];
        o->scheme = GPIS_UNI;
        o->ok = 1;
        finished = 1;
    } else if (m->absorption_only) {
        if (maxT == INFINITY) {
            o->ok = 0;
            finished = 1;
        } else {
            o->sample_t = maxT;
            int vis = transmittance_one(m, r, ray, &first_scatter, &last_gp_id, &last_aniso, n_eval);
            o->weight[0] = o->weight[1] = o->weight[2] = vis ? 1.f : 0.f;
            o->exited = 1;
            o->scheme = GPIS_UNI;
            aniso = last_aniso;
        }
    } else {
        double t = maxT;
        int exited;
        do {
            exited = !intersect_gp(m, r, ro, rd, (float)startT, farT, ray->u_jitter, first_scatter, &t, &last_gp_id, n_eval);
            if (t < (double)maxT) {
                v3d g = sample_gradient(m, r, at(ro, rdn, t), n_eval);
                aniso = g;
                first_scatter = 0;
                if (!isfinite((aniso.x + aniso.y + aniso.z) / 3.0)) {
                    aniso.x = 1.; aniso.y = 0.; aniso.z = 0.;
                    o->t = t; o->exited = exited; o->ok = 0; o->gp_id = last_gp_id;
                    finished = 1;
                    break;
                }
            }
            startT = t;
        } while (t < (double)maxT && exited);
        if (!finished) {
            o->t = t;
            o->exited = exited;
            if (!exited) {
                double d = aniso.x * (double)ray->dir[0]; d += aniso.y * (double)ray->dir[1]; d += aniso.z * (double)ray->dir[2];
                double l2 = 0.; l2 += aniso.x * aniso.x; l2 += aniso.y * aniso.y; l2 += aniso.z * aniso.z;
                if (d > 0) {
                    o->gp_id = last_gp_id; o->ok = 0;
                    finished = 1;
                } else if (l2 < (double)0.0000001f) {
                    aniso.x = 1.; aniso.y = 0.; aniso.z = 0.;
                    o->gp_id = last_gp_id; o->ok = 0;
                    finished = 1;
                } else {                                                   /* _gp->color(ro + rd t), GPM.cpp:316 */
                    float col = m->P.mean_color.enabled ? (float)ramp_eval(&m->P.mean_color, at(ro, rdn, t)) : 1.f;
                    o->weight[0] = o->weight[1] = o->weight[2] = col;
                    o->continued_weight[0] = o->continued_weight[1] = o->continued_weight[2] = col;
                }
            } else {
                aniso = sample_gradient(m, r, at(ro, rdn, t), n_eval);      /* GPM.cpp:319 */
                o->weight[0] = o->weight[1] = o->weight[2] = 1.f;
                o->continued_weight[0] = o->continued_weight[1] = o->continued_weight[2] = 1.f;
            }
            if (!finished) {
                float ft = (float)t;
                o->sample_t = ft < maxT ? ft : maxT;
                o->continued_t = (float)t;
                for (int c = 0; c < 3; ++c) {
                    o->weight[c] *= m->sigma_s_over_t[c];
                    o->continued_weight[c] *= m->sigma_s_over_t[c];
                }
                o->scheme = GPIS_UNI;
            }
        }
    }
    if (!finished) {
        for (int c = 0; c < 3; ++c) o->p[c] = ray->pos[c] + o->sample_t * ray->dir[c];
        o->gp_id = last_gp_id;
        o->ok = 1;
    }
    o->aniso[0] = aniso.x; o->aniso[1] = aniso.y; o->aniso[2] = aniso.z;
}

static void *run_job(void *arg)
{
    job *J = (job *)arg;
    const ws_model *m = J->m;
    ws_real r;
    real_alloc(&r, m->S.basis_functions);
    for (size_t i = J->begin; i < J->end; ++i) {
        uint32_t pss[4];
        if (J->rays) {
            const gpis_ray_in *ray = &J->rays[i];
            pss_of(m, ray->pixel[0], ray->pixel[1], ray->spp, ray->segment, pss);
            real_sample(m, pss, &r);
            if (J->out) {
                sample_distance_one(m, &r, ray, &J->out[i], &J->n_eval);
            } else {
                int fs = ray->first_scatter != 0, gid = ray->last_gp_id;
                v3d la = {ray->last_aniso[0], ray->last_aniso[1], ray->last_aniso[2]};
                J->visible[i] = (uint8_t)transmittance_one(m, &r, ray, &fs, &gid, &la, &J->n_eval);
            }
        } else if (J->q) {
            const gpis_ws_query *q = &J->q[i];
            pss_of(m, q->pixel[0], q->pixel[1], q->spp, q->segment, pss);
            real_sample(m, pss, &r);
            v3d p = {q->p[0], q->p[1], q->p[2]};
            int id;
            double v = real_eval(m, &r, p, &id);
            v3d g = sample_gradient(m, &r, p, &J->n_eval);
            if (J->value) J->value[i] = v;
            if (J->gp_id) J->gp_id[i] = id;
            if (J->grad3) { J->grad3[3 * i] = g.x; J->grad3[3 * i + 1] = g.y; J->grad3[3 * i + 2] = g.z; }
        } else {
            const uint32_t *w = J->pss4 + 4 * i;
            pss_of(m, w[0], w[1], w[2], w[3], pss);
            real_sample(m, pss, &r);
            for (int k = 0; k < r.n; ++k) {
                double *o = J->basis + ((size_t)i * r.n + k) * 6;
                o[0] = r.d[3 * k]; o[1] = r.d[3 * k + 1]; o[2] = r.d[3 * k + 2];
                o[3] = r.om[k]; o[4] = r.ph[k]; o[5] = r.w[k];
            }
        }
    }
    real_free(&r);
    return NULL;
}
static int run(const gpis_params *P, const gpis_ws_params *S, job proto, int threads, uint64_t *n_eval)
{
    ws_model m;
    if (model_init(&m, P, S)) return -2;
    if (threads < 1) threads = 1;
    if (threads > WS_MAX_THREADS) threads = WS_MAX_THREADS;
    if ((size_t)threads > proto.n) threads = proto.n ? (int)proto.n : 1;
    pthread_t th[WS_MAX_THREADS];
    job jobs[WS_MAX_THREADS];
    for (int k = 0; k < threads; ++k) {
        jobs[k] = proto;
        jobs[k].m = &m;
        jobs[k].begin = proto.n * (size_t)k / (size_t)threads;
        jobs[k].end = proto.n * (size_t)(k + 1) / (size_t)threads;
        jobs[k].n_eval = 0;
        pthread_create(&th[k], NULL, run_job, &jobs[k]);
    }
    uint64_t total = 0;
    for (int k = 0; k < threads; ++k) {
        pthread_join(th[k], NULL);
        total += jobs[k].n_eval;
    }
    if (n_eval) *n_eval = total;
    return 0;
}

/* ---- entry points (ctypes) ----------------------------------------------------------------------------------------------------- */
int ws_oracle_sample_distance(const gpis_params *P, const gpis_ws_params *S, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, int threads,
                              uint64_t *n_eval)
{
    job j;
    memset(&j, 0, sizeof j);
    j.rays = rays; j.out = out; j.n = n;
    return run(P, S, j, threads, n_eval);
}
int ws_oracle_transmittance(const gpis_params *P, const gpis_ws_params *S, size_t n, const gpis_ray_in *rays, uint8_t *visible, int threads,
                            uint64_t *n_eval)
{
    job j;
    memset(&j, 0, sizeof j);
    j.rays = rays; j.visible = visible; j.n = n;
    return run(P, S, j, threads, n_eval);
}
int ws_oracle_eval(const gpis_params *P, const gpis_ws_params *S, size_t n, const gpis_ws_query *q, double *value, double *grad3, int32_t *gp_id,
                   int threads)
{
    job j;
    memset(&j, 0, sizeof j);
    j.q = q; j.value = value; j.grad3 = grad3; j.gp_id = gp_id; j.n = n;
    return run(P, S, j, threads, NULL);
}
int ws_oracle_basis(const gpis_params *P, const gpis_ws_params *S, size_t n, const uint32_t *pss4, double *out, int threads)
{
    job j;
    memset(&j, 0, sizeof j);
    j.pss4 = pss4; j.basis = out; j.n = n;
    return run(P, S, j, threads, NULL);
}
size_t ws_oracle_sizes(int which) { return which == 0 ? sizeof(gpis_ws_params) : sizeof(gpis_ws_query); }
