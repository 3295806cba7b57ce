/*
 * gpis.h — C ABI of the MI355X-native sparse-convolution GPIS hot path.
 *
 * This is the drop-in boundary: the entry points below are what a binding in the
 * reference (a `Medium` subclass registered in MediumFactory.cpp:13-22) would call in
 * place of the CPU code in
 *   src/core/media/SparseConvolutionNoiseMedium.cpp   (SCNM.cpp)
 *   src/core/media/GaussianProcessMedium.cpp          (GPM.cpp)
 *   src/core/math/SparseConvolutionNoise.cpp          (SCN.cpp)
 *   src/core/math/GPFunctions.cpp                     (GPF.cpp)
 * Plain pointers and sizes only; no C++ types, no torch types, no exceptions.
 *
 * Memory convention: every `*_batch` entry takes DEVICE pointers (hipMalloc'd, or a
 * torch tensor's data_ptr) and enqueues on `stream` (a hipStream_t passed as void*,
 * NULL = the null stream).  The resident-kernel form of the march (the default) never
 * synchronises; the wavefront form (GPIS_ORDER_SCATTERED with a guide field, or
 * GPIS_MARCH_FORM_WAVE) synchronises `stream` once per step/sort/evaluate iteration to read
 * how many rays are left.  The `*_host` variants take HOST pointers, stage through an
 * internal device workspace and synchronise before returning — they are what a
 * batch-of-one `Medium` adapter uses.
 *
 * Threading: a handle may be used from several host threads on distinct streams, as Tungsten's
 * render workers use one `const Medium`.  Entry points serialise on a per-handle
 * mutex while they ENQUEUE (kernels of different callers still overlap on the device); the
 * workspaces the handle owns (tile drivers, wavefront march) are handed from one caller's stream
 * to the next with an event, so a second caller never overwrites a workspace still in use.
 * The `*_host` entries are the exception: they hold the mutex END TO END (upload, kernel, event
 * wait, download) because the two staging slots are state of the handle — concurrent batch-of-one
 * callers of one handle (Tungsten's render workers through the Medium adapter) are served one
 * after the other, 150 us each.  That path is a compatibility path, not a throughput path:
 * a renderer that wants the GPU busy batches its rays.  The function-space
 * host entries serialise the same way on their own lock.
 * gpis_destroy / gpis_build_guide / gpis_drop_guide must not race with other calls on the handle.
 *
 * Environment: a few diagnostic overrides are read ONCE, in gpis_create, as the initial values
 * of the options below and of the cell table: GPIS_MARCH=resident|wave, GPIS_WAVE_TAIL=<rays>,
 * GPIS_PATHS_SORT=0, GPIS_PATHS_PRESORT=0, GPIS_CHUNK_LOG2=<16..28>, GPIS_DISABLE_FAST=1,
 * GPIS_DISABLE_TABLE=1, GPIS_TABLE_HALF_EXTENT=<cells>, GPIS_PERSIST=0, GPIS_SOLO_MAX=<lanes>, GPIS_RANGE_LEN=<rays>.  Nothing is read from
 * the environment after gpis_create.  Results never depend on any of them.
 *
 * All functions return GPIS_OK (0) or a negative gpis_status; gpis_last_error()
 * returns a thread-local message for the last failure.
 */
#ifndef GPIS_H_
#define GPIS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPIS_ABI_VERSION 3

typedef enum gpis_status {
    GPIS_OK = 0,
    GPIS_ERR_INVALID_ARG = -1,   /* bad pointer / size / enum */
    GPIS_ERR_UNSUPPORTED = -2,   /* a parameter combination outside the built scope */
    GPIS_ERR_DEVICE = -3,        /* HIP runtime error (message in gpis_last_error) */
    GPIS_ERR_NO_DEVICE = -4      /* no gfx950 device / extension cannot run */
} gpis_status;

/* GPCorrelationContext, src/core/math/GaussianProcess.hpp:26-31 (same numeric order). */
typedef enum gpis_corr_ctx {
    GPIS_CTX_GLOBAL = 0,
    GPIS_CTX_RENEWAL_PLUS = 1,
    GPIS_CTX_RENEWAL = 2,
    GPIS_CTX_NONE = 3
} gpis_corr_ctx;

/* SparseConv1DSamplingScheme, src/core/media/Medium.hpp:40-44. */
typedef enum gpis_scheme_1d { GPIS_UNI = 0, GPIS_NEE = 1, GPIS_MIS = 2 } gpis_scheme_1d;

/* Mean functions, src/core/math/GPFunctions.hpp:867-1087. */
typedef enum gpis_mean_type {
    GPIS_MEAN_HOMOGENEOUS = 0,   /* offset                       GPF.hpp:867-901  */
    GPIS_MEAN_SPHERICAL = 1,     /* |p-c| - r                    GPF.hpp:903-945  */
    GPIS_MEAN_LINEAR = 2,        /* max((p-ref).dir*scale, min)  GPF.hpp:947-1005 */
    GPIS_MEAN_PROCEDURAL = 3,    /* max(min, sdf(T^-1 p)*scale + offset)  GPF.hpp:1049-1087, GPF.cpp:250-296 */
    GPIS_MEAN_TABULATED = 4      /* (grid(W p) + offset)*scale, W = world -> index; "volume": -log(max(1e-4, grid))  GPF.hpp:1007-1025, GPF.cpp:143-194 */
} gpis_mean_type;

/* SdfFunctions::Function (math/SdfFunctions.hpp:12-18, same numeric order): the shape of a procedural mean, "func". */
typedef enum gpis_sdf_function {
    GPIS_SDF_KNOB = 0,
    GPIS_SDF_KNOB_INNER = 1,
    GPIS_SDF_KNOB_OUTER = 2,
    GPIS_SDF_TWO_SPHERES = 3,
    GPIS_SDF_PLANE = 4
} gpis_sdf_function;

/* NoiseType of ProceduralNoise / ProceduralNoiseVec (GPF.hpp:613-650, 702-739): the four ramps (GPF.cpp:57-69, 91-103) and
 * the two fbm noises over 3D simplex noise (GPF.cpp:70-83, 104-117; math/SdfFunctions.cpp:199-296). */
typedef enum gpis_ramp_type {
    GPIS_RAMP_BOTTOM_TOP = 0,    /* along y */
    GPIS_RAMP_LEFT_RIGHT = 1,    /* along x */
    GPIS_RAMP_FRONT_BACK = 2,    /* along z */
    GPIS_RAMP_BOTTOM_TOP_LEFT_RIGHT = 3,  /* product of a y ramp and an x ramp ("min2".."end2"), GPF.cpp:96-103 */
    GPIS_NOISE_SANDSTONE = 4,    /* "sandstone": three nested fbm, scalar fields lerp(min, max, .), vector fields clamp(0.2 col) */
    GPIS_NOISE_RUST = 5          /* "rust": smoothStep(0.4, 0.6, fbm -/+ 0.1 fbm(25 p)), scalar lerp(min, max, .), vector lerp((0.278, 0.212, 0.141), 1, .) */
} gpis_ramp_type;

/* A procedural field of type "noise" (ProceduralNoise / ProceduralNoiseVec, GPF.hpp:596-776, GPF.cpp:43-138).  Used for the
 * scalar fields "var" (variance) and "aniso" (ProceduralNoise: 2 fbm octaves) and for the vector fields "ls" (the kernel scale
 * is the largest component, GPF.cpp:1729-1735) and the mean's "color" / "emission" (ProceduralNoiseVec: 10 octaves; the three
 * components are equal for the ramp noises and differ for sandstone / rust).  On the device `sin` / `sqrt` of the fbm hash are
 * ocml's, not glibc's: values agree with the CPU to the stated tolerance, not bit for bit. */
typedef struct gpis_ramp {
    int32_t enabled;
    int32_t type;                    /* gpis_ramp_type */
    double min, max, start, end;     /* "min", "max", "start", "end"      (defaults 1, 500, 0, 1) */
    double min2, max2, start2, end2; /* "min2", "max2", "start2", "end2"  (bottom_top_left_right) */
} gpis_ramp;

/* Stationary covariance kernels with a sparse-convolution splatting kernel (GPF.cpp).  Matérn with v = 1.5 needs Boost's
 * cyl_bessel_k (GPF.cpp:1055, 1073), which is neither vendored nor installed: outside the built scope.  Matérn / Gabor kernels
 * define no isotropic-space transform, no 1D kernel and no second derivative (GPF.hpp:2002-2110), so they are accepted for
 * world-space 3D sampling with correlation context none / global / renewal. */
typedef enum gpis_kernel_type {
    GPIS_KERNEL_SQUARED_EXPONENTIAL = 0,   /* GPF.cpp:654-865 */
    GPIS_KERNEL_MATERN = 1,                /* "matern": "sigma", "v" (0.5 or 2.5), "lengthScale", "aniso"     GPF.cpp:866-1082 */
    GPIS_KERNEL_GABOR_ANISO = 2,           /* "gabor_aniso": "sigma", "a_inv", "f_inv", "omega"               GPF.cpp:1086-1150 */
    GPIS_KERNEL_GABOR_ISO = 3              /* "gabor_iso": "sigma", "a_inv", "f_inv"                          GPF.cpp:1155-1214 */
} gpis_kernel_type;

typedef struct gpis_mean {
    int32_t type;          /* gpis_mean_type */
    float radius;          /* spherical */
    float offset;          /* homogeneous; procedural "offset"; tabulated "offset" (JSON default 0) */
    float scale;           /* linear; procedural "scale"; tabulated "scale" (JSON default 1) */
    float min;             /* linear, procedural (default -FLT_MAX) */
    int32_t func;          /* procedural: gpis_sdf_function; tabulated: != 0 is the "volume" flag (the field is reused, as the
                              procedural mean reused the former padding word); not read for the other types */
    double center[3];      /* spherical centre / linear reference_point */
    double dir[3];         /* linear direction (normalised by gpis_create as LinearMean::fromJson does) */
} gpis_mean;
/* A procedural mean is ProceduralMean over one of the reference's SDF shapes: mean(a) = max(min, sdf(T^-1 . float(a)) * scale + offset)
 * in float, widened; dmean_da is the reference's one-sided difference with eps = 0.001f, evaluated in the order a, +x, +y, +z
 * (GPF.cpp:279-296).  T is the mean's "transform" (identity until gpis_set_mean_transform).  Scalar-field objects ("f") are
 * outside the built scope.
 *
 * A tabulated mean is TabulatedMean over a dense voxel grid (gpis_set_mean_grid; the descriptor and the lookup are those of
 * gpis_variance_grid below): res = double(density(W . float(a))) with W the grid's world -> index transform; with "volume"
 * (func != 0) res = -log(max(0.0001, res)) in double; mean(a) = (res + offset) * scale in double — NOT the procedural
 * sdf * scale + offset.  dmean_da is the one-sided difference with the double eps = 0.001, evaluated in the order +x, +y, +z, a
 * (GPF.cpp:165-190).  It reads offset, scale and func only.  Until a grid is set the density is 0, the background of an empty
 * tree.  Its colour field is evaluated at a itself; its emission is the grid's (GPF.cpp:174-177), and emission, detail and
 * temperature grids are outside the built scope: a medium whose PRIMARY mean is tabulated emits 0 whatever its mean_emission
 * field says.  The "quadratic" sampler is refused; sparse VDB files are read by the loader, which hands over a dense array.
 *
 * Where such media run: either type, in either slot of the CSG pair, is served by the sparse-convolution medium (gpis_create) on
 * the lane-per-ray all-features path instance — all gpis_render_scene_s* frame drivers, their adaptive entries, the batch entry
 * points.  GPIS_OPT_PERSISTENT has no effect on them; there is no fast table, no wavefront and no persistent form, and
 * gpis_build_guide refuses them (GPIS_ERR_UNSUPPORTED).  The function-space entries (gpis_fs_*) refuse them with
 * GPIS_ERR_UNSUPPORTED and gpis_ws_create (the weight-space medium) with GPIS_ERR_INVALID_ARG, each with a message that names the
 * mean. */

/*
 * All JSON keys of the hot path (SURVEY.md §5 "Config / flags"):
 *   medium:      SCNM.cpp:57-73, GPM.cpp:97-126, Medium.cpp:37
 *   covariance:  GPF.cpp:654-679 (squared_exponential), GPF.hpp:1481-1484 (localScale),
 *                GPF.hpp:1134-1137 (lateralScale)
 *   wrapper:     GPF.hpp:2211-2217 + GPF.cpp:1590-1606 (proc_nonstationary: ls ramp, multiResolutionGrid)
 */
typedef struct gpis_params {
    uint32_t abi_version;            /* must be GPIS_ABI_VERSION */
    /* --- sparse_conv_noise medium --- */
    float step_size;                 /* "step_size"  default 0.01 */
    uint32_t min_step;               /* "min_step"   default 8 */
    uint32_t seed;                   /* "seed"       _globalSeed */
    float impulse_density;           /* "impulse_density" */
    int32_t single_realization;      /* "single_realization" */
    int32_t isotropic_3d_sampling;   /* "isotropic_3D_sampling" (iso-RAY space: SCN.cpp:17 hard-wires it) */
    int32_t sampling_1d;             /* "1D_sampling" */
    int32_t scheme_1d;               /* "1D_sampling_scheme" gpis_scheme_1d */
    int32_t correlation_xy;          /* "1D_gradient_correlationXY" */
    int32_t surf_vol_phase_separate; /* "surf_vol_phase_separate" */
    float surf_vol_phase_amp_thresh; /* "surf_vol_phase_amp_thresh" */
    /* --- gaussian_process medium base --- */
    int32_t correlation_context;     /* "correlation_context" gpis_corr_ctx (required) */
    int32_t max_bounces;             /* "max_bounces" default 1024 */
    float sigma_a[3];                /* "sigma_a" */
    float sigma_s[3];                /* "sigma_s" */
    float density;                   /* "density" */
    /* --- squared_exponential covariance --- */
    float sigma;                     /* "sigma" */
    float length_scale;              /* "lengthScale" */
    float aniso[3];                  /* "aniso" */
    int32_t use_aniso_mtx;           /* "useAnisoMtx" */
    float aniso_mtx[9];              /* "anisoMtx" row-major, used when use_aniso_mtx */
    float local_scale;               /* "localScale" (_kernelScale, default 3) */
    /* --- proc_nonstationary wrapper (0 = plain stationary kernel) --- */
    int32_t nonstationary;           /* 1: ProceduralNonstationaryCovariance with an "ls" ramp */
    int32_t multi_resolution_grid;   /* "multiResolutionGrid" */
    int32_t ls_ramp_type;            /* gpis_ramp_type */
    int32_t _pad0;
    double ls_min, ls_max;           /* ramp "min","max" */
    double ls_start, ls_end;         /* ramp "start","end" */
    /* --- mean(s) --- */
    gpis_mean mean;                  /* GaussianProcess::_mean,  _id = 0 */
    int32_t has_mean_additional;     /* GaussianProcess::_mean_additional (CSG min), _id_additional = 1 */
    int32_t _pad1;
    gpis_mean mean_additional;
    /* --- rest of the proc_nonstationary wrapper and of the mean (GPF.cpp:1590-1606, GPF.hpp:803-862) --- */
    double ls_min2, ls_max2;         /* second ramp of an "ls" field of type bottom_top_left_right */
    double ls_start2, ls_end2;
    gpis_ramp var;                   /* "var": getVariance(p) (GPF.cpp:1638-1641); the noise amplitude becomes var(p) * sigma (GPF.cpp:1235-1237) */
    gpis_ramp mean_color;            /* mean "color":    MediumSample.weight *= color(p) on a hit (GPM.cpp:316) */
    gpis_ramp mean_emission;         /* mean "emission": MediumSample.emission (GPM.cpp:317) — gpis_mean_color_emission_* */
    /* --- other stationary kernels (sigma / length_scale / aniso above are shared) --- */
    int32_t kernel_type;             /* gpis_kernel_type */
    float matern_v;                  /* "v" */
    float gabor_a_inv, gabor_f_inv;  /* "a_inv", "f_inv" (the reference stores a = 1/a_inv, f = 1/f_inv) */
    float gabor_omega[3];            /* "omega" (normalised at construction, GPF.cpp:1095) */
    int32_t _pad2;
    /* --- "aniso" field of proc_nonstationary (GPF.cpp:1600-1602): an angle in units of pi/2 that turns the in-plane anisotropy
     *     (axis ratio 1.5 : 1/1.5 : 1, hard-coded in the reference, GPF.hpp:2372) of the splatting kernel about z
     *     (getNonstationaryAniso3D, GPF.cpp:1678-1689).  Built for 3D sampling (world and isotropic-ray space); with 1D sampling
     *     the medium is refused (getNonstationaryAniso1D / ...CovSplatCov1D, GPF.cpp:1691-1727, are outside the built scope). --- */
    gpis_ramp aniso_field;
    /* --- FunctionSpaceGaussianProcessMedium (FunctionSpaceGaussianProcessMedium.cpp:34-43): read by the
     *     gpis_fs_* entry points only.  "skip_space" = 0 and "step_size_cov" (dead code in the reference, :98-106) are not carried. --- */
    int32_t fs_sample_points;        /* "sample_points" (2 .. GPIS_FS_MAX_POINTS; the reference's default is 32) */
    int32_t _pad3;
    double fs_step_size;             /* "step_size" of the function-space medium (0 = the whole segment in one batch of points) */
    /* --- GridNonstationaryCovariance (GPF.cpp:1326-1427; needs nonstationary = 1): the variance comes from a voxel grid
     *     (gpis_set_variance_grid; 1 until one is set, GPF.cpp:1386-1391) and the kernel scale from a threshold on it.  The "ls",
     *     "var" and "aniso" fields of the procedural wrapper are not read in this flavour. --- */
    int32_t grid_nonstationary;      /* 1: this flavour of the non-stationary wrapper */
    int32_t grid_surf_vol_amp_separate; /* "surf_vol_amp_separate" */
    float grid_offset, grid_scale;   /* "offset", "scale": (density + offset) * scale */
    float grid_surf_vol_amp_thresh;  /* "surf_vol_amp_thresh" */
    float grid_surf_amp_scale, grid_vol_amp_scale;   /* "surf_amp_scale", "vol_amp_scale" */
    float grid_surf_ls_scale, grid_vol_ls_scale;     /* "surf_ls_scale", "vol_ls_scale" */
    int32_t _pad4;
} gpis_params;

/* The voxel grid of a GridNonstationaryCovariance, as a dense array: what VdbGrid::density(p) (VdbGrid.cpp:405-431) returns for
 * an index-space point — p clamped to [bounds_min + 2, bounds_max - 3], then OpenVDB's PointSampler (interpolate 0) or BoxSampler
 * (1: trilinear, weights in double, each stage narrowed to float).  OpenVDB is not vendored by the reference and absent here: the
 * two samplers are restated from its published source (tools/Interpolation.h); PARITY UNPINNED for this lookup.  "quadratic" is
 * refused.  voxel (i, j, k) of the index-space box origin + [0, dims) is voxels[i + dims[0] * (j + dims[1] * k)]; anything
 * outside it is 0 (the tree's background). */
typedef struct gpis_variance_grid {
    int32_t dims[3];
    int32_t interpolate;             /* 0 "point", 1 "linear" */
    int32_t origin[3];               /* index-space coordinate of voxel (0, 0, 0) */
    int32_t _pad;
    float bounds_min[3], bounds_max[3];   /* VdbGrid::bounds() (index space) */
    float inv_natural_transform[16]; /* row-major Mat4f, world -> index space (VdbGrid::invNaturalTransform) */
} gpis_variance_grid;
/* (set with gpis_set_variance_grid, declared with the other entry points below) */

/* The function-space comparison path (FunctionSpaceGaussianProcessMedium.cpp:58-282): the field is sampled at `sample_points`
 * positions of the segment from the multivariate normal the GP prior (or its conditional, given the previous segment's
 * values) defines there — covariance build, pseudo-inverse through a symmetric eigen-decomposition, Cholesky (or the
 * eigen square root when it fails), GaussianProcess.cpp:590-753, Gaussian.cpp:121-232.
 * Built for: squared-exponential covariance in its GP form (sigma^2 exp(-d^T diag(aniso) d / (2 l^2)), GPF.hpp:1602-1605,
 * GPF.cpp:770-772), the analytic means, all four correlation contexts, normal sampling "ConditionedGaussian".
 *
 * gpis_fs_state = the caller-owned MediumState part this medium adds: state.gpContext (GPContextFunctionSpace,
 * GaussianProcessMedium.hpp:23-33: points, derivative kinds and the GPRealNodeValues) and the path's PathSampleGenerator
 * (a PCG32 stream, UniformPathSampler), from which the medium draws an unbounded number of variates.  It is a VALUE: a shadow
 * segment works on a copy and never alters the path's context (in the reference the copy of MediumState shares the
 * GPRealNode, which applyMemory mutates in place, GaussianProcess.cpp:134-168). */
#define GPIS_FS_MAX_POINTS 64
#define GPIS_FS_MAX_CTX 66
typedef struct gpis_fs_state {
    uint64_t sampler_state;          /* PCG32 state (UniformSampler.hpp:41-75) */
    int32_t has_context;             /* state.gpContext != nullptr */
    int32_t is_intersect;            /* GPRealNodeValues::_isIntersect */
    int32_t n_points;                /* ctxt->points.size() */
    int32_t n_values;                /* ctxt->values rows (differs from n_points only transiently) */
    double sampled_grad[3];          /* GPRealNodeValues::_sampledGrad */
    double points[GPIS_FS_MAX_CTX][3];
    double values[GPIS_FS_MAX_CTX];
    int32_t derivs[GPIS_FS_MAX_CTX]; /* 0 = Derivative::None, 1 = Derivative::First */
} gpis_fs_state;

/*
 * One ray segment handed to Medium::sampleDistance / Medium::transmittance
 * (Medium.hpp:104-108): the Ray (math/Ray.hpp), the caller-owned Medium::MediumState
 * (Medium.hpp:59-88) and RayInfo (MediumSample.hpp:14-18), plus the single
 * PathSampleGenerator::next1D() the path consumes (SCNM.cpp:129).  128 bytes.
 */
typedef struct gpis_ray_in {
    float pos[3];
    float dir[3];
    float near_t;
    float far_t;              /* may be +inf: clamped to near_t+2000 (GPM.cpp:229-231) */
    uint32_t pixel[2];        /* info.pixelSampleSegment.xy */
    uint32_t spp;             /* info.pixelSampleSegment.z  */
    uint32_t segment;         /* info.pixelSampleSegment.w  (bounce index, PathTracer.cpp:64) */
    uint32_t scene_seed;      /* info.sceneSeed */
    float info_t;             /* info.t */
    float u_jitter;           /* sampler.next1D() */
    uint32_t first_scatter;   /* state.firstScatter */
    int32_t bounce;           /* state.bounce */
    float last_val;           /* state.lastVal */
    int32_t last_gp_id;       /* state.lastGPId */
    int32_t _pad;
    double last_aniso[3];     /* state.lastAniso */
    double _reserved[3];
} gpis_ray_in;

/*
 * Result of one sampleDistance call: the MediumSample fields the path writes
 * (GPM.cpp:224-340) and the MediumState updates the caller must apply:
 *   state.lastAniso = aniso; state.lastVal = last_val; state.lastGPId = gp_id;
 *   state.firstScatter = false (when gradient_sampled); state.bounce++; state.info.t += sample_t.
 * 96 bytes.
 */
typedef struct gpis_seg_out {
    double t;                 /* intersect t (double, SCNM.cpp:102) */
    double aniso[3];          /* sample.aniso = sampled gradient */
    float sample_t;           /* sample.t = min(float(t), maxT) */
    float continued_t;        /* sample.continuedT */
    float weight[3];          /* sample.weight */
    float continued_weight[3];
    float p[3];               /* sample.p */
    float last_val;           /* state.lastVal after the call */
    int32_t exited;           /* sample.exited */
    int32_t ok;               /* return value of sampleDistance (0 → caller terminates the path) */
    int32_t gp_id;            /* sample.gpId */
    int32_t scheme;           /* sample.sparseConv1DSamplingScheme */
} gpis_seg_out;

/*
 * The realization handle MediumSample.ctxt points to (GPContextSparseConvNoise,
 * SparseConvolutionNoiseMedium.hpp:11-16) reduced to its mutable part: the
 * pathwise-update conditioning coefficients (SCN.hpp:7-21).  32 bytes.
 */
typedef struct gpis_cond_coeff {
    float value_scale;
    float gradient_scale[3];
    float ray_origin[3];
    uint32_t n_evals;         /* noise evaluations spent on this segment (diagnostic) */
} gpis_cond_coeff;

/*
 * A single noise query: SparseConvolutionNoiseRealization::evaluateValue /
 * evaluateGradient (SCN.cpp:73-99) — unit-test surface.  `t_segment` is the
 * `t` argument (distance along the current segment); `info_t` is RayInfo::t.  96 bytes.
 */
typedef struct gpis_query {
    float p[3];
    float dir[3];
    float t_segment;
    float info_t;
    uint32_t pixel[2];
    uint32_t spp;
    uint32_t segment;
    uint32_t scene_seed;
    uint32_t _pad[3];
    gpis_cond_coeff coeff;    /* conditioning state to evaluate under (all-zero = unconditioned) */
} gpis_query;

/* Input of neePDF / neeGrad (SCN.cpp:652-743). 96 bytes. */
typedef struct gpis_nee_query {
    float ray_dir[3];
    float normal[3];
    float p[3];
    float t_segment;          /* neePDF's `tSegment` */
    float info_t;
    uint32_t pixel[2];
    uint32_t spp;
    uint32_t segment;
    uint32_t scene_seed;
    gpis_cond_coeff coeff;
} gpis_nee_query;

typedef struct gpis_medium gpis_medium;   /* opaque handle */

/* Derived constants the path precomputes once (GPF.cpp:654-679, 696-709, 741-760);
 * exposed so tests can pin them against the oracle. */
typedef struct gpis_derived {
    float world_to_local[9];   /* row-major */
    float local_to_world[9];
    float kernel_radius_world; /* splattingKernelRadius(false, 1) */
    float kernel_radius_iso;   /* splattingKernelRadius(true, 1)  */
    float norm3d_world;        /* sqrt(sparseConvNoiseVariance3D(world)) at scale 1; 0 for non-stationary media (position dependent) */
    float norm3d_iso;          /* sqrt(sparseConvNoiseVariance3D(iso)); 0 for non-stationary media */
    float norm1d;              /* sqrt(sparseConvNoiseVariance1D); 0 for non-stationary media */
    uint32_t impulses_per_cell;
    int32_t activate_conditioning; /* SCN.cpp:21 */
    int32_t effective_scheme_1d;   /* SCN.cpp:23-26 */
    int32_t multi_resolution;      /* SCN.cpp:30 */
    int32_t fast_path;             /* 1 when the single-realization cell-table kernels are in use */
} gpis_derived;

/* ---- lifetime ------------------------------------------------------------------- */

/* Replaces SparseConvolutionNoiseMedium::fromJson + prepareForRender
 * (SCNM.cpp:57-73, GPM.cpp:97-126,152-158).  `device` = HIP device ordinal. */
int gpis_create(const gpis_params *params, int device, gpis_medium **out);
int gpis_destroy(gpis_medium *m);
int gpis_get_derived(const gpis_medium *m, gpis_derived *out);
const char *gpis_last_error(void);
/* Fills `p` with the reference's defaults (SCNM.cpp:17-34, GPM.cpp:86-95, GPF.hpp:1729,1784). */
void gpis_default_params(gpis_params *p);

/* ---- the hot path (device pointers) --------------------------------------------- */

/* Medium::sampleDistance for n independent segments (GPM.cpp:221-341 → SCNM.cpp:102-183,
 * 93-100).  `coeff` may be NULL. */
int gpis_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays,
                               gpis_seg_out *out, gpis_cond_coeff *coeff, void *stream);

/* Medium::transmittance (GPM.cpp:343-393): visible[i] = 1 if the segment exits, else 0
 * (the reference returns Vec3f(1) / Vec3f(0)). */
int gpis_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays,
                             uint8_t *visible, void *stream);

/* SparseConvolutionNoiseRealization::evaluateValue / evaluateGradient (SCN.cpp:73-99). */
int gpis_eval_value_batch(gpis_medium *m, size_t n, const gpis_query *q,
                          float *value, int32_t *gp_id, void *stream);
int gpis_eval_gradient_batch(gpis_medium *m, size_t n, const gpis_query *q,
                             float *grad3, void *stream);

/* SparseConvolutionNoiseRealization::conditioning (SCN.cpp:431-595): q[i].p/dir/... is the
 * segment start; target_val / target_grad3 are state.lastVal / state.lastAniso. */
int gpis_conditioning_batch(gpis_medium *m, size_t n, const gpis_query *q,
                            const float *target_val, const float *target_grad3,
                            gpis_cond_coeff *coeff_out, void *stream);

/* SparseConvolutionNoiseRealization::neePDF / neeGrad (SCN.cpp:652-743). */
int gpis_nee_pdf_batch(gpis_medium *m, size_t n, const gpis_nee_query *q, float *pdf, void *stream);
int gpis_nee_grad_batch(gpis_medium *m, size_t n, const gpis_nee_query *q, float *grad3, void *stream);

/* MeanFunction::color / emission (GPF.hpp:849-857) at n points (xyz triples in DOUBLE, as the reference evaluates them at
 * ro + rd * t, GPM.cpp:316-317): the factor sampleDistance has already applied to `weight` on a hit, and the value a binding
 * stores in MediumSample.emission.  color3 / emission3: n xyz triples of float; either may be NULL. */
int gpis_mean_color_emission_batch(gpis_medium *m, size_t n, const double *p3, float *color3, float *emission3, void *stream);
int gpis_mean_color_emission_host(gpis_medium *m, size_t n, const double *p3, float *color3, float *emission3);
/* (with a procedural primary mean, colour is evaluated at Vec3d(T^-1 . Vec3f(p)), GPF.hpp:1065-1073; emission at p itself) */

/* GaussianProcess::mean_weight_space (GaussianProcess.cpp:379-393) at n double-precision points, any mean type: the value, the id
 * of the slot the CSG minimum chose (0 = mean, 1 = mean_additional) and dmean_da of that slot.  Any output may be null. */
int gpis_mean_batch(gpis_medium *m, size_t n, const double *p3, double *value, int32_t *id, double *grad3, void *stream);
int gpis_mean_host(gpis_medium *m, size_t n, const double *p3, double *value, int32_t *id, double *grad3);

/* The "transform" of a procedural mean (ProceduralMean::_configTransform, GPF.cpp:252-253): a row-major Mat4f.  which = 0: mean,
 * 1: mean_additional.  The library inverts it as Mat4f::invert does (Mat4f.hpp:75-101; a zero determinant gives the identity) and
 * applies the inverse as transformPoint.  Waits for the device, takes the handle's lock.  GPIS_ERR_INVALID_ARG for a slot that is
 * not procedural. */
int gpis_set_mean_transform(gpis_medium *m, int which, const float transform[16]);

/* Medium::sampleDistance / transmittance of the function-space medium (GaussianProcessMedium.cpp:221-393 over
 * FunctionSpaceGaussianProcessMedium::intersectGP / sampleGradient).  rays[i].u_jitter is not used (every variate comes from
 * states[i].sampler_state); states are read and written in place (device pointers).  The two entries share one device
 * workspace per handle: launches of the SAME handle must be ordered (one stream, or an event between them).  The frame of this
 * medium: gpis_fs_render_scene_s and gpis_fs_render_scene_s_paths, at the end of this header. */
int gpis_fs_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, gpis_seg_out *out, void *stream);
int gpis_fs_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, uint8_t *visible, void *stream);
/* The same two entries for host pointers (synchronous; what the Medium binding of the function-space medium calls with a batch
 * of one, integration/HipFunctionSpaceMedium.cpp): rays, states and results are staged through the handle's device buffers. */
int gpis_fs_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, gpis_seg_out *out);
int gpis_fs_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_fs_state *states, uint8_t *visible);

/* Test surface of the function-space path's dense linear algebra: `count` n x n column-major matrices of doubles (device
 * pointers, 1 <= n <= GPIS_FS_MAX_CTX), one wave each.  op GPIS_FS_OP_EIGH: Eigen::SelfAdjointEigenSolver<MatrixXd> (lower
 * triangle read; eigenvectors -> out, eigenvalues ascending -> evals, which may be NULL); GPIS_FS_OP_NORM_TRANSFORM:
 * MultivariateNormalDistribution's normTransform (Eigen::LLT, else eigenvectors x sqrt(max(eigenvalues, 0)), Gaussian.cpp:
 * 121-167); GPIS_FS_OP_PINV: pseudo_inverse (GaussianProcess.cpp:645-662).  Results are bit-identical to the reference's
 * vendored Eigen under the reference's build flags (tests/golden/ref_fs_primitives.npz). */
typedef enum gpis_fs_linalg_op { GPIS_FS_OP_EIGH = 0, GPIS_FS_OP_NORM_TRANSFORM = 1, GPIS_FS_OP_PINV = 2 } gpis_fs_linalg_op;
int gpis_fs_linalg_batch(gpis_medium *m, int op, int n, size_t count, const double *in, double *out, double *evals, void *stream);

/* Test surface of csrc/gpis_libm.hpp, the device's bit-for-bit restatement of the host libm (glibc 2.35, x86-64 with FMA) for the
 * double-precision functions this path calls: out[i] = fn(x[i]) (fn(x[i], y[i]) for GPIS_LIBM_POW; sin -> out, cos -> out2 for
 * GPIS_LIBM_SINCOS and GPIS_LIBM_SINCOSF; GPIS_LIBM_LOGF and GPIS_LIBM_SINCOSF round x to float first and widen the results).  Device pointers; y and out2 may be NULL where
 * unused.  Needs no medium handle; runs on the current device. */
typedef enum gpis_libm_fn { GPIS_LIBM_EXP = 0, GPIS_LIBM_LOG = 1, GPIS_LIBM_LOGF = 2, GPIS_LIBM_SIN = 3, GPIS_LIBM_COS = 4, GPIS_LIBM_SINCOS = 5,
                            GPIS_LIBM_POW = 6, GPIS_LIBM_SINCOSF = 7 } gpis_libm_fn;
int gpis_libm_batch(int fn, size_t n, const double *x, const double *y, double *out, double *out2, void *stream);

/* Test surface of the library's own radix sort (csrc/gpis_sort.hip: stable LSD sort of (uint32 key, uint32 value) pairs, used by
 * the wavefront march and the multi-bounce driver to regroup rays by lattice cell).  Device pointers; scratch is allocated and
 * freed inside the call. */
int gpis_sort_pairs_u32(size_t n, const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out, void *stream);

/* Bit-exact primitives (MathUtil.hpp:179-224, UniformSampler.hpp:41-75, BitManip.hpp:47-50):
 * out[i] = xxhash32 of `arity` (1..4) words at words[i*arity..]; and the PCG32 stream
 * after set_state(state[i]) — `count` raw nextI() draws each. */
int gpis_xxhash32_batch(gpis_medium *m, size_t n, int arity, const uint32_t *words,
                        uint32_t *out, void *stream);
int gpis_pcg32_stream_batch(gpis_medium *m, size_t n, const uint64_t *state, uint32_t count,
                            uint32_t *out, void *stream);

/* ---- host-pointer entries (synchronous) ------------------------------------------
 * What a `Medium` adapter inside the reference calls (a batch of one per sampleDistance / transmittance), and what a
 * host-side wavefront integrator calls with whole batches.  The two march entries move their records in chunks of
 * 262 144 through two streams (H2D, kernel and D2H of consecutive chunks overlap).  Buffers obtained from
 * gpis_alloc_host (pinned memory) are transferred by DMA directly; any other host memory is staged through pinned
 * buffers of the handle with one extra memcpy each way. */
void *gpis_alloc_host(size_t bytes);      /* pinned host memory; NULL on failure */
void gpis_free_host(void *p);
int gpis_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays,
                              gpis_seg_out *out, gpis_cond_coeff *coeff);
int gpis_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible);
int gpis_eval_value_host(gpis_medium *m, size_t n, const gpis_query *q, float *value, int32_t *gp_id);
int gpis_eval_gradient_host(gpis_medium *m, size_t n, const gpis_query *q, float *grad3);
int gpis_conditioning_host(gpis_medium *m, size_t n, const gpis_query *q, const float *target_val,
                           const float *target_grad3, gpis_cond_coeff *coeff_out);
int gpis_nee_pdf_host(gpis_medium *m, size_t n, const gpis_nee_query *q, float *pdf);
int gpis_nee_grad_host(gpis_medium *m, size_t n, const gpis_nee_query *q, float *grad3);

/* ---- measurement ---------------------------------------------------------------- */

/* Device counters: noise evaluations (evaluateValue/evaluateGradient-equivalents,
 * conditioning evaluations included) and segments, accumulated since the last reset.
 * Synchronises the device. */
int gpis_get_counters(gpis_medium *m, uint64_t *n_eval, uint64_t *n_seg);
int gpis_reset_counters(gpis_medium *m);

/* Per-kernel timing with HIP events recorded on the launch stream around every march-kernel
 * launch (off by default; events cost a few microseconds per launch).  `which`: 0 = the
 * sampleDistance kernel, 1 = the transmittance kernel, 2 = the neePDF / neeGrad launches of
 * gpis_render_scene_s_nee (time and launches only).  Returns the summed kernel time, the
 * number of launches, and that kernel's share of the evaluation / segment counters since the
 * last gpis_reset_counters.  Synchronises the device. */
int gpis_set_profiling(gpis_medium *m, int enable);

/* How the rays of the *_batch / *_host march entries are ordered.  Results never depend on it; with a
 * guide field built it selects the form of the march: GPIS_ORDER_COHERENT (default) — the 64 consecutive
 * records of a wave are neighbours in lattice space (camera rays in pixel order): one resident kernel per
 * batch; GPIS_ORDER_SCATTERED — arbitrary order (bounced rays of a wavefront integrator): the march
 * runs as step / sort / evaluate iterations that regroup the exact evaluations by lattice cell. */
enum { GPIS_ORDER_COHERENT = 0, GPIS_ORDER_SCATTERED = 1 };
int gpis_set_batch_order(gpis_medium *m, int order);

/* Tuning options of a handle (speed only — results never depend on them). */
typedef enum gpis_option {
    GPIS_OPT_MARCH_FORM = 0,     /* form of the guided march: gpis_march_form; AUTO follows gpis_set_batch_order */
    GPIS_OPT_WAVE_TAIL = 1,      /* wavefront march: below this many active rays one wave finishes one ray (default 262144; 0 = never) */
    GPIS_OPT_PATHS_SORT = 2,     /* gpis_render_scene_s_paths: regroup secondary segments by lattice cell (default 1) */
    GPIS_OPT_PATHS_PRESORT = 3,  /* ... also when the wavefront march (which regroups the exact work itself) runs (default 1) */
    GPIS_OPT_CHUNK_LOG2 = 4,     /* log2 of the tile drivers' samples per chunk (8..28; 0 = as large as the device holds) */
    GPIS_OPT_PERSISTENT = 5,     /* per-path media: 1 (default) = persistent refilling march kernels, 0 = one ray per lane per launch */
    GPIS_OPT_SOLO_MAX = 6,       // persistent march: evaluate sideways (lane = impulse) while at most this many lanes of a wave have a
                                 //   pending evaluation; -1 (default) = derived from impulse_density
    GPIS_OPT_RANGE_LEN = 7,      // guided march (resident form): 0 (default) = one ray per lane per launch; > 0 = rays per wave with
                                 //   in-wave refill as segments finish (multiple of 64; measured slower on camera rays)
    GPIS_OPT_DEFER_GRAD = 8,     // guided march (resident form): 0 (default) = the segment's gradient is evaluated at the end of the march kernel;
                                 //   1 = by a second kernel over the pending records (measured: DESIGN.md 8, the spill experiment)
    GPIS_OPT_SCENE_EXIT_STATE = 9,   // gpis_render_scene_s, diagnostic: 0 (default) = the primary march of the resident guided form does not
                                     //   evaluate lastVal and the gradient of a segment that exits (the driver reads neither); 1 = it does
    GPIS_OPT_SCENE_COMPACT = 10,     // gpis_render_scene_s on the resident guided march without exit state: 1 (default) = its kernels pass
                                     //   32-byte ray / hit records (71 B of workspace per sample); 0 = the 128 / 96-byte records of the batch
                                     //   ABI (236 B per sample).  The same evaluations either way; environment: GPIS_SCENE_COMPACT
    GPIS_OPT_SHADOW_LEAN = 11,       // transmittance on the resident guided march: 1 (default) = the march ends at the first step whose sign
                                     //   differs (exact or certified), keeps signs only and skips the start value of a continued segment;
                                     //   0 = it refines the crossing as sampleDistance does.  The same visibility either way, fewer
                                     //   evaluations with 1; environment: GPIS_SHADOW_LEAN
    GPIS_OPT_COUNT_
} gpis_option;
typedef enum gpis_march_form { GPIS_MARCH_FORM_AUTO = 0, GPIS_MARCH_FORM_RESIDENT = 1, GPIS_MARCH_FORM_WAVE = 2 } gpis_march_form;
int gpis_set_option(gpis_medium *m, int option, long long value);
int gpis_get_option(gpis_medium *m, int option, long long *value);
int gpis_get_kernel_profile(gpis_medium *m, int which, double *total_ms, uint64_t *launches,
                            uint64_t *n_eval, uint64_t *n_seg);

/* ---- certified guide field (single-realization media) ------------------------ */

/* Tabulates the medium's lattice noise on a grid of `points_per_cell` (8/16/32/64) samples per cell
 * over |grid coordinate| < half_extent_cells, with a rigorous per-block error bound, and switches
 * sampleDistance / transmittance to the guided march: steps whose sign the table certifies cost one
 * lookup, all others run the exact evaluation, so results are unchanged.  Memory:
 * (2*half*ppc)^3 * 4 bytes (4.3 GB for half=16, ppc=32).  Returns GPIS_ERR_UNSUPPORTED for media
 * the wave-cooperative path does not cover.  gpis_drop_guide frees it. */
int gpis_build_guide(gpis_medium *m, int half_extent_cells, int points_per_cell);
int gpis_drop_guide(gpis_medium *m);
/* Size of the guide field: the samples are stored in bricks of 16^3 grid points and only the bricks in which the certificate can be
 * asked for more than the mean (|mean| within sigma * bound(|N|) / norm somewhere in the brick) are tabulated; everywhere else
 * every step is decided by the mean alone.  bytes_dense = what the full grid would take.  All zero without a guide field. */
typedef struct gpis_guide_info {
    int32_t half_extent_cells, points_per_cell;
    uint64_t bricks_total, bricks_allocated, bricks_usable;
    uint64_t bytes_samples, bytes_bounds, bytes_dense;
    uint64_t selfcheck_points_tabulated;      /* of the last gpis_guide_selfcheck: points that fell into tabulated bricks */
} gpis_guide_info;
int gpis_get_guide_info(gpis_medium *m, gpis_guide_info *out);
/* March steps certified by the guide since the last gpis_reset_counters: each stands for one
 * evaluateValue call of the reference (exact evaluations stay in n_eval). */
int gpis_get_guide_steps(gpis_medium *m, uint64_t *n_guide);
/* Test surface: evaluates the exact lattice sum and the guide at n grid-space points (device
 * pointer, xyz triples; consecutive groups of 64 must lie within one cell of each other) and reports
 * how many violate |exact - guide| <= bound (must be 0), the largest ratio and the mean bound. */
int gpis_guide_selfcheck(gpis_medium *m, size_t n, const float *points3, uint64_t *checked,
                         uint64_t *violations, float *max_ratio, float *mean_bound, void *stream);

/* Test surface for the march's certificate: for each ray (device pointer) the first `steps` march
 * positions of SCNM.cpp:129-132 are classified by the guide, and every certified sign is compared with
 * the sign of the exact evaluateValue at the same position; `violations` must be 0. */
int gpis_guide_raycheck(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint32_t steps,
                        uint64_t *certified, uint64_t *violations, void *stream);

/* ---- tile → ray-batch driver (SURVEY.md §8d "Scene S", §8f-1) -------------------- */

typedef struct gpis_scene_s {
    uint32_t width, height;
    uint32_t spp_begin, spp_count;    /* sample indices [spp_begin, spp_begin+spp_count) */
    uint32_t scene_seed;              /* 0xBA5EBA11 */
    uint32_t tile_size;               /* 16 (PathTraceIntegrator.hpp:27) */
    float cam_pos[3];                 /* (0,0,4) */
    float cam_fov_deg;                /* 35 */
    float bound_radius;               /* 1.5 */
    float light_dir[3];               /* (0.5,0.7,0.5)/|.| (normalised by the driver) */
    float light_radiance;             /* 1 */
    uint32_t y_begin, y_count;        /* image rows this call covers */
    uint32_t shard_index, shard_count; /* shard_count > 1: of those rows, only the tile rows t (tile_size pixels high, counted
                                          from y_begin) with t % shard_count == shard_index — the interleaved tile-row split of
                                          the multi-GPU driver; 0 or 1 = all rows */
} gpis_scene_s;

void gpis_default_scene_s(gpis_scene_s *s, uint32_t width, uint32_t height, uint32_t spp);

/* Copies `voxels` (host pointer, dims[0] * dims[1] * dims[2] floats) to the device and switches the lookup on.  The medium must
 * have been created with grid_nonstationary = 1.  Not to be called while work of this handle is in flight. */
int gpis_set_variance_grid(gpis_medium *m, const gpis_variance_grid *g, const float *voxels);

/* The voxel grid of a tabulated mean (TabulatedMean::_grid, GPF.cpp:143-153), in the descriptor gpis_set_variance_grid takes.
 * which = 0: mean, 1: mean_additional.  Copies `voxels` (host pointer, dims[0] * dims[1] * dims[2] floats) to the device; the copy
 * belongs to the handle, is replaced by a second call for the same slot and freed by gpis_destroy.  It is independent of the
 * variance grid's copy: a medium may carry both.  Waits for the device, takes the handle's lock; not to be called while work of
 * this handle is in flight.  GPIS_ERR_INVALID_ARG for a slot that is not tabulated, for which = 1 without has_mean_additional,
 * for null or non-positive dims and for interpolate outside {0, 1} ("quadratic" is refused, as for the variance grid). */
int gpis_set_mean_grid(gpis_medium *m, int which, const gpis_variance_grid *g, const float *voxels);

/* A neural SDF mean (NeuralMean over GPNeuralNetwork's mean network, GPF.cpp:197-248, GPNeuralNetwork.hpp): an fp64 MLP
 * v = W0 p + b0 (no activation), v = sin(Wk v + bk) per hidden layer, (Wout v + bout)(0), evaluated at
 * q = mult(transform^-1, p) clamped to the bounds when it lies outside them; mean = (nn(q) + offset) * scale.  The library
 * evaluates it with the reference's arithmetic bit for bit (Eigen's three summation orders, the host's sin) and hands it to the
 * march as the voxels of a tabulated mean (gpis_bake_mean_network): the march itself never evaluates the network.
 * dims[k] = (in, out) of layer k: dims[0].in = 3, dims[k].in = dims[k-1].out, the last out = 1, every width <= 256, n_layers in
 * 2 .. 16; anything else is GPIS_ERR_INVALID_ARG with a message.  The weights are one array of doubles in the order of the
 * reference's file: per layer out x in column-major, then out biases. */
#define GPIS_NN_MAX_LAYERS 16
#define GPIS_NN_MAX_WIDTH 256
typedef struct gpis_mean_network {
    int32_t n_layers;
    int32_t _pad;
    int32_t dims[GPIS_NN_MAX_LAYERS][2];
    double bounds_min[3], bounds_max[3];   /* GPNeuralNetwork::_bounds */
    float offset, scale;
    float transform[16];                   /* row-major Mat4f; inverted as gpis_set_mean_transform inverts one */
} gpis_mean_network;

/* NeuralMean::mean (value) and dmean_da (grad3: eps = 0.001 in double, mean at +x, +y, +z and a, each difference / eps) at n
 * double-precision points.  Either output may be null.  No medium handle: the _host form takes host pointers and runs on the
 * current device; the _batch form takes device pointers for the weights, the points and the outputs and allocates its
 * activation workspace (networks wider than 64 only) for the call.  `weights` holds the sum over the layers of out * (in + 1)
 * doubles. */
int gpis_network_mean_host(const gpis_mean_network *net, const double *weights, size_t n, const double *p3, double *value, double *grad3);
int gpis_network_mean_batch(const gpis_mean_network *net, const double *weights, size_t n, const double *p3, double *value, double *grad3,
                            void *stream);

/* Evaluates the network on the lattice of `g` and installs the result as the voxel grid of the tabulated mean in slot `which`,
 * exactly as gpis_set_mean_grid installs one (same lock, same model refresh, an earlier grid of the slot replaced).  Voxel
 * (i, j, k) gets float(mean(x)) with x_r = double(A[4r]) (origin_i + i) + double(A[4r+1]) (origin_j + j) +
 * double(A[4r+2]) (origin_k + k) + double(A[4r+3]), A = index_to_world (rows 0..2 of a row-major Mat4f), summed left to right,
 * unfused.  `weights` is a host pointer.  The voxels stay on the device unless voxels_out (host pointer, dims[0] * dims[1] *
 * dims[2] floats) is given.  GPIS_ERR_INVALID_ARG as gpis_set_mean_grid and for an invalid network. */
int gpis_bake_mean_network(gpis_medium *m, int which, const gpis_mean_network *net, const double *weights, const gpis_variance_grid *g,
                           const float index_to_world[12], float *voxels_out);

/* Allocates the workspace gpis_render_scene_s needs for `s` ahead of the first frame: 71 B per sample of the largest chunk the
 * device holds with the compact records (the resident march, GPIS_OPT_SCENE_COMPACT: 9.5 GB for a whole 1920x1080x64 frame),
 * 236 B per sample (31.3 GB) otherwise.  The call is meant to run beside gpis_build_guide, so it does not look at whether a guide
 * is present yet: a medium that can carry a guide gets the guided body's size, and a handle that then renders without a guide
 * grows the arrays on demand.  Optional: the render entry allocates on demand, each of its three arrays
 * right before the first kernel that needs it.  This entry does not take the handle's lock: call it from a second host thread
 * while gpis_build_guide runs (allocation time is per byte and overlaps the guide build's kernels) — not concurrently with a
 * render call that uses a DIFFERENT scene size on the same handle. */
int gpis_reserve_scene_workspace(gpis_medium *m, const gpis_scene_s *s);

/* Renders rows [y_begin, y_begin+y_count) × all columns × spp_count samples of scene S and
 * ACCUMULATES sum-of-radiance into radiance_sum[height*width] (float, device pointer,
 * indexed y*width+x; caller divides by total spp).  Runs primary sampleDistance, shading,
 * one shadow transmittance per hit.  hit_count (device, may be NULL) accumulates per-pixel hits.
 * The driver's internal segment records of primary rays that EXIT carry no state (last_val = 0, aniso = 0: lastVal and the
 * gradient at farT are not evaluated, GPIS_OPT_SCENE_EXIT_STATE), since the estimator reads only ok / exited of them; the records
 * gpis_sample_distance_batch returns are complete as ever.  Image and hit counts do not depend on the option.
 * Where that lean primary march runs (a guide field, the resident form, no range refill, no deferred gradient), the driver's kernels
 * pass 32-byte ray and hit records instead of gpis_ray_in / gpis_seg_out (GPIS_OPT_SCENE_COMPACT): the camera position, the light
 * direction and the first_scatter / bounce values of a launch are kernel arguments, the fields only per-path media read are dropped.
 * The marches evaluate exactly what they evaluate on the full records. */
int gpis_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum,
                        uint32_t *hit_count, void *stream);

/* Specular micro-surface + light of finite solid angle for gpis_render_scene_s_nee. 32 bytes. */
typedef struct gpis_surface_s {
    float eta, k;             /* ConductorBsdf "eta", "k" (one channel; Fresnel.hpp:102-123) */
    float albedo;
    float cap_cos;            /* the light: an infinite spherical cap about scene.light_dir, cos of its half-angle
                                 (InfiniteSphereCap "cap_angle") */
    float cap_radiance;
    float _pad[3];
} gpis_surface_s;

/* Scene S with the reference's specular NEE coupling: per sample the primary
 * sampleDistance, then TraceBase::volumeEstimateDirect = volumeLightSample + volumePhaseSample
 * (TraceBase.cpp:346-420) for a BRDFPhaseFunction over a ConductorBsdf (BRDFPhaseFunction.cpp:27-96,
 * ConductorBsdf.cpp:59-139) and one InfiniteSphereCap light:
 *   light sample (schemes NEE, MIS): f = albedo * F(wi.z) * neePDF(half-vector normal); the shadow segment
 *     runs on a state copy whose lastAniso = neeGrad(half-vector normal); weight power-heuristic unless NEE;
 *   phase sample (schemes UNI, MIS): mirror direction about the sampled normal, pdf = neePDF(normal), counts
 *     when it falls inside the cap.
 * The scheme is the one sampleDistance reports per sample (gpis_seg_out.scheme).  The cap direction is drawn
 * with a rejection-sampled azimuth (sqrt only) instead of SampleWarp::uniformSphericalCap's sin/cos. */
int gpis_render_scene_s_nee(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_s *surf,
                            float *radiance_sum, void *stream);

/* Multi-bounce paths with the estimator of gpis_render_scene_s_nee at every hit: PathTracer::traceSample
 * (PathTracer.cpp:62-169) over TraceBase::handleVolume (TraceBase.cpp:539-563) for the conductor micro-surface and the cap
 * light.  Accepts and refuses what gpis_render_scene_s_nee does (handles, surf, rows, tile-row shards, spp ranges) and refuses
 * max_path_bounces < 1.  Per sample (x, y, k): one PCG32 stream, set_state(xxhash32(x, y, k, scene_seed) + 1); the draws jx, jy
 * and the first march jitter; the camera ray clipped to the bounding sphere (a miss adds nothing and marches nothing);
 * thr = 1, E = 0.  Then for b = 0; b + 1 < max_path_bounces; ++b:
 *   1. sampleDistance of the current ray with segment word b (its gpis_cond_coeff is kept).  !ok ends the path;
 *      thr = thr * weight[0]; `exited` ends the path (the light seen directly is never added).
 *   2. L = volumeLightSample + volumePhaseSample exactly as gpis_render_scene_s_nee computes them for this segment; the shadow
 *      segments run on the state copy with segment b+1, bounce+1, first_scatter = 0 (lastAniso = neeGrad(half vector) for the
 *      light sample, the sampled aniso for the phase sample).  Draws in the serial order: z and the disk pairs (schemes NEE,
 *      MIS), then ONE jitter per shadow segment that is marched, the light's first.  E = E + thr * L.
 *   3. The bounce (ConductorBsdf::sample, ConductorBsdf.cpp:59-76): thr = thr * F with the F = albedo * conductorReflectance(eta,
 *      k, wi.z) that went into L; thr == 0 ends the path (PathTracer.cpp:143); w = normalized(toGlobal(-wi.x, -wi.y, wi.z)) for
 *      every scheme; no chord of (p, w) through the bounding sphere ends the path.  The reference evaluates neePDF for the
 *      sampled direction and does not use the value; no such evaluation is made (or counted) here.
 *   4. Only if b + 2 < max_path_bounces, the next ray: pos = p, dir = w, near = 0, far = the chord's end, segment b+1,
 *      first_scatter = 0, bounce+1, last_val / last_gp_id / last_aniso from the segment's result, info_t + sample_t, and
 *      u_jitter = the stream's next draw.  Otherwise nothing follows and nothing is drawn.
 * There is NO Russian roulette (PathTracer.cpp:145-151 is left out, as in the Lambert path drivers: nextBoolean would add a
 * draw per bounce).  The segment of bounce max_path_bounces - 1 is not marched, since it cannot contribute (TraceBase.cpp:546):
 * max_path_bounces = 1 adds zeros, and with max_path_bounces = 2 on a medium whose weight[0] is exactly 1 the image equals
 * gpis_render_scene_s_nee's bit for bit.  All float arithmetic runs with contraction off.
 * Each pixel's sum of E, taken in sample order from zero, is ACCUMULATED into radiance_sum[height*width] once per chunk of
 * samples, and per pixel the segments marched (path, light shadow and phase shadow segments) into seg_count[height*width]
 * (device pointers; seg_count may be NULL).  Image and counts depend neither on how a frame is cut into calls (rows, shards,
 * spp ranges) or chunks (GPIS_OPT_CHUNK_LOG2) nor on any tuning option.  Asynchronous on `stream`. */
int gpis_render_scene_s_nee_paths(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_s *surf, int max_path_bounces,
                                  float *radiance_sum, uint32_t *seg_count, void *stream);

/* Multi-bounce wavefront driver on scene S: per sample, up to `max_path_bounces`
 * medium interactions following PathTracer::traceSample / TraceBase::handleVolume
 * (PathTracer.cpp:62-75, TraceBase.cpp:539-563):
 *   sampleDistance (segment word = bounce, PathTracer.cpp:64) → on a hit: next-event estimation of
 *   the directional light through a state copy with segment+1 (TraceBase.cpp:546-549, 346-386:
 *   BRDFPhaseFunction/Lambert eval = albedo/pi * cos, Dirac light → no MIS) with one shadow
 *   transmittance, then a cosine-weighted bounce about the sampled normal (throughput *= albedo).
 * The bounce direction is drawn by rejection from the unit disk (sqrt only) instead of
 * SampleWarp::cosineHemisphere's sin/cos so that CPU and GPU agree bit for bit.
 * Accumulates sum-of-radiance into radiance_sum[height*width] (device pointer). */
int gpis_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo,
                              float *radiance_sum, void *stream);

/* gpis_render_scene_s_paths carried in RGB, with the medium's emission (MediumSample.emission, GPM.cpp:317): the image the
 * per-channel quantities of the medium give — gpis_seg_out.weight[3] (mean colour, sigma_s / sigma_t per channel) and the mean's
 * "emission" — under PathTracer::traceSample (PathTracer.cpp:72-73: emission += throughput * sample.emission; throughput *=
 * sample.weight).  Accepts the handles, rows, tile-row shards, spp ranges, chunking and stream of gpis_render_scene_s_paths;
 * GPIS_ERR_INVALID_ARG (nothing is written) for max_path_bounces < 1, a NULL albedo (host pointer, 3 floats) or radiance_sum3, a
 * row range outside the image, a bad shard, a weight-space handle.
 * Per sample, operation for operation in float with contraction off: the draws jx, jy, u_march and the camera ray of
 * gpis_render_scene_s_paths; thr[c] = 1, em[c] = 0.  Let E = "mean_emission is enabled" and B = max_path_bounces.  For b = 0, 1, ...:
 *   1. sampleDistance with segment word b.  The last segment marched is b = B-2 when !E (the loop of gpis_render_scene_s_paths)
 *      and b = B-1 when E: that segment can only add its hit's emission; no NEE and no bounce follow it.
 *   2. !ok ends the path and adds nothing.
 *   3. On a hit (ok && !exited) when E: e = emission(ro + rd * t), ro the ray position widened to double, rd the direction
 *      normalised in double, t = gpis_seg_out.t — the point and the evaluation of gpis_mean_color_emission_*; e rounded to float;
 *      em[c] = em[c] + (thr[c] * e[c]) with thr BEFORE the weight and the product rounded to float on its own.
 *   4. thr[c] = thr[c] * weight[c]; `exited` ends the path.
 *   5. For b < B-1: next-event estimation and the cosine bounce exactly as gpis_render_scene_s_paths (same conditions, draws and
 *      order of draws) with f[c] = albedo[c] * (1.0f/3.1415926536f) * wo.z and contrib[c] = thr[c] * (f[c] * light_radiance); after
 *      the shadow transmittance em[c] = em[c] + (visible ? contrib[c] : 0); then thr[c] *= albedo[c].  Within a bounce the emission
 *      term is added before the NEE term.
 * Each pixel's sum of em[c], taken per channel in sample order from zero, is ACCUMULATED into radiance_sum3[3*(y*width+x)+c]
 * (device pointer, 3*height*width floats) once per chunk of samples, and per pixel the segments marched (path plus shadow
 * segments) into seg_count[height*width] (device pointer; may be NULL).  Image and counts depend neither on how a frame is cut
 * into calls or chunks nor on GPIS_OPT_PATHS_SORT / PATHS_PRESORT / MARCH_FORM / PERSISTENT / CHUNK_LOG2.
 * Consequences: with !E and albedo[0] == albedo, channel 0 is gpis_render_scene_s_paths bit for bit, for every medium; with E,
 * max_path_bounces = 1 renders first-hit emission (with !E it adds zeros and marches nothing).  NaN components a field returns
 * propagate as float arithmetic gives them.  Asynchronous on `stream`. */
int gpis_render_scene_s_paths_rgb(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, const float albedo[3],
                                  float *radiance_sum3, uint32_t *seg_count, void *stream);

/* ---- variance-driven adaptive sampling (PathTraceIntegrator.cpp:43-163, SampleRecord.hpp:44-65; RendererSettings.hpp:39-51:
 * "adaptive_sampling" true and "spp_step" 16 are the reference's defaults) ---------------------------------------------------- */
typedef struct gpis_adaptive_s {
    uint32_t spp_step;        /* 16  RendererSettings "spp_step" */
    uint32_t threshold;       /* 16  PathTraceIntegrator::AdaptiveThreshold; >= 2 */
    uint32_t seed;            /* 0xBA5EBA11: seed of the integrator's own UniformSampler */
    uint32_t _pad;
} gpis_adaptive_s;

/* SampleRecord.hpp:13-15, one per 4x4 variance tile, index vx + vy * ceil(width/4). 24 bytes. */
typedef struct gpis_adaptive_record {
    uint32_t sample_count, next_sample_count, sample_index;
    float adaptive_weight, mean, running_variance;
} gpis_adaptive_record;

typedef struct gpis_adaptive_info { uint32_t passes_rendered, stopped_early; uint64_t samples; } gpis_adaptive_info;

void gpis_default_adaptive_s(gpis_adaptive_s *a);

/* gpis_render_scene_s — the same Lambert estimator, sample for sample — under the sample schedule of the reference's
 * PathTraceIntegrator.  Sparse-convolution handles; s->spp_count is the AVERAGE number of samples per pixel, S.
 *
 * Pass loop (PathTraceIntegrator::startRender / advanceSpp): cur = 0; while cur < S: next = min(cur + spp_step, S), n = next - cur;
 * one plan step (gpis_adaptive_plan_host below, = generateWork, :109-133); a 0 from it ends the frame; else the pass is rendered
 * and cur = next.  The records start zeroed (SampleRecord.hpp:17-22).  The integrator's sampler is UniformSampler(hash32(seed))
 * (:194, UniformSampler.hpp:22, MathUtil.hpp:169) less the ceil(W/16) * ceil(H/16) nextI() draws of diceTiles (:26-41):
 * gpis_adaptive_rng_init_host.  Nothing else draws from it.
 *
 * Samples of a pass (renderTile, :135-163): pixel (x, y) belongs to record (x/4) + (y/4) * ceil(W/4) and takes the samples
 * k = s->spp_begin + sample_index + i, i < next_sample_count of that record; each is exactly the sample (x, y, k) of
 * gpis_render_scene_s.  DIFFERENCE from the reference: it hands traceSample `_currentSpp + i` as the spp word (:148), which
 * repeats realization seeds across passes once a count exceeds spp_step; every draw of this library derives from k, so that
 * would be the same sample twice.  sample_index + i is the reference's own startPath index (:147).
 * Clamp (:149-156): a sample value that is NaN, infinite or > 65536 counts as 0, in the image and in the statistics.
 * Image: per pixel and pass the samples are summed in i order from zero; that sum is ACCUMULATED once into
 * radiance_sum[y*width+x], the count into sample_count, the hits into hit_count (device pointers, height*width entries; the caller
 * divides each pixel by its own sample_count).  While no sample is clamped, a pixel therefore equals bit for bit what the
 * sequence of gpis_render_scene_s calls with its (spp_begin, spp_count) ranges gives.
 * Statistics: per record SampleRecord::addSample(float) (Welford in float, :44-50, contraction off) over the tile's pixels
 * row-major, clipped at the image edge, then i — the order of renderTile, since its 16-pixel tiles are multiples of 4.
 * records (device pointer, ceil(W/4) * ceil(H/4) entries, may be NULL) receives the records after the last rendered pass with the
 * closing sample_index += next_sample_count applied: sample_index is then the tile's samples per pixel.  info (host pointer, may be
 * NULL): passes rendered, whether a plan step ended the frame early, samples rendered.  hit_count may be NULL.
 * Image, counts and records depend neither on how a pass is cut into chunks (GPIS_OPT_CHUNK_LOG2; cuts fall between records,
 * and a record larger than a chunk is a chunk of its own) nor on any tuning option; the marches are those gpis_render_scene_s
 * launches (32-byte records where it would pass them).
 * GPIS_ERR_INVALID_ARG, nothing written: rows other than the whole image or shard_count > 1 (the percentile needs the whole
 * frame), spp_step == 0, threshold < 2, a NULL a / radiance_sum / sample_count, a weight-space handle, spp_count == 0.
 * The plan runs on the host: the entry SYNCHRONISES `stream` once per pass (and returns with the stream idle). */
int gpis_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                 float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count,
                                 gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);
/* host only, no device needed: one PathTraceIntegrator::generateWork step on `records` (in place, n_records must be
 * ceil(width/4) * ceil(height/4)); returns 1 (render the pass), 0 (maxError == 0: stop; only sample_index and adaptive_weight
 * have changed), < 0 error.  *rng_state is the integrator sampler's PCG state.  current_spp / pass_spp are _currentSpp and
 * _nextSpp - _currentSpp (pass_spp >= 1).  In order: sample_index += next_sample_count; below the threshold next_sample_count =
 * pass_spp; else errorPercentile95 (:43-58), the clamp to it, dilateAdaptiveWeights (:60-84), distributeAdaptiveSamples
 * (:86-107: double totalWeight in record order, int adaptiveBudget = (pass_spp-1)*W*H in 32 bits, /16, the float factor, the
 * running pixelPdf carry with one next1D() per record), next_sample_count = adaptiveSamples + 1.  min / max are MathUtil.hpp's
 * (a < b ? a : b, a > b ? a : b); int(fractionalSamples) of a NaN is taken as 0 and saturates at +-2^31. */
int gpis_adaptive_plan_host(const gpis_adaptive_s *a, uint32_t width, uint32_t height, uint32_t current_spp,
                            uint32_t pass_spp, uint64_t *rng_state, size_t n_records, gpis_adaptive_record *records);
/* host only: the PCG state gpis_render_scene_s_adaptive starts a width x height frame with (0 for a NULL a). */
uint64_t gpis_adaptive_rng_init_host(const gpis_adaptive_s *a, uint32_t width, uint32_t height);
/* host only, test surface: SampleRecord::addSample over values[n] onto *rec, then variance() and errorEstimate() of the result
 * (out2, may be NULL) — the statistics the device kernel and the plan step compute. */
void gpis_adaptive_record_add_host(gpis_adaptive_record *rec, size_t n, const float *values, float *out2);

/* gpis_render_scene_s_paths_rgb — the same RGB path estimator, sample for sample — under the sample schedule of
 * gpis_render_scene_s_adaptive: what the reference's PathTraceIntegrator runs by default (traceSample into a Vec3f, spent by
 * generateWork).  Sparse-convolution handles; s->spp_count is the AVERAGE number of samples per pixel, S.
 * Pass loop, records, RNG: exactly those of gpis_render_scene_s_adaptive above — the plan step gpis_adaptive_plan_host, the start
 * state gpis_adaptive_rng_init_host, record (x/4) + (y/4) * ceil(W/4); sample i of a record in a pass is
 * k = s->spp_begin + sample_index + i, with the DIFFERENCE from the reference's `_currentSpp + i` stated there.
 * A sample: (x, y, k) gives the em[3] and the segments gpis_render_scene_s_paths_rgb computes for the sample (x, y, k) — its
 * arithmetic, draws and segment words, see that entry; with mean_emission enabled the extra last segment is marched too.
 * Clamp (PathTraceIntegrator.cpp:149-156 on a Vec3f): if ANY component of em is NaN, +-infinite or > 65536, all three components
 * count as 0, in the image and in the statistics.  A large negative finite component is kept (the reference keeps it).  The
 * sample's segments still count in seg_count: they were marched.
 * Statistics: SampleRecord::addSample(float) on the luminance of the clamped value (SampleRecord.hpp:52-55, Vec.hpp:218-222),
 * ((c0 * 0.2126f) + (c1 * 0.7152f)) + (c2 * 0.0722f), every product and sum rounded to float (contraction off), in the order of
 * gpis_render_scene_s_adaptive: the tile's pixels row-major, clipped at the image edge, then i.
 * Image: per pixel, pass and channel the clamped samples are summed in i order from zero; that sum is ACCUMULATED once into
 * radiance_sum3[3*(y*width+x)+c] (device pointer, 3*height*width floats), the count into sample_count[y*width+x], the segments
 * marched (path plus shadow) into seg_count[y*width+x] (device pointers, height*width entries; seg_count may be NULL).
 * records (device pointer, may be NULL) and info (host pointer, may be NULL) are filled as by gpis_render_scene_s_adaptive,
 * including the closing sample_index += next_sample_count.
 * Image, counts, records and info depend neither on how a pass is cut into chunks (GPIS_OPT_CHUNK_LOG2, default 2^25 samples as
 * gpis_render_scene_s_paths_rgb; cuts fall between records, and a record larger than a chunk is a chunk of its own) nor on
 * GPIS_OPT_PATHS_SORT / PATHS_PRESORT / MARCH_FORM / PERSISTENT.
 * GPIS_ERR_INVALID_ARG, nothing written: max_path_bounces < 1, a NULL albedo (host pointer, 3 floats) / radiance_sum3 / a /
 * sample_count, a weight-space handle, rows other than the whole image, shard_count > 1, spp_step == 0, threshold < 2,
 * spp_count == 0.  GPIS_ERR_UNSUPPORTED: a plan that gives a record 0 or more than 2^28 samples in a pass.  GPIS_ERR_DEVICE: the
 * device cannot hold the workspace of the smallest chunk.
 * Consequences: with threshold >= S the schedule is uniform, and while nothing is clamped the image equals bit for bit the
 * sequence of gpis_render_scene_s_paths_rgb calls with the passes' (spp_begin, spp_count) ranges accumulated into one buffer;
 * without emission and with max_path_bounces = 1 every sample is zero: the first pass is rendered, then the plan step ends the
 * frame (stopped_early = 1, passes_rendered = 1).
 * The entry SYNCHRONISES `stream` once per pass and returns with the stream idle. */
extern int gpis_render_scene_s_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                  int max_path_bounces, const float albedo[3],
                                                  float *radiance_sum3, uint32_t *sample_count, uint32_t *seg_count,
                                                  gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);
/* host only, test surface: the Vec3f clamp and the luminance of gpis_render_scene_s_paths_rgb_adaptive on rgb_in[3*n] — the
 * clamped values into rgb_out[3*n] and their luminances into luminance[n] (each may be NULL), by the functions the kernels call. */
extern void gpis_adaptive_rgb_value_host(size_t n, const float *rgb_in, float *rgb_out, float *luminance);

/* gpis_render_scene_s_paths and gpis_render_scene_s_nee_paths — the mono Lambert path estimator and the conductor NEE / MIS path
 * estimator, sample for sample — under the sample schedule of gpis_render_scene_s_adaptive (PathTraceIntegrator.cpp:43-163,
 * SampleRecord.hpp:44-65).  Sparse-convolution handles; s->spp_count is the AVERAGE number of samples per pixel, S; whole frames
 * on one GPU.
 * Pass loop, records, RNG: exactly those of gpis_render_scene_s_adaptive — the plan step gpis_adaptive_plan_host, the start state
 * gpis_adaptive_rng_init_host, records zeroed at the start, record (x/4) + (y/4) * ceil(W/4); sample i of a record in a pass is
 * k = s->spp_begin + sample_index + i, with the DIFFERENCE from the reference's `_currentSpp + i` stated there.
 * A sample: (x, y, k) is the sample (x, y, k) of the uniform entry — its seed, draws, segment words, marches and arithmetic, see
 * gpis_render_scene_s_paths / gpis_render_scene_s_nee_paths; its value is the scalar E that entry adds for it.
 * Clamp (PathTraceIntegrator.cpp:149-156): an E that is NaN, +-infinite or > 65536 counts as 0, in the image and in the
 * statistics.  The sample's segments still count in seg_count: they were marched.
 * Statistics: SampleRecord::addSample(float) on the clamped E, in the order of gpis_render_scene_s_adaptive: the tile's pixels
 * row-major, clipped at the image edge, then i.
 * Image: per pixel and pass the clamped E are summed in i order from zero; that sum is ACCUMULATED once into
 * radiance_sum[y*width+x], the count into sample_count[y*width+x] and, for the NEE entry, the segments marched (path, light shadow
 * and phase shadow segments) into seg_count[y*width+x] (device pointers, height*width entries; seg_count may be NULL).
 * records (device pointer, may be NULL) and info (host pointer, may be NULL) are filled as by gpis_render_scene_s_adaptive,
 * including the closing sample_index += next_sample_count.
 * Image, counts, records and info depend neither on how a pass is cut into chunks (GPIS_OPT_CHUNK_LOG2, default the uniform
 * entry's: 2^25 samples for the Lambert driver, 2^27 for the NEE driver; cuts fall between records, and a record larger than a
 * chunk is a chunk of its own) nor on any tuning option: GPIS_OPT_PATHS_SORT / PATHS_PRESORT / MARCH_FORM / PERSISTENT for the
 * Lambert entry, MARCH_FORM / PERSISTENT for the NEE entry.
 * GPIS_ERR_INVALID_ARG, nothing written: everything the uniform entry refuses (max_path_bounces < 1, a weight-space handle, for
 * the NEE entry a NULL surf or cap_cos outside (-1, 1)), a NULL a / radiance_sum / sample_count, rows other than the whole image,
 * shard_count > 1, spp_step == 0, threshold < 2, spp_count == 0.  GPIS_ERR_UNSUPPORTED: a plan that gives a record 0 or more than
 * 2^28 samples in a pass.  GPIS_ERR_DEVICE: the device cannot hold the workspace of the smallest chunk.
 * Consequences: with threshold >= S the schedule is uniform, and while nothing is clamped the image equals bit for bit the
 * uniform entry called once per pass with that pass's (spp_begin, spp_count), accumulated into one buffer; at
 * max_path_bounces = 2 on a medium whose weight[0] is exactly 1 the NEE entry under that condition equals
 * gpis_render_scene_s_nee called the same way; max_path_bounces = 1 makes every sample zero: the first pass is rendered, then
 * the plan step ends the frame (passes_rendered = 1, stopped_early = 1, seg_count all zero).
 * Each entry SYNCHRONISES `stream` once per pass and returns with the stream idle. */
extern int gpis_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                              int max_path_bounces, float albedo,
                                              float *radiance_sum, uint32_t *sample_count,
                                              gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);
extern int gpis_render_scene_s_nee_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                  const gpis_surface_s *surf, int max_path_bounces,
                                                  float *radiance_sum, uint32_t *sample_count, uint32_t *seg_count,
                                                  gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);

/* gpis_surface_s per channel: the coloured conductor (ConductorBsdf.cpp:24-28, Fresnel.hpp:136-143: one reflectance per channel)
 * under a coloured cap light.  64 bytes. */
typedef struct gpis_surface_rgb_s {
    float eta[3], k[3];        /* ConductorBsdf "eta", "k" */
    float albedo[3];
    float cap_radiance[3];     /* InfiniteSphereCap emission */
    float cap_cos;             /* as gpis_surface_s.cap_cos */
    float _pad[3];
} gpis_surface_rgb_s;
/* the reference's default conductor, copper: eta = (0.200438, 0.924033, 1.10221), k = (3.91295, 2.45285, 2.14219); albedo 1,
 * cap_radiance 1, cap_cos 0.9781476 (a 12-degree cap).  Materials by name (ComplexIorList) are the loader's to resolve. */
void gpis_default_surface_rgb(gpis_surface_rgb_s *surf);

/* gpis_render_scene_s_nee_paths carried in RGB, with the medium's emission: the conductor NEE / MIS path estimator as the
 * reference's integrator runs it for a ConductorBsdf, whose Fresnel term, albedo and light are Vec3f, on a medium whose weight and
 * emission are Vec3f.  Accepts and refuses what gpis_render_scene_s_nee_paths does (handles, rows, tile-row shards, spp ranges,
 * chunking, stream; GPIS_ERR_INVALID_ARG, nothing written, for max_path_bounces < 1, a NULL surf or radiance_sum3, cap_cos outside
 * (-1, 1), a row range outside the image, a bad shard, a weight-space handle).
 * Per sample, operation for operation in float with contraction off.  The stream, the draws and their order, the rays, the
 * masks, the queries and the segments are those of gpis_render_scene_s_nee_paths step for step: no direction, pdf, heuristic or
 * draw depends on colour.  thr[c] = 1, em[c] = 0.  Let E = "mean_emission is enabled" and B = max_path_bounces.  For b = 0, 1, ...:
 *   1. sampleDistance with segment word b.  The last segment marched is b = B-2 when !E and b = B-1 when E: that segment can only
 *      add its hit's emission; no estimator and no bounce follow it.  !ok ends the path and adds nothing.
 *   2. Emission and weight: steps 3 and 4 of gpis_render_scene_s_paths_rgb verbatim — on a hit when E, e = emission(ro + rd * t)
 *      as gpis_mean_color_emission_* evaluates it, em[c] = em[c] + (thr[c] * e[c]) with thr BEFORE the weight; then
 *      thr[c] = thr[c] * weight[c]; `exited` ends the path.  Within a bounce the emission term is added before the NEE terms.
 *   3. F[c] = albedo[c] * conductorReflectance(eta[c], k[c], wi.z): the scalar function of gpis_render_scene_s_nee per channel,
 *      its eta == 0 && k == 0 -> 1 case included.
 *   4. Light sample (schemes NEE, MIS): f[c] = F[c] * neePDF(half vector).  The shadow segment is marched iff f is not zero in
 *      every channel (Vec3f == 0.0f, Vec.hpp:452-458) and the chord exists.  lightF[c] = f[c] * cap_radiance[c] / pdf_l, times the
 *      scalar power heuristic unless the scheme is NEE.
 *   5. Phase sample (schemes UNI, MIS): phaseF[c] = cap_radiance[c] * F[c], times the scalar heuristic unless the scheme is UNI.
 *   6. L[c] = the visible ones of lightF[c] and phaseF[c], the light's first; L = 0 for both iff cap_radiance is zero in every
 *      channel (TraceBase.cpp:374, 410 on a Vec3f).  em[c] = em[c] + thr[c] * L[c] with the thr of step 2.
 *   7. The bounce: thr[c] = thr[c] * F[c]; the path ends when max(thr[0..2]) == 0 (PathTracer.cpp:143; Vec::max: m = thr[0], then
 *      each larger component); the rest is steps 3 and 4 of gpis_render_scene_s_nee_paths, the next ray (and its jitter) following
 *      only if its segment b+1 is one of those step 1 marches.
 * There is NO Russian roulette, as in gpis_render_scene_s_nee_paths.
 * Each pixel's sum of em[c], taken per channel in sample order from zero, is ACCUMULATED into radiance_sum3[3*(y*width+x)+c]
 * (device pointer, 3*height*width floats) once per chunk of samples, and per pixel the segments marched (path, light shadow and
 * phase shadow segments) into seg_count[height*width] (device pointer; may be NULL).  Image and counts depend neither on how a
 * frame is cut into calls (rows, shards, spp ranges) or chunks (GPIS_OPT_CHUNK_LOG2) nor on any tuning option.
 * Consequences: with eta[c] = eta, k[c] = k, albedo[c] = albedo, cap_radiance[c] = cap_radiance on a medium without emission
 * whose three weight channels are equal, every channel and seg_count equal gpis_render_scene_s_nee_paths bit for bit; on any
 * medium without emission, channel c equals that entry given channel c's surface wherever weight[c] == weight[0], as long as
 * the channels agree on which f and which throughputs are zero (a light segment or a path that one channel alone keeps alive is
 * marched here and not by that channel's mono frame, which moves seg_count and the later draws); with E, max_path_bounces = 1
 * renders first-hit emission (with !E it adds zeros and marches nothing).  Asynchronous on `stream`. */
int gpis_render_scene_s_nee_paths_rgb(gpis_medium *m, const gpis_scene_s *s, const gpis_surface_rgb_s *surf, int max_path_bounces,
                                      float *radiance_sum3, uint32_t *seg_count, void *stream);

/* gpis_render_scene_s_nee_paths_rgb — the same estimator, sample for sample — under the sample schedule of
 * gpis_render_scene_s_adaptive.  Pass loop, records, RNG, sample numbering (k = s->spp_begin + sample_index + i), chunking and
 * the synchronisation once per pass are those of gpis_render_scene_s_nee_paths_adaptive; the Vec3f clamp (any NaN, +-infinite or
 * > 65536 component zeroes the sample; its segments still count), the statistics on the luminance of the clamped value and the
 * image / sample_count / seg_count layout are those of gpis_render_scene_s_paths_rgb_adaptive.
 * GPIS_ERR_INVALID_ARG, nothing written: everything gpis_render_scene_s_nee_paths_rgb refuses, a NULL a / sample_count, rows other
 * than the whole image, shard_count > 1, spp_step == 0, threshold < 2, spp_count == 0.  GPIS_ERR_UNSUPPORTED and GPIS_ERR_DEVICE as
 * gpis_render_scene_s_nee_paths_adaptive.
 * Consequence: with threshold >= S and nothing clamped the image equals bit for bit gpis_render_scene_s_nee_paths_rgb called once
 * per pass with that pass's (spp_begin, spp_count), accumulated into one buffer. */
extern int gpis_render_scene_s_nee_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                      const gpis_surface_rgb_s *surf, int max_path_bounces,
                                                      float *radiance_sum3, uint32_t *sample_count, uint32_t *seg_count,
                                                      gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);

/* Materials chosen by GP id: the medium's phase-function table (GPM.cpp:119-125: "phase_function", then
 * "additional_phase_functions"; GaussianProcessMedium::sampleDistance ends with sample.phase = _phaseFunctions[state.lastGPId],
 * GPM.cpp:335), each entry a BRDFPhaseFunction over a ConductorBsdf or a LambertBsdf, under ONE light, gpis_surface_rgb_s's cap.
 * The id of a hit is gpis_seg_out.gp_id: the slot the CSG minimum chose (has_mean_additional) or the surface / volume side of
 * surf_vol_phase_separate (SCN.cpp:80-86). */
#define GPIS_MAX_MATERIALS 4
typedef enum gpis_material_type { GPIS_MATERIAL_CONDUCTOR = 0, GPIS_MATERIAL_LAMBERT = 1 } gpis_material_type;
typedef struct gpis_material_rgb {   /* 48 bytes */
    int32_t type;                    /* gpis_material_type */
    float eta[3], k[3];              /* conductor only */
    float albedo[3];
    int32_t _pad[2];
} gpis_material_rgb;
typedef struct gpis_materials_s {    /* 224 bytes */
    uint32_t n_materials;            /* 1 .. GPIS_MAX_MATERIALS: material[0] = the medium's phase function, 1.. = additional_phase_functions */
    float cap_cos;                   /* the light: gpis_surface_rgb_s's cap */
    float cap_radiance[3];
    uint32_t _pad[3];
    gpis_material_rgb material[GPIS_MAX_MATERIALS];
} gpis_materials_s;
/* n_materials = 2: material[0] the copper of gpis_default_surface_rgb (albedo 1), material[1] Lambert with albedo 0.8; the cap
 * of gpis_default_surface_rgb (cap_cos 0.9781476, radiance 1). */
void gpis_default_materials(gpis_materials_s *mats);

/* gpis_render_scene_s_nee_paths_rgb with the material of every hit chosen by its GP id:
 *     material[gp_id < n_materials ? gp_id : 0]
 * (the reference indexes its table unchecked; the fallback is the Tungsten binding's rule).  Accepts and refuses what
 * gpis_render_scene_s_nee_paths_rgb does, with `mats` in the place of `surf` (cap_cos outside (-1, 1) included), and refuses
 * (GPIS_ERR_INVALID_ARG, nothing written) n_materials outside 1 .. GPIS_MAX_MATERIALS and a type outside gpis_material_type in
 * any of the n_materials entries.
 * Per sample, operation for operation in float with contraction off.  Everything up to the material is
 * gpis_render_scene_s_nee_paths_rgb verbatim: the PCG32 stream and the camera step, the segment words, step 1 (which segments are
 * marched, with and without emission), step 2 (the emission with thr BEFORE the weight, then thr[c] = thr[c] * weight[c]), no
 * Russian roulette, one jitter per shadow segment that is marched (the light's first), and the copy of the state at the hit that
 * the shadow segments and the next segment start from (segment word + 1, last_gp_id = the hit's id).  Then, per hit:
 *   CONDUCTOR: steps 3-7 of gpis_render_scene_s_nee_paths_rgb with the material's eta, k, albedo and the table's cap.
 *   LAMBERT (BRDFPhaseFunction over LambertBsdf, LambertBsdf.cpp:27-68, under a non-Dirac light): both estimators run, with the
 *   power heuristic, WHATEVER scheme the segment reports (TraceBase.cpp:354, 380, 396, 415 ask isSpecular() first), and there is
 *   no neePDF / neeGrad query.  Frame and wi as in the conductor step; pdf_l = (0.5f * (1.0f/3.1415926536f)) / (1.0f - cap_cos).
 *     L1. Light sample.  The cap direction d by the draws of the conductor's light sample (z, then the disk pairs), always;
 *         wo = normalized(to_local(frame, d)); f[c] = albedo[c] * (1.0f/3.1415926536f) * wo.z if wi.z > 0 && wo.z > 0, else 0.
 *         The shadow segment is marched iff some f[c] != 0 and the chord from the hit along d exists; it starts from the state
 *         copy with last_aniso = the hit's own aniso (no evalGrad: TraceBase.cpp:371 is specular-only).
 *         lightF[c] = f[c] * cap_radiance[c] / pdf_l, times power_heuristic(pdf_l, wo.z * (1.0f/3.1415926536f)).
 *     L2. Phase sample, only if wi.z > 0 (otherwise no draws).  One cosine direction wo_p by unit-disk rejection (dx, dy pairs
 *         until d2 = dx*dx + dy*dy satisfies d2 < 1; z = sqrtf(max(1 - d2, 0))), w_p = normalized(to_global(frame, wo_p)).  It
 *         counts iff !(dot(w_p, capDir) < cap_cos) and the chord along w_p exists; then its shadow segment is marched.
 *         phaseF[c] = cap_radiance[c] * albedo[c], times power_heuristic(wo_p.z * (1.0f/3.1415926536f), pdf_l).
 *     L3. L and em[c] = em[c] + thr[c] * L[c] as step 6 of gpis_render_scene_s_nee_paths_rgb (the all-channels-zero cap_radiance
 *         rule included).
 *     L4. The bounce (handleVolume, TraceBase.cpp:552, draws a second, independent sample): wi.z <= 0 ends the path without a
 *         draw; otherwise another disk-rejection cosine direction w and thr[c] = thr[c] * albedo[c]; max(thr) == 0 ends the path;
 *         chord, next ray and next jitter as in the conductor step.
 *   Order of draws at a Lambert hit: the light direction, the phase direction, the shadow jitters (the light's first, only for
 *   the segments marched), the bounce direction, the next segment's jitter.  This is the one difference from the serial
 *   reference beside the rejection samplers: the serial code draws the light's jitter before the phase direction, and the staged
 *   kernels need both directions at set-up (as the conductor step needs its two jitters ahead).
 * Image, counts, accumulation and the independence of cuts, chunks and tuning options are those of
 * gpis_render_scene_s_nee_paths_rgb.  Consequences: a table whose entries all equal one conductor gives that entry's frame bit
 * for bit; on a medium whose ids are all 0, material[1..] changes nothing.  Asynchronous on `stream`. */
int gpis_render_scene_s_material_paths_rgb(gpis_medium *m, const gpis_scene_s *s, const gpis_materials_s *mats, int max_path_bounces,
                                           float *radiance_sum3, uint32_t *seg_count, void *stream);

/* gpis_render_scene_s_material_paths_rgb — the same estimator, sample for sample — under the sample schedule of
 * gpis_render_scene_s_adaptive, exactly as gpis_render_scene_s_nee_paths_rgb_adaptive runs gpis_render_scene_s_nee_paths_rgb: its
 * pass loop, records, camera step, clamp, luminance statistics and sums.  Refuses what either of those two entries refuses. */
extern int gpis_render_scene_s_material_paths_rgb_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                           const gpis_materials_s *mats, int max_path_bounces,
                                                           float *radiance_sum3, uint32_t *sample_count, uint32_t *seg_count,
                                                           gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);

/* ---- weight-space GP medium (WeightSpaceGaussianProcessMedium.cpp, WeightSpaceGaussianProcess.cpp) --------------------
 * The field of one realization is  f(p) = sqrt(cov(p,p)) * (sqrt(2/N) * sum_i w_i cos((d_i . p) * omega_i + phi_i)) + mean(p)
 * with N random Fourier features of the squared-exponential covariance (WSG:120-127, 160-240).  A realization is fixed by the
 * pixelSampleSegment word pss = (pixel.x, pixel.y, spp, segment): the basis (phi_i, then the spectral sample d_i * omega_i,
 * 5 uniforms per function) comes from a PCG32 stream seeded with xxhash32(pss), the weights w_i (standard normals, pairs of
 * Box–Muller) from a stream seeded with seed + xxhash32(pss).  single_realization: pss = (0,0,0,0) for every ray; correlation
 * context GLOBAL: pss.w = 0; the other contexts: a new realization on every segment (WSM:159-180).
 *
 * gpis_ws_create reads these fields of gpis_params: step_size (> 0; 0 is the affine-arithmetic sphere trace, refused), min_step,
 * seed, single_realization, correlation_context, max_bounces, sigma_a, sigma_s, density, sigma, length_scale, aniso, mean,
 * has_mean_additional, mean_additional, mean_color (ramp types only), kernel_type (squared exponential only), nonstationary and
 * grid_nonstationary (must be 0).  use_aniso_mtx / aniso_mtx are accepted and ignored: the reference's spectral sampler reads only
 * the "aniso" vector (GPF.hpp:1812-1815).  Everything else of gpis_params is ignored.
 * Refused with GPIS_ERR_UNSUPPORTED: step_size == 0, kernels other than squared exponential and the non-stationary wrappers
 * (their spectral samplers draw from std::mt19937 / std::gamma_distribution), normal methods beckmann / ggx, intersect method
 * mean, basis_functions outside 0..GPIS_WS_MAX_BASIS.
 *
 * rays[i].u_jitter is the one sampler.next1D() of the march (WSM:247).  All results are bit-identical to the reference's double
 * evaluation.  The device restates glibc's cos / sin for |x| < 105414350 only: an entry for which one of the evaluations the
 * reference performs met a larger argument returns GPIS_ERR_UNSUPPORTED (results are written but must not be used); march points
 * the device evaluated ahead and discarded do not count.  For that check the ws batch entries synchronise `stream` before they
 * return.  min_step 0 is accepted with the reference's arithmetic: (far - near) / 0.0f is +inf (the step is step_size), or NaN
 * when far == near (no march point). */
#define GPIS_WS_PARAMS_VERSION 1
#define GPIS_WS_MAX_BASIS 1024
typedef enum gpis_normal_method {
    GPIS_NORMAL_CONDITIONED_GAUSSIAN = 0,   /* "conditioned_gaussian": the analytic gradient of the realization (WSG:50-76) */
    GPIS_NORMAL_FINITE_DIFFERENCES = 1,     /* "finite_differences": central differences, float eps = 1e-4 (WSM:89-114) */
    GPIS_NORMAL_BECKMANN = 2,               /* refused */
    GPIS_NORMAL_GGX = 3                     /* refused */
} gpis_normal_method;
typedef enum gpis_intersect_method { GPIS_INTERSECT_GP_DISCRETE = 0, GPIS_INTERSECT_MEAN = 1 /* refused */ } gpis_intersect_method;
typedef struct gpis_ws_params {
    uint32_t version;                /* must be GPIS_WS_PARAMS_VERSION */
    int32_t basis_functions;         /* "basis_functions" (0 .. GPIS_WS_MAX_BASIS; default 300; 0 = the mean alone) */
    int32_t normal_method;           /* "normal_method" gpis_normal_method */
    int32_t intersect_method;        /* "intersect_method" gpis_intersect_method */
    int32_t _pad[4];
} gpis_ws_params;
/* One point query of gpis_ws_eval_batch: the realization of (pixel, spp, segment) under the medium's rule above.  48 bytes. */
typedef struct gpis_ws_query {
    double p[3];
    uint32_t pixel[2];
    uint32_t spp;
    uint32_t segment;
    uint32_t _pad[2];
} gpis_ws_query;

/* Fills `p` with the reference's defaults (WSM:21-32, GPM.cpp:86-95). */
void gpis_ws_default_params(gpis_ws_params *p);
/* WeightSpaceGaussianProcessMedium::fromJson + prepareForRender.  For single_realization the global basis is built on the device
 * here.  The handle is freed by gpis_destroy; it is accepted by the gpis_ws_* entries only (the other entries return
 * GPIS_ERR_INVALID_ARG for it, and the gpis_ws_* entries for any other handle). */
int gpis_ws_create(const gpis_params *params, const gpis_ws_params *ws, int device, gpis_medium **out);
/* Medium::sampleDistance / transmittance (GPM.cpp:221-393 over WSM:64-291), device pointers, one wave per segment. */
int gpis_ws_sample_distance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, void *stream);
int gpis_ws_transmittance_batch(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible, void *stream);
/* The same for host pointers (synchronous; what integration/HipWeightSpaceMedium.cpp calls with a batch of one). */
int gpis_ws_sample_distance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out);
int gpis_ws_transmittance_host(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible);
/* Test surface: WeightSpaceRealization::evaluate (value, gp id) and the medium's normal method's gradient (evaluateGradient, or
 * the six-point finite differences) at q[i].p.  Device pointers; value, grad3 (xyz triples) and gp_id may each be NULL. */
int gpis_ws_eval_batch(gpis_medium *m, size_t n, const gpis_ws_query *q, double *value, double *grad3, int32_t *gp_id, void *stream);
/* Test surface: the basis and weights of n realizations.  pss4: n words (pixel.x, pixel.y, spp, segment), mapped by the medium's
 * rule above; out: n x N records of 6 doubles (d.x, d.y, d.z, omega, phi, w) in basis order.  Device pointers. */
int gpis_ws_basis_batch(gpis_medium *m, size_t n, const uint32_t *pss4, double *out, void *stream);
/* Evaluations the reference performs (n_eval: value evaluations of the march, gradient evaluations counted once, finite
 * differences six times), evaluations the device computed (n_spec >= n_eval: speculative march positions included) and
 * segments since the last reset.  Synchronises the device. */
int gpis_ws_get_counters(gpis_medium *m, uint64_t *n_eval, uint64_t *n_spec, uint64_t *n_seg);
int gpis_ws_reset_counters(gpis_medium *m);
/* gpis_render_scene_s over the weight-space medium.  Covers the rows [y_begin, y_begin+y_count), the tile-row shard
 * (shard_index / shard_count) and the samples [spp_begin, spp_begin+spp_count) that `s` selects.  Per sample: the draws of
 * gpis_render_scene_s (PCG32 seeded with xxhash32(x, y, spp, scene_seed) + 1, then jx, jy, u_march, u_shadow), a primary
 * sampleDistance, Lambert shading against the directional light, and one shadow transmittance per lit hit through a state copy
 * with segment + 1, first_scatter = 0 and last_aniso / last_gp_id / last_val / info_t / bounce carried from the primary result.
 * ACCUMULATES the per-pixel sum, taken in sample order, into radiance_sum[height*width] (float, device pointer, indexed
 * y*width+x; the caller divides by the total spp) and the per-pixel hits into hit_count (device pointer, may be NULL).  The image
 * does not depend on how a frame is cut into calls (rows, shards, spp ranges), nor on the order in which waves finish.
 * One fused kernel, one wave per sample: no ray or segment records in device memory; under single_realization or context GLOBAL
 * the primary's realization serves the shadow segment.  Weight-space handles only (any other handle: GPIS_ERR_INVALID_ARG;
 * gpis_render_scene_s keeps refusing weight-space handles).  Returns GPIS_ERR_UNSUPPORTED under the cos / sin argument rule
 * above, for which it synchronises `stream` once per call.  gpis_ws_get_counters: n_eval counts the reference's evaluations,
 * n_seg the primary segments marched plus the shadow segments marched. */
int gpis_ws_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum, uint32_t *hit_count, void *stream);
/* gpis_render_scene_s_paths over the weight-space medium: the same estimator, operation for operation.  Rows, tile-row shard and
 * spp range as gpis_ws_render_scene_s.  Per sample: PCG32 seeded with xxhash32(x, y, spp, scene_seed) + 1, the draws jx, jy,
 * u_march, the camera ray and its bounding-sphere chord; then for bounce = 0 .. max_path_bounces-1 a sampleDistance with segment
 * word = bounce (!ok ends the path; throughput *= weight[0]; exited ends the path).  On a hit, while bounce < max_path_bounces-1:
 * next-event estimation when wi.z > 0, wo.z > 0 (Duff frame about the normalised aniso) and the light direction has a chord —
 * one shadow transmittance through a state copy with segment bounce+1, first_scatter = 0 and last_aniso / last_gp_id / last_val /
 * info_t / bounce carried from the result, its jitter the next draw of the stream, contributing
 * throughput * (albedo * (1/3.1415926536f) * wo.z * light_radiance) when visible; then the cosine bounce by unit-disk rejection
 * (sqrt only), throughput *= albedo, and — only if the path lives on — the next chord, segment bounce+1 and the next jitter.  The
 * segment of bounce max_path_bounces-1 is marched (it counts below) although nothing after it reaches the image, so
 * max_path_bounces = 1 adds zeros.  A sample's emission is the sum of its contributions in bounce order; ACCUMULATES each pixel's
 * sum of emissions, taken in sample order, into radiance_sum[height*width] (float, device pointer, indexed y*width+x).  The image
 * does not depend on how a frame is cut into calls, nor on the order in which waves finish.  max_path_bounces >= 1, else
 * GPIS_ERR_INVALID_ARG; albedo is taken as given.
 * One fused kernel, one wave per sample, the whole path in the wave: no ray or segment records in device memory.  Under
 * single_realization or context GLOBAL one realization serves the whole path; under the other contexts the shadow segment of
 * bounce b and the path segment of bounce b+1 carry the same segment word b+1 and are marched from one realization.
 * Weight-space handles only (any other handle: GPIS_ERR_INVALID_ARG; gpis_render_scene_s_paths keeps refusing weight-space
 * handles).  Returns GPIS_ERR_UNSUPPORTED under the cos / sin argument rule above, for which it synchronises `stream` once per
 * call.  gpis_ws_get_counters: n_eval counts the reference's evaluations, n_seg the path segments marched plus the shadow
 * segments marched. */
int gpis_ws_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo,
                                 float *radiance_sum, void *stream);

/* gpis_ws_render_scene_s and gpis_ws_render_scene_s_paths — the same estimators, sample for sample — under the sample schedule of
 * gpis_render_scene_s_adaptive.  Weight-space handles only; s->spp_count is the AVERAGE number of samples per pixel, S.
 * Pass loop, records, RNG: exactly those of gpis_render_scene_s_adaptive — the plan step gpis_adaptive_plan_host, the start state
 * gpis_adaptive_rng_init_host, records zeroed at the start, record (x/4) + (y/4) * ceil(W/4), whole frames on one GPU.
 * Sample identity: sample i of a record in a pass is the sample (x, y, k = s->spp_begin + sample_index + i) of
 * gpis_ws_render_scene_s / gpis_ws_render_scene_s_paths: the same PCG32 seed, the same draws, the same pixelSampleSegment words
 * (hence the same realizations and the same realization reuse inside a sample) and the same marches; the DIFFERENCE from the
 * reference's `_currentSpp + i` is the one stated at gpis_render_scene_s_adaptive.
 * Sample value v.  Lambert frame: v = lit ? clamp(cv * light_radiance) : 0, where cv = cos(normal, light) * (visible ? 1 : 0) and
 * lit (a shadow segment was marched) are what gpis_ws_render_scene_s sums; the hit is ok && !exited of the primary segment.  Path
 * driver: v = clamp(emission), the sample's sum of NEE contributions.  clamp: NaN, +-infinite and > 65536 count as 0
 * (PathTraceIntegrator.cpp:149-156), in the image and in the statistics.
 * Statistics: SampleRecord::addSample(float) on v over the tile's pixels row-major, clipped at the image edge, then i.  The path
 * driver is a mono estimator: its statistic is the scalar v itself, as for the Lambert entry — NOT the luminance of a grey Vec3f
 * (0.2126f v + 0.7152f v + 0.0722f v rounds differently).
 * Image: per pixel and pass v is summed in i order from zero; that sum is ACCUMULATED once into radiance_sum[y*width+x], the count
 * into sample_count and the hits into hit_count (device pointers, height*width entries; hit_count may be NULL).  While nothing is
 * clamped a pixel equals bit for bit the sequence of uniform-driver calls over its (spp_begin, spp_count) ranges.
 * records (device pointer, may be NULL) and info (host pointer, may be NULL) are filled as by gpis_render_scene_s_adaptive,
 * including the closing sample_index += next_sample_count.
 * chunk_log2: a pass runs in chunks of 2^chunk_log2 samples, one fused launch each; 0 means 2^22 (the chunk of the uniform
 * drivers), else 8 .. 28.  Cuts fall between records, and a record larger than the chunk is a chunk of its own.  It is an
 * argument because weight-space handles have no gpis_set_option.  No result depends on it.
 * gpis_ws_get_counters: n_eval, n_spec and n_seg advance by exactly what the same samples cost through the uniform entries.
 * The cos / sin argument rule above is read at each pass's synchronisation; on a hit the entry returns GPIS_ERR_UNSUPPORTED at
 * once (what was written must not be used).
 * GPIS_ERR_INVALID_ARG, nothing written: a handle that is not weight-space, rows other than the whole image or shard_count > 1,
 * spp_step == 0, threshold < 2, spp_count == 0, a NULL s / a / radiance_sum / sample_count, chunk_log2 outside {0, 8 .. 28},
 * max_path_bounces < 1.  GPIS_ERR_UNSUPPORTED: a plan that gives a record 0 or more than 2^28 / 16 samples per pixel in a pass; a
 * chunk whose samples plus the resident grid reach 2^32 (the work counter).
 * The entries SYNCHRONISE `stream` once per pass and return with the stream idle. */
extern int gpis_ws_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int chunk_log2,
                                           float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count,
                                           gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);
extern int gpis_ws_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a, int chunk_log2,
                                                 int max_path_bounces, float albedo,
                                                 float *radiance_sum, uint32_t *sample_count,
                                                 gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);

/* gpis_render_scene_s over the function-space medium: the frame of gpis_ws_render_scene_s (above) with this medium's sampler and
 * state.  Covers the rows [y_begin, y_begin+y_count), the tile-row shard (shard_index / shard_count) and the samples
 * [spp_begin, spp_begin+spp_count) that `s` selects.  Per sample (x, y, k): ONE PCG32 stream, set_state(xxhash32(x, y, k,
 * scene_seed) + 1); its first two draws are jx, jy, and the medium draws every later variate from it, as the reference's medium
 * draws from the path's PathSampleGenerator (no u_march / u_shadow is drawn; u_jitter is not read).  The camera ray and its
 * bounding-sphere chord are gpis_render_scene_s's (first_scatter = 1, bounce = 0, segment = 0); a miss contributes nothing.  The
 * primary segment is a sampleDistance from an empty state (has_context = 0) whose sampler_state is the stream after jx, jy; a hit
 * is ok && !exited (!ok is neither a hit nor lit).  Lambert shading against the directional light: n = float(aniso / |aniso|),
 * c = n . l; when c > 0 and (p, l) meets the bounding sphere, one shadow transmittance with near 0, far t1, segment + 1,
 * first_scatter = 0, bounce + 1 and last_aniso / last_gp_id / last_val / info_t + sample_t carried from the primary result.  The
 * shadow segment CONTINUES from the state the primary left — its context (points, derivs, values, sampled_grad, is_intersect)
 * and the sampler where the primary stopped — as in the reference, so Renewal, Renewal+ and Global condition it on the primary's
 * values.  It runs in place on the sample's one state; nothing follows it in this estimator, so that equals running on a copy.
 * Contribution (c * (visible ? 1 : 0)) * light_radiance.
 * ACCUMULATES each pixel's sum, taken in sample order from zero and added once per call, into radiance_sum[height*width] (float,
 * device pointer, indexed y*width+x; the caller divides by the total spp) and the per-pixel hits into hit_count (device pointer,
 * may be NULL).  The image does not depend on how a frame is cut into calls (rows, shards, spp ranges, chunks) nor on the order
 * in which workgroups finish; nothing is added atomically into the image.
 * One fused kernel, one wave per sample in flight, work taken from a global counter: no state, ray or segment record per sample in
 * device memory (one state slot per resident workgroup, 8 B of records per sample of a chunk; GPIS_OPT_CHUNK_LOG2 sets the chunk,
 * 0 = 2^22 samples).  Handles of gpis_create whose parameters the gpis_fs_* entries accept (squared-exponential covariance,
 * analytic mean, 2..64 sample points); anything else, a weight-space handle included: GPIS_ERR_INVALID_ARG.  The entry shares the
 * handle's function-space workspace with the gpis_fs_* batch entries: launches of the SAME handle must be ordered (one stream, or
 * an event between them). */
int gpis_fs_render_scene_s(gpis_medium *m, const gpis_scene_s *s, float *radiance_sum, uint32_t *hit_count, void *stream);
/* gpis_render_scene_s_paths over the function-space medium: the estimator of gpis_ws_render_scene_s_paths (above), operation for
 * operation, with this medium's sampler and state as in gpis_fs_render_scene_s.  Rows, tile-row shard and spp range as the other
 * frame entries.  Per sample (x, y, k): ONE PCG32 stream, set_state(xxhash32(x, y, k, scene_seed) + 1); its first two draws are
 * jx, jy, and every later draw belongs to the medium or to the bounce, in program order (no u_march / u_shadow is drawn; u_jitter
 * is not read).  Camera ray and bounding-sphere chord as gpis_fs_render_scene_s; a miss contributes nothing and marches nothing.
 * The path state starts empty (has_context = 0) with the stream after jx, jy as its sampler.  For bounce b = 0 ..
 * max_path_bounces-1: a sampleDistance on the path state with segment word b (!ok ends the path; throughput *= weight[0]; exited
 * ends the path).  On a hit, while b < max_path_bounces-1: next-event estimation when wi.z > 0, wo.z > 0 (Duff frame about the
 * normalised aniso) and (p, l) has a chord — one shadow transmittance (near 0, far t1, segment b+1, first_scatter = 0, bounce + 1,
 * last_aniso / last_gp_id / last_val / info_t + sample_t carried from the result) on a COPY of the path's state: gpis_fs_state is
 * a value, and the shadow segment never alters the path's context.  The sampler is not copied: the shadow segment draws from the
 * path's stream where the path segment stopped, and the path goes on from where the shadow segment stopped.  Contribution
 * throughput * (((albedo * (1/3.1415926536f)) * wo.z) * light_radiance) when visible.  Then, if wi.z <= 0 the path ends; otherwise
 * the cosine bounce by unit-disk rejection (sqrt only) from the same stream, throughput *= albedo, and — if (p, w) has a chord —
 * segment b+1 on the path's own context: the one the path segment of bounce b left, so Renewal, Renewal+ and Global condition it
 * on that segment's values and not on the shadow segment's.  The segment of bounce max_path_bounces-1 is marched and counted;
 * nothing after it is observable and the driver stops there, so max_path_bounces = 1 adds zeros.
 * A sample's emission is the sum of its contributions in bounce order.  ACCUMULATES each pixel's sum of emissions, taken in sample
 * order from zero and added once per call, into radiance_sum[height*width] (float, device pointer, indexed y*width+x), and per
 * pixel the segments marched, path segments plus shadow segments, into seg_count (device pointer, may be NULL).  The image
 * depends neither on how a frame is cut into calls and chunks nor on the order in which workgroups finish; nothing is added
 * atomically into the image.
 * One fused kernel, one wave per sample in flight, the whole path in the workgroup, work taken from a global counter: no ray,
 * segment or state record per sample in device memory (two state slots per resident workgroup — the path's and the shadow
 * segment's copy — and 8 B of records per sample of a chunk; GPIS_OPT_CHUNK_LOG2 sets the chunk, 0 = 2^22 samples).
 * max_path_bounces >= 1, else GPIS_ERR_INVALID_ARG; albedo is taken as given.  Handles as gpis_fs_render_scene_s: anything it
 * refuses, a weight-space handle included, is GPIS_ERR_INVALID_ARG here (gpis_render_scene_s_paths and
 * gpis_ws_render_scene_s_paths keep their own refusals).  The entry shares the handle's function-space workspace with
 * gpis_fs_render_scene_s and the gpis_fs_* batch entries: launches of the SAME handle must be ordered (one stream, or an event
 * between them). */
int gpis_fs_render_scene_s_paths(gpis_medium *m, const gpis_scene_s *s, int max_path_bounces, float albedo,
                                 float *radiance_sum, uint32_t *seg_count, void *stream);

/* gpis_fs_render_scene_s and gpis_fs_render_scene_s_paths — the same estimators, sample for sample — under the sample schedule of
 * gpis_render_scene_s_adaptive.  Handles as the two uniform entries; s->spp_count is the AVERAGE number of samples per pixel, S.
 * Pass loop, records, RNG: exactly those of gpis_render_scene_s_adaptive — the plan step gpis_adaptive_plan_host, the start state
 * gpis_adaptive_rng_init_host, records zeroed at the start, record (x/4) + (y/4) * ceil(W/4), whole frames on one GPU.
 * Sample identity: sample i of a record in a pass is the sample (x, y, k = s->spp_begin + sample_index + i) of
 * gpis_fs_render_scene_s / gpis_fs_render_scene_s_paths: the same single PCG32 stream set_state(xxhash32(x, y, k, scene_seed) + 1),
 * jx, jy first and every later draw the medium's or the bounce's in program order, the same segment words and the same handling of
 * the state — in the frame driver the shadow segment runs in place on the sample's one state, in the path driver every shadow
 * segment runs on a copy of the path's state and the sampler is not copied.  The DIFFERENCE from the reference's
 * `_currentSpp + i` is the one stated at gpis_render_scene_s_adaptive.
 * Sample value v.  Lambert frame: v = lit ? clamp(cv * light_radiance) : 0, where cv = cos(normal, light) * (visible ? 1 : 0) and
 * lit (a shadow segment was marched) are what gpis_fs_render_scene_s sums; the hit is ok && !exited of the primary segment.  Path
 * driver: v = clamp(emission), the sample's sum of NEE contributions — the scalar, not a luminance.  clamp: NaN, +-infinite and
 * > 65536 count as 0 (PathTraceIntegrator.cpp:149-156), in the image and in the statistics; the segments of a clamped path sample
 * still count.
 * Statistics: SampleRecord::addSample(float) on v over the tile's pixels row-major, clipped at the image edge, then i.
 * Image: per pixel and pass v is summed in i order from zero; that sum is ACCUMULATED once into radiance_sum[y*width+x], the count
 * into sample_count and the hits into hit_count / the segments marched, path plus shadow, into seg_count (device pointers,
 * height*width entries; hit_count / seg_count may be NULL).  While nothing is clamped a pixel equals bit for bit the sequence of
 * uniform-driver calls over its (spp_begin, spp_count) ranges.  Nothing is added atomically into the image, and no result depends
 * on the order in which workgroups finish.
 * max_path_bounces = 1: every sample is zero, so the first pass is rendered and the plan step ends the frame (passes_rendered = 1,
 * stopped_early = 1); seg_count is NOT zero, since the path driver marches and counts the segment of the last bounce.
 * records (device pointer, may be NULL) and info (host pointer, may be NULL) are filled as by gpis_render_scene_s_adaptive,
 * including the closing sample_index += next_sample_count.
 * A pass runs in chunks of 2^GPIS_OPT_CHUNK_LOG2 samples, one fused launch each (0 = 2^22, as the uniform entries).  Cuts fall
 * between records, and a record larger than the chunk is a chunk of its own.  No result depends on it.
 * GPIS_ERR_INVALID_ARG, nothing written: everything the uniform entry refuses (a weight-space handle, parameters outside the
 * function-space scope, max_path_bounces < 1), a NULL s / a / radiance_sum / sample_count, rows other than the whole image or
 * shard_count > 1, spp_step == 0, threshold < 2, spp_count == 0.  GPIS_ERR_UNSUPPORTED: a plan that gives a record 0 or more than
 * 2^28 / 16 samples per pixel in a pass; a chunk whose samples plus the resident grid reach 2^32 (the work counter).
 * The entries SYNCHRONISE `stream` once per pass and return with the stream idle.  They share the handle's function-space
 * workspace, state slots and work counter with the uniform entries and the gpis_fs_* batch entries: launches of the SAME handle
 * must be ordered; two adaptive calls on one handle run one after the other. */
extern int gpis_fs_render_scene_s_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                           float *radiance_sum, uint32_t *sample_count, uint32_t *hit_count,
                                           gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);
extern int gpis_fs_render_scene_s_paths_adaptive(gpis_medium *m, const gpis_scene_s *s, const gpis_adaptive_s *a,
                                                 int max_path_bounces, float albedo,
                                                 float *radiance_sum, uint32_t *sample_count, uint32_t *seg_count,
                                                 gpis_adaptive_record *records, gpis_adaptive_info *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPIS_H_ */
