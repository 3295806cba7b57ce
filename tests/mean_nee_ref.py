"""TEST INFRASTRUCTURE: the media, query sets and frames of the NEE tests with an out-of-line mean (tests/test_mean_nee_cpu.py,
tests/test_gpu_mean_nee.py).

The reference is tests/sdf_march_ref.py's SdfComposite.nee_pdf / nee_grad (tests/grid_march_ref.py's GridComposite inherits them): the
frozen oracle's own neePDF / neeGrad on the same medium with the mean replaced by the LinearMean whose gradient is, in float, exactly the
out-of-line mean's.  That holds for axis-aligned gradients only, so every case SELECTS its queries from a pool by that rule; the numbers
each case rests on (selected queries per gradient class or CSG id, pdf > 0 / pdf == 0) are asserted on the reference alone by
tests/test_mean_nee_cpu.py, which also records them (COUNTS there)."""
import numpy as np

import grid_march_ref as gmr
import sdf_march_ref as smr

f32 = np.float32
N_QUERIES = 512
POOL = 4096

# the four media of tests/test_gpu_parity.py::test_1d_sampling_and_nee: (correlation_context, correlation_xy, scheme_1d)
FAMILY = {
    "renewal+xy-mis": ("RENEWAL_PLUS", 1, "MIS"),
    "renewal+-nee": ("RENEWAL_PLUS", 0, "NEE"),
    "renewal-uni": ("RENEWAL", 0, "UNI"),
    "none-mis": ("NONE", 0, "MIS"),
}
MEANS = ("plane", "plane-x", "plane-z", "plane-min", "knob", "grid-point", "grid-linear", "csg-plane-slab", "csg-slab-plane")
PLANE_SCALE, PLANE_OFFSET = 0.7, 0.1


def c2(pkg, family):
    ctx, xy, scheme = FAMILY[family]
    p = pkg.params_for_config("C2")
    p["correlation_context"] = getattr(pkg.CTX, ctx)
    p["correlation_xy"] = xy
    p["scheme_1d"] = getattr(pkg.SCHEME, scheme)
    return p


def _transform(inv3, shift):
    """the "transform" T of a procedural mean whose inverse is [inv3 | shift]: entries 0 and +-1 and a dyadic translation, so that
    Mat4f::invert returns that inverse exactly"""
    Tinv = np.eye(4)
    Tinv[:3, :3] = inv3
    Tinv[:3, 3] = shift
    return np.linalg.inv(Tinv).astype(f32)


# plane evaluates y of T^-1 p: -x + 0.25 under T_X (the world gradient along -x), z - 0.125 under T_Z (along +z)
T_X = _transform([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], (0.5, 0.25, -0.25))
T_Z = _transform([[1, 0, 0], [0, 0, 1], [0, -1, 0]], (0.25, -0.125, 0.5))


def axis_grid(pkg, interpolate, axis=2):
    """16^3 voxels of size 0.2 about the origin (index = 5 p + 8) whose value varies along one axis only, smoothly and not linearly:
    the mean's one-sided differences along the two other axes are exact zeros"""
    k = np.arange(16)
    line = (0.15 * k - 1.0 + 0.05 * np.sin(1.3 * k)).astype(f32)
    shape = [1, 1, 1]
    shape[2 - axis] = 16                                  # voxels[k, j, i]: z, y, x
    vox = np.broadcast_to(line.reshape(shape), (16, 16, 16))
    T = np.diag([5.0, 5.0, 5.0, 1.0])
    T[:3, 3] = 8.0
    return gmr.grid(pkg, vox, T.astype(f32), interpolate)


def slab_grid(pkg):
    """the slab |x| - 0.45 on the same 16^3 lattice (linear interpolation): a distance field that varies along x only"""
    x = (np.arange(16) - 8.0) / 5.0
    vox = np.broadcast_to((np.abs(x) - 0.45).astype(f32).reshape(1, 1, 16), (16, 16, 16))
    T = np.diag([5.0, 5.0, 5.0, 1.0])
    T[:3, 3] = 8.0
    return gmr.grid(pkg, vox, T.astype(f32), "linear")


def medium(pkg, family, mean):
    """(params, grids, transforms) of one case"""
    base = c2(pkg, family)
    grids, tfs = [None, None], [None, None]
    if mean.startswith("plane"):
        p = smr.procedural(pkg, base, "plane", scale=PLANE_SCALE, offset=PLANE_OFFSET, minimum=PLANE_OFFSET if mean == "plane-min" else None)
        tfs[0] = {"plane-x": T_X, "plane-z": T_Z}.get(mean)
    elif mean == "knob":
        p = smr.procedural(pkg, base, "knob")
    elif mean.startswith("grid"):
        p = gmr.tabulated(pkg, base, offset=0.05, scale=0.9)
        grids[0] = axis_grid(pkg, mean[5:])
    else:
        w = 1 if mean == "csg-plane-slab" else 0             # the slot of the slab
        slots = ("mean", "mean_additional")
        p = gmr.tabulated(pkg, base, slot=slots[w])
        p = smr.procedural(pkg, p, "plane", scale=PLANE_SCALE, offset=PLANE_OFFSET, slot=slots[1 - w])
        p["has_mean_additional"] = 1
        grids[w] = slab_grid(pkg)
    return p, tuple(grids), tuple(tfs)


def composite(pkg, ob, family, mean, threads=8):
    p, grids, tfs = medium(pkg, family, mean)
    return gmr.GridComposite(pkg, ob, p, grids=grids, transforms=tfs, threads=threads)


def pool(mean, seed=23):
    """the pool the queries are selected from: 4096 points of [-1.3, 1.3]^3, float-exact; the point-sampled grid gets 96 more that lie
    within half a difference step (0.0005) below a voxel boundary along z, where its one-sided difference is not zero"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.3, 1.3, (POOL, 3)).astype(f32)
    if mean == "grid-point":
        extra = rng.uniform(-1.3, 1.3, (96, 3))
        extra[:, 2] = (rng.integers(3, 12, 96) + 0.5 - 8.0) / 5.0 - rng.uniform(0.0001, 0.0005, 96)      # index k + 1/2: the sampler's tie
        pts = np.concatenate([extra.astype(f32), pts])
    return pts


def select(comp, points, n=N_QUERIES):
    """the first n points of the pool whose reference gradient is axis-aligned in float, balanced between the zero and the non-zero
    gradients and, for a CSG pair, between the ids, as far as the pool allows: (points, grad, id, pool size used, qualifying points)"""
    _, gid, g = comp.mean(points.astype(np.float64))
    gf = g.astype(f32)
    ok = (gf != 0).sum(axis=1) <= 1
    cls = 2 * gid + (gf != 0).any(axis=1)
    idx = np.nonzero(ok)[0]
    classes = np.unique(cls[idx])
    take = []
    for c in classes:                                       # an equal share per class first, the rest in pool order
        take.extend(idx[cls[idx] == c][:n // len(classes)])
    rest = np.setdiff1d(idx, take)
    take = np.sort(np.concatenate([np.array(take, dtype=np.int64), rest[:max(0, n - len(take))]]))
    return points[take], g[take], gid[take], int(ok.sum())


def case(pkg, ob, family, mean, threads=8):
    """composite, queries, and what the input conditions rest on, from the reference alone"""
    comp = composite(pkg, ob, family, mean, threads)
    pts, g, gid, qualifying = select(comp, pool(mean))
    q = smr.nee_queries(pkg, pts, g, seed=29)
    k, s = comp.nee_standin(q)
    info = dict(qualifying=qualifying, selected=len(q), zero=int((k < 0).sum()), nonzero=int((k >= 0).sum()),
                axes=sorted(set(int(v) for v in k[k >= 0])), negative=int((s < 0).sum()), magnitudes=int(np.unique(s[k >= 0]).size),
                ids=[int((gid == 0).sum()), int((gid == 1).sum())])
    return comp, q, gid, info


_memo = {}


def reference(pkg, ob, family, mean):
    """case() with the reference's nee_pdf / nee_grad, computed once per process and read-only: dict(comp, q, gid, info, pdf, grad)"""
    key = (family, mean)
    if key not in _memo:
        comp, q, gid, info = case(pkg, ob, family, mean)
        r = dict(comp=comp, q=q, gid=gid, info=info, pdf=comp.nee_pdf(q), grad=comp.nee_grad(q))
        for k in ("q", "gid", "pdf", "grad"):
            r[k].setflags(write=False)
        _memo[key] = r
    return _memo[key]


def analytic_plane_nee(comp, q, mean):
    """nee_pdf / nee_grad of a plane case with the reference built from the ANALYTIC gradient of the plane (its own scale along its
    axis, 0 where `min` clips) in place of the one-sided difference: what a device that differentiated the plane exactly would return"""
    axis, sign = {"plane": (1, 1.0), "plane-min": (1, 1.0), "plane-x": (0, -1.0), "plane-z": (2, 1.0)}[mean]
    val = comp.mean(np.asarray(q["p"], dtype=f32).astype(np.float64))[0]
    clipped = (val <= np.float64(f32(PLANE_OFFSET))) if mean == "plane-min" else np.zeros(len(q), dtype=bool)
    pdf, grad = np.zeros(len(q), dtype=f32), np.zeros((len(q), 3), dtype=f32)
    for mask, orc in ((clipped, comp.noise), (~clipped, comp._nee_oracle(axis, f32(sign) * f32(PLANE_SCALE)))):
        i = np.nonzero(mask)[0]
        if len(i):
            pdf[i], grad[i] = orc.nee_pdf(q[i]), orc.nee_grad(q[i])
    return pdf, grad


# ---- frames ------------------------------------------------------------------------------------------------------------------------
# the frame's plane is y of T_X^-1 p = -x + 0.25: the mean 0.7 (0.25 - x) + 0.1 is negative for x > 0.393.  Seen from the camera at
# (0, 0, 4), rays on the right of the image enter that half-space and hit; rays on the left stay in x < 0.39 and miss.
def frame_medium(pkg, scheme="mis"):
    import nee_paths_ref as npr
    p = smr.procedural(pkg, npr._c2(pkg, scheme), "plane", scale=PLANE_SCALE, offset=PLANE_OFFSET)
    return p, (None, None), (T_X, None)


def constant_grid_medium(pkg, scheme="mis"):
    """the constant grid 0.25 with offset 0.25 and scale 0.5 (tests/test_gpu_grid_mean.py::test_constant_grid_anchor_against_the_oracle):
    (params, grids, the homogeneous 0.25 medium the oracle renders)"""
    import nee_paths_ref as npr
    base = npr._c2(pkg, scheme)
    hom = np.array(base)
    hom["mean"]["type"], hom["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.25
    g = gmr.grid(pkg, np.full((8, 8, 8), 0.25, f32), gmr.sphere_world_to_index(8, 0.4), "linear")
    return gmr.tabulated(pkg, base, offset=0.25, scale=0.5), (g, None), hom


def frame_reference(pkg, ob, max_bounces):
    """NeePathsRef.compose on the plane medium of frame_medium, the composite standing in for the oracle (once per process, read-only)"""
    import nee_paths_ref as npr
    key = ("frame", int(max_bounces))
    if key not in _memo:
        p, grids, tfs = frame_medium(pkg)
        comp = gmr.GridComposite(pkg, ob, p, grids=grids, transforms=tfs, threads=8)
        c = npr.NeePathsRef(pkg, ob).compose(comp, npr.frame(ob), pkg.default_surface_s(), max_bounces)
        c.image.setflags(write=False)
        c.seg_count.setflags(write=False)
        _memo[key] = c
    return _memo[key]
