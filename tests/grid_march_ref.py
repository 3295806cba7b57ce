"""TEST INFRASTRUCTURE: the march of a medium with a tabulated (voxel grid) mean, composed on the CPU.

The frozen oracle knows no such mean.  GridComposite is tests/sdf_march_ref.py's SdfComposite — the oracle's noise, the march,
the conditioning and the evaluation counting, all inherited unchanged — with the mean replaced: per slot the value and the gradient
come from tests/sdf_mean_ref.py for the types 0-3 and from tests/grid_mean_ref.py (the C restatement of TabulatedMean) for type 4;
the CSG minimum is GaussianProcess::mean_weight_space's `add < m`.  The colour field is MeanFunction's own (evaluated at the point
itself); the emission is TabulatedMean's override, 0 without an emission grid, when the PRIMARY mean is tabulated
(GaussianProcess::emission asks the primary mean): such a medium is not emissive, so `params` says so and the path composite
(tests/paths_rgb_ref.py) does not march the last segment whose only effect would be an emission of 0."""
import numpy as np

import grid_mean_ref
import sdf_march_ref as smr

f32 = np.float32


def tabulated(pkg, params, offset=0.0, scale=1.0, volume=False, slot="mean"):
    p = np.array(pkg.as_params(params))
    p[slot]["type"] = pkg.MEAN_TYPE.TABULATED
    p[slot]["offset"] = offset
    p[slot]["scale"] = scale
    p[slot]["func"] = 1 if volume else 0
    if slot == "mean_additional":
        p["has_mean_additional"] = 1
    return p


def grid(pkg, voxels, world_to_index, interpolate="linear", origin=(0, 0, 0)):
    """a grid_mean_ref.Grid from the arguments of Medium.set_mean_grid"""
    d, v = pkg.variance_grid_desc(voxels, world_to_index, interpolate, origin)
    return grid_mean_ref.Grid(np.frombuffer(d.tobytes(), dtype=grid_mean_ref.DESC)[0], v)


def set_grid(medium, which, g):
    """hand a grid_mean_ref.Grid (any descriptor, bounds larger than the array included) to gpis_set_mean_grid; a grid whose bounds
    are its array goes through Medium.set_mean_grid just as well"""
    import ctypes
    d, v = np.array(g.desc), g.voxels
    medium.L.check(medium.L.lib.gpis_set_mean_grid(medium.h, int(which), d.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p)),
                   "gpis_set_mean_grid")


class MeanRef:
    """GaussianProcess::mean_weight_space of a gpis_params record whose slots may be tabulated: (value, id, grad).  Needs no oracle."""

    def __init__(self, pkg, params, grids=(None, None), transforms=(None, None)):
        import sdf_mean_ref
        self.pkg = pkg
        self.params = np.array(pkg.as_params(params))
        self.grids, self.transforms = grids, transforms
        self.gref = grid_mean_ref.GridMeanRef()
        self.mref = sdf_mean_ref.SdfMeanRef()

    def _slot(self, w, p):
        mu = self.params["mean_additional" if w else "mean"]
        if int(mu["type"]) == self.pkg.MEAN_TYPE.TABULATED:
            return self.gref.mean(self.grids[w], p, offset=mu["offset"], scale=mu["scale"], volume=int(mu["func"]) != 0)
        one = np.array(self.params)
        one["mean"] = mu
        one["has_mean_additional"] = 0
        v, _, g = self.mref.mean(one, p, (self.transforms[w], None))
        return v, g

    def mean(self, points):
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        m, g = self._slot(0, p)
        gid = np.zeros(p.shape[0], dtype=np.int32)
        if int(self.params["has_mean_additional"]):
            add, ga = self._slot(1, p)
            pick = add < m
            m = np.where(pick, add, m)
            g = np.where(pick[:, None], ga, g)
            gid = pick.astype(np.int32)
        return m, gid, g


class GridComposite(smr.SdfComposite):
    def __init__(self, pkg, ob, params, grids=(None, None), transforms=(None, None), threads=16):
        super().__init__(pkg, ob, params, transforms=transforms, threads=threads)
        self.means = MeanRef(pkg, params, grids, transforms)
        self.primary_tabulated = int(self.params["mean"]["type"]) == pkg.MEAN_TYPE.TABULATED
        if self.primary_tabulated:
            self.params["mean_emission"]["enabled"] = 0

    def mean(self, points):
        return self.means.mean(points)

    def mean_color_emission(self, points):
        if not self.primary_tabulated:
            return super().mean_color_emission(points)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        col, _ = self.noise.mean_color_emission(p)
        return col, np.zeros((p.shape[0], 3), dtype=f32)


# ---- the test grids (a numpy formula each: no voxel file is committed) and the point classes of the lookup --------------------------
DIMS = (9, 11, 13)                  # x, y, z
ORIGIN = (-4, -5, -6)


def world_to_index():
    """rotation x non-uniform scale x translation (row-major Mat4f): the ball of radius 1.5 lands around the (9, 11, 13) box"""
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    tr = np.array([[1, 0, 0, 0.2], [0, 1, 0, -0.1], [0, 0, 1, 0.3], [0, 0, 0, 1.0]])
    return (tr @ np.diag([4 / 1.5, 5 / 1.5, 6 / 1.5, 1.0]) @ rot).astype(f32)


def demo_voxels(seed=7):
    """voxels[k, j, i] of the (9, 11, 13) grid: a smooth field plus noise, negative values included"""
    nx, ny, nz = DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    rng = np.random.default_rng(seed)
    return (np.sin(0.7 * i) + 0.5 * np.cos(0.5 * j) + 0.1 * k - 0.4 + 0.25 * rng.standard_normal((nz, ny, nx))).astype(f32)


def demo_grid(pkg, interpolate, wide_bounds=False):
    """the (9, 11, 13) grid at origin (-4, -5, -6); wide_bounds: bounds() reaches 4 voxels past the array on every side, so the clamp
    lets the samplers read neighbours outside the array (the background 0)"""
    g = grid(pkg, demo_voxels(), world_to_index(), interpolate, ORIGIN)
    if wide_bounds:
        g.desc["bounds_min"] = g.desc["bounds_min"] - 4
        g.desc["bounds_max"] = g.desc["bounds_max"] + 4
    return g


def index_coords(g, points):
    """invNaturalTransform * Vec3f(p) in float, left to right (Mat4f.hpp:168-175), before the clamp: (n, 3) float32"""
    T = g.desc["inv_natural_transform"].reshape(4, 4)
    x, y, z = (np.asarray(points)[:, c].astype(f32) for c in range(3))
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def numpy_density(g, points):
    """VdbGrid::density in numpy: (density float32, classes) with classes a dict of boolean masks over the points"""
    d = g.desc
    dims, org = [int(v) for v in d["dims"]], [int(v) for v in d["origin"]]
    vox = g.voxels.reshape(dims[2], dims[1], dims[0])
    raw = index_coords(g, points)
    lo, hi = (d["bounds_min"] + f32(2)).astype(f32), (d["bounds_max"] - f32(3)).astype(f32)
    q = np.minimum(np.maximum(raw, lo[None, :]), hi[None, :]).astype(f32)
    qd = q.astype(np.float64)

    def at(i, j, k):
        i, j, k = i - org[0], j - org[1], k - org[2]
        inside = (i >= 0) & (j >= 0) & (k >= 0) & (i < dims[0]) & (j < dims[1]) & (k < dims[2])
        v = vox[np.clip(k, 0, dims[2] - 1), np.clip(j, 0, dims[1] - 1), np.clip(i, 0, dims[0] - 1)]
        return np.where(inside, v, f32(0)), inside

    unclamped = (raw == q).all(axis=1)
    classes = {
        "integer": unclamped & (qd == np.floor(qd)).any(axis=1),
        "negative": unclamped & ((qd < 0) & (qd != np.floor(qd))).any(axis=1),
        "tie": unclamped & ((qd - np.floor(qd)) == 0.5).any(axis=1),
    }
    for c, name in enumerate("xyz"):
        classes["below " + name] = raw[:, c] < lo[c]
        classes["above " + name] = raw[:, c] > hi[c]
    if int(d["interpolate"]) == 0:
        idx = [np.floor(qd[:, c] + 0.5).astype(np.int64) for c in range(3)]
        v, inside = at(*idx)
        classes["outside"] = ~inside
        return v.astype(f32), classes
    fl = np.floor(qd)
    i, j, k = (fl[:, c].astype(np.int64) for c in range(3))
    u, v, w = (qd[:, c] - fl[:, c] for c in range(3))

    def lerp(a, b, t):
        return (a + ((b - a).astype(f32).astype(np.float64) * t).astype(f32)).astype(f32)

    corner, ins = {}, []
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                corner[di, dj, dk], inside = at(i + di, j + dj, k + dk)
                ins.append(inside)
    ins = np.stack(ins)
    classes["outside"] = ins.any(axis=0) & ~ins.all(axis=0)           # some corners in the array, some in the background
    res = lerp(lerp(lerp(corner[0, 0, 0], corner[0, 0, 1], w), lerp(corner[0, 1, 0], corner[0, 1, 1], w), v),
               lerp(lerp(corner[1, 0, 0], corner[1, 0, 1], w), lerp(corner[1, 1, 0], corner[1, 1, 1], w), v), u)
    return res, classes


def _exact_preimages(g, targets, rng):
    """world points (float-exact doubles) of which at least one index coordinate lands EXACTLY on the target's: the double preimage
    of each target, narrowed, and its neighbours a few ulps away, kept where the float arithmetic of the lookup hits the target"""
    T = g.desc["inv_natural_transform"].reshape(4, 4).astype(np.float64)
    inv = np.linalg.inv(T)
    w0 = (np.c_[targets, np.ones(len(targets))] @ inv.T)[:, :3].astype(f32)
    cand = [w0]
    for _ in range(8):
        steps = rng.integers(-3, 4, w0.shape)
        w = w0.copy()
        for s in range(1, 4):
            w = np.where(steps >= s, np.nextafter(w, f32(np.inf)), w)
            w = np.where(steps <= -s, np.nextafter(w, f32(-np.inf)), w)
        cand.append(w.astype(f32))
    cand = np.concatenate(cand)
    tgt = np.concatenate([targets] * 9).astype(f32)
    keep = (index_coords(g, cand) == tgt).any(axis=1)
    return np.unique(cand[keep], axis=0).astype(np.float64)


def demo_points(g, seed=11):
    """2 000 uniform world points of [-2.2, 2.2]^3 (past every face of the clamp box) plus points whose index coordinates are exact
    integers, exact halves (the point sampler's ties) and negative"""
    rng = np.random.default_rng(seed)
    uni = rng.uniform(-2.2, 2.2, (2000, 3))
    ii, jj, kk = np.meshgrid(np.arange(-2, 3), np.arange(-3, 4), np.arange(-4, 5), indexing="ij")
    lattice = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1).astype(np.float64)
    lattice = lattice + rng.uniform(-0.4, 0.4, lattice.shape) * (rng.random(lattice.shape) < 0.5)     # some coordinates off the lattice
    ints = _exact_preimages(g, np.round(lattice), rng)
    ties = _exact_preimages(g, np.floor(lattice) + 0.5, rng)
    return np.concatenate([uni, ints, ties])


def sphere_voxels(n=24, voxel=0.125):
    """the SDF of the unit-ish scene of the march tests, sampled on n^3 voxels of size `voxel` centred on the origin: a sphere of
    radius 0.8 about (0, 0, 0) united with a sphere of radius 0.45 about (0.7, 0.5, 0.1) (the minimum of the two distances)"""
    c = (np.arange(n) - (n - 1) / 2) * voxel
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    a = np.sqrt(x * x + y * y + z * z) - 0.8
    b = np.sqrt((x - 0.7) ** 2 + (y - 0.5) ** 2 + (z - 0.1) ** 2) - 0.45
    return np.minimum(a, b).astype(f32)


def sphere_world_to_index(n=24, voxel=0.125, angle=0.35):
    """world -> index of sphere_voxels, the grid rotated by `angle` about (1, 1, 0) / sqrt(2) (not axis-aligned) and shifted"""
    ax = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R / voxel
    M[:3, 3] = (n - 1) / 2 + R @ np.array([0.03, -0.02, 0.04]) / voxel
    return M.astype(f32)
