"""The references of the tabulated mean (GPIS_MEAN_TABULATED), on the CPU.

(a) The raw density of tests/native/grid_mean_ref.c (the C restatement of VdbGrid::density over a dense array) equals the frozen
    oracle's grid_unscaled_variance (offset 0, scale 1: the same lookup, written for GridNonstationaryCovariance) and a numpy
    statement of clamp + Point / Box sampler, on the (9, 11, 13) grid at origin (-4, -5, -6) under a rotation x non-uniform scale x
    translation, over 2 000 uniform points and the classes where a lookup goes wrong — each asserted non-empty.
(b) TabulatedMean::mean / dmean_da of the C file against a numpy statement in double: the order of the four evaluations, the double
    eps, the "volume" branch on both sides of 0.0001 and below zero.
(c) The anchor against the oracle itself: a constant grid makes the mean (c + offset) * scale with gradient exactly 0, so the
    march composite of tests/grid_march_ref.py must equal the oracle's homogeneous-mean medium in every gpis_seg_out field and
    coefficient, and the CSG pair (tabulated constant 100, spherical) the oracle's (homogeneous 100, spherical) medium."""
import ctypes
import math

import numpy as np
import pytest

import grid_march_ref as gmr
import grid_mean_ref
import sdf_march_ref as smr
import test_sdf_march_cpu as cpu

pytestmark = pytest.mark.skipif(not grid_mean_ref.available(), reason="no C compiler for the restatement")

f32 = np.float32
N = 321


@pytest.fixture(scope="module")
def gref():
    return grid_mean_ref.GridMeanRef()


def _oracle_with_grid(pkg, ob, g):
    """the oracle's GridNonstationaryCovariance medium over the grid g, offset 0 and scale 1: grid_unscaled_variance is the density"""
    p = pkg.params_for_config("C3")
    p["grid_nonstationary"] = 1
    p["grid_offset"], p["grid_scale"] = 0.0, 1.0
    orc = ob.Oracle(p)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert orc.lib.oracle_set_variance_grid(orc.h, vp(g.desc), vp(g.voxels)) == 0
    return orc


# ---- (a) the lookup ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_bounds", (False, True), ids=("bounds=array", "bounds>array"))
@pytest.mark.parametrize("interpolate", ("linear", "point"))
def test_density_equals_the_oracle_and_numpy(pkg, ob, gref, interpolate, wide_bounds):
    g = gmr.demo_grid(pkg, interpolate, wide_bounds)
    pts = gmr.demo_points(g)
    want, classes = gmr.numpy_density(g, pts)
    counts = {k: int(v.sum()) for k, v in classes.items()}
    print(interpolate, "wide" if wide_bounds else "tight", len(pts), counts)
    need = ["integer", "negative", "tie"]
    if wide_bounds:
        need.append("outside")            # +1 neighbours (or the nearest voxel) beyond the array: the background 0
    else:
        need += ["%s %s" % (side, axis) for side in ("below", "above") for axis in "xyz"]     # beyond each face of the clamp box
        assert counts["outside"] == 0
    for k in need:
        assert counts[k] > 0, (k, counts)
    got = gref.density(g, pts)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, pts[bad[:4]], got[bad[:4]], want[bad[:4]])
    orc = _oracle_with_grid(pkg, ob, g).grid_unscaled_variance(pts)
    bad = np.nonzero(got.view(np.uint32) != orc.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, pts[bad[:4]], got[bad[:4]], orc[bad[:4]])
    assert np.unique(got).size > 100


def test_floor_not_truncation(pkg, gref):
    """a negative, non-integer index coordinate: floor(-1.25) = -2 and weight 0.75, where a truncation would read voxel -1"""
    vox = np.arange(8 * 8 * 8, dtype=f32).reshape(8, 8, 8)
    g = gmr.grid(pkg, vox, np.eye(4, dtype=f32), "linear", origin=(-4, -4, -4))
    p = np.array([[-1.25, -0.5, -1.0]])
    at = lambda i, j, k: float(vox[k + 4, j + 4, i + 4])
    lo = 0.5 * (at(-2, -1, -1) + at(-2, 0, -1))
    hi = 0.5 * (at(-1, -1, -1) + at(-1, 0, -1))
    assert gref.density(g, p)[0] == f32(lo + 0.75 * (hi - lo))
    g0 = gmr.grid(pkg, vox, np.eye(4, dtype=f32), "point", origin=(-4, -4, -4))
    assert gref.density(g0, np.array([[-1.5, -0.5, -1.0]]))[0] == f32(at(-1, 0, -1))          # ties round up: floor(x + 0.5)


# ---- (b) mean and dmean_da -----------------------------------------------------------------------------------------------------
_host_log = np.frompyfunc(math.log, 1, 1)          # the host libm's log, which the C restatement links (numpy's own may differ by an ulp)


def _log(x):
    return _host_log(np.asarray(x, dtype=np.float64)).astype(np.float64)


def _numpy_mean(g, pts, offset, scale, volume):
    """TabulatedMean::mean in double over the numpy density"""
    res = gmr.numpy_density(g, pts)[0].astype(np.float64) if g is not None else np.zeros(len(pts))
    if volume:
        res = -_log(np.where(0.0001 > res, 0.0001, res))
    return (res + np.float64(f32(offset))) * np.float64(f32(scale))


@pytest.mark.parametrize("volume", (False, True))
@pytest.mark.parametrize("interpolate", ("linear", "point"))
def test_mean_and_gradient_equal_the_numpy_statement(pkg, gref, interpolate, volume):
    g = gmr.demo_grid(pkg, interpolate)
    pts = gmr.demo_points(g)[::3]
    offset, scale = 0.3, 0.7
    val, grad = gref.mean(g, pts, offset, scale, volume)
    eps = 0.001                                        # the double 0.001, not double(0.001f)
    assert np.float64(f32(0.001)) != eps
    base = _numpy_mean(g, pts, offset, scale, volume)
    if volume:
        dens = gmr.numpy_density(g, pts)[0]
        assert (dens < 0.0001).any() and (dens > 0.0001).any()          # both sides of max(0.0001, res)
    assert np.array_equal(val, base)
    for c in range(3):
        step = np.zeros(3)
        step[c] = eps
        assert np.array_equal(grad[:, c], (_numpy_mean(g, pts + step, offset, scale, volume) - base) / eps), c
    assert grad.any()
    if interpolate == "point":        # piecewise constant: the gradient is 0 except across a voxel face
        return
    assert (grad != 0).any(axis=1).mean() > 0.5
    # double(0.001f) as eps gives other gradients on the same points: the statement above tells the two apart
    e32 = np.float64(f32(0.001))
    other = (_numpy_mean(g, pts + np.array([e32, 0, 0]), offset, scale, volume) - base) / e32
    assert not np.array_equal(other, grad[:, 0])


def test_evaluation_order_of_the_gradient(pkg, gref):
    """(vals[k] - vals[3]) / eps with vals[3] = mean(a): on a grid that is linear in x the x difference is the slope and y, z are 0"""
    k, j, i = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    g = gmr.grid(pkg, (0.25 * i).astype(f32), np.eye(4, dtype=f32), "linear")
    pts = np.random.default_rng(2).uniform(2.1, 3.9, (64, 3))
    val, grad = gref.mean(g, pts, 0.0, 2.0)
    assert np.allclose(grad[:, 0], 0.5, rtol=0, atol=1e-3) and (grad[:, 0] > 0).all()
    assert np.array_equal(grad[:, 1:], np.zeros((64, 2)))
    assert np.allclose(val, 0.5 * pts[:, 0], rtol=0, atol=1e-6)


def test_volume_branch_around_its_floor(pkg, gref):
    """res above, at and below 0.0001, and negative.  0.0001 is no float: `at` is the float nearest to it, which lies BELOW the double
    0.0001 (so a comparison in float would keep it and a comparison in double replaces it), and the next float up lies above"""
    near = f32(0.0001)
    up = np.nextafter(near, f32(1))
    assert np.float64(near) < 0.0001 < np.float64(up)
    pts = np.array([[3.3, 3.4, 3.6]])
    for c, floored in ((f32(0.5), False), (up, False), (near, True), (f32(0.00001), True), (f32(0), True), (f32(-2.5), True)):
        g = gmr.grid(pkg, np.full((8, 8, 8), c, f32), np.eye(4, dtype=f32), "linear")
        val, grad = gref.mean(g, pts, 0.25, 3.0, volume=True)
        res = 0.0001 if floored else np.float64(c)
        want = (-math.log(res) + 0.25) * 3.0
        assert val[0] == want, (c, val[0], want)
        assert np.array_equal(grad, np.zeros((1, 3)))
    # the two sides of the floor give different values: the float nearest 0.0001 is floored, its upper neighbour is not
    a = gref.mean(gmr.grid(pkg, np.full((8, 8, 8), near, f32), np.eye(4, dtype=f32)), pts, volume=True)[0][0]
    b = gref.mean(gmr.grid(pkg, np.full((8, 8, 8), up, f32), np.eye(4, dtype=f32)), pts, volume=True)[0][0]
    c = gref.mean(gmr.grid(pkg, np.full((8, 8, 8), f32(-1), f32), np.eye(4, dtype=f32)), pts, volume=True)[0][0]
    assert a == c and b < a


def test_no_grid_is_the_background(gref):
    pts = np.random.default_rng(0).uniform(-1, 1, (17, 3))
    val, grad = gref.mean(None, pts, 0.5, 2.0)
    assert np.array_equal(val, np.full(17, 1.0)) and not grad.any()
    val, _ = gref.mean(None, pts, 0.5, 2.0, volume=True)
    assert np.array_equal(val, np.full(17, (-math.log(0.0001) + 0.5) * 2.0))


# ---- (c) the anchor against the oracle -----------------------------------------------------------------------------------------
def _constant_grid(pkg, c):
    return gmr.grid(pkg, np.full((8, 8, 8), c, f32), gmr.sphere_world_to_index(8, 0.4), "linear")


def _same(a, b, fields):
    cpu._same(a, b, fields)


@pytest.mark.parametrize("name", ("none", "renewal", "renewal+", "1d_mis"))
def test_constant_grid_is_the_homogeneous_mean(pkg, ob, name):
    """(0.25 + 0.25) * 0.5 = 0.25, every step exact: the oracle's homogeneous mean of offset 0.25.  First-scatter and
    continued segments (Renewal+ and the 1D scheme condition on the gradient, which is exactly 0 on both sides)."""
    base = cpu.base(pkg, name)
    hom = np.array(base)
    hom["mean"]["type"], hom["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.25
    orc = ob.Oracle(hom, threads=8)
    params = gmr.tabulated(pkg, base, offset=0.25, scale=0.5)
    comp = gmr.GridComposite(pkg, ob, params, grids=(_constant_grid(pkg, 0.25), None), threads=8)
    pts = np.random.default_rng(3).uniform(-1.5, 1.5, (257, 3))
    v, gid, g = comp.mean(pts)
    assert np.array_equal(v, np.full(257, 0.25)) and not g.any() and not gid.any()
    rays = smr.camera_rays(pkg, N, 5)
    want, wcoeff = orc.sample_distance(rays, want_coeff=True)
    rays2 = cpu.continued_rays(pkg, want, 6)
    for r in (rays, rays2):
        w, wc = orc.sample_distance(r, want_coeff=True)
        got, coeff = comp.sample_distance(r, want_coeff=True)
        assert (w["exited"] == 0).sum() >= N // 10 and (w["exited"] != 0).sum() >= N // 10
        _same(got, w, pkg.SEG_OUT.names)
        _same(coeff, wc, ("value_scale", "gradient_scale", "ray_origin"))
        if name != "1d_mis":
            _same(coeff, wc, ("n_evals",))
        assert np.array_equal(comp.transmittance(r), orc.transmittance(r))


@pytest.mark.parametrize("order", ("tabulated first", "tabulated second"))
def test_csg_pair_with_a_constant_grid(pkg, ob, order):
    """(tabulated constant 0.25 + 99.75 = 100, spherical) is the oracle's (homogeneous 100, spherical) medium, in either slot order"""
    base = cpu.base(pkg, "renewal")
    sph = np.array(pkg.default_params()["mean"])
    sph["type"], sph["radius"], sph["center"] = pkg.MEAN_TYPE.SPHERICAL, 0.8, (0.1, 0.0, -0.1)
    hom = np.array(sph)
    hom["type"], hom["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 100.0
    tab_slot, sph_slot = ("mean", "mean_additional") if order == "tabulated first" else ("mean_additional", "mean")
    want_p = np.array(base)
    want_p["has_mean_additional"] = 1
    want_p[tab_slot], want_p[sph_slot] = hom, sph
    params = np.array(want_p)
    params = gmr.tabulated(pkg, params, offset=99.75, scale=1.0, slot=tab_slot)
    w = 0 if tab_slot == "mean" else 1
    grids = [None, None]
    grids[w] = _constant_grid(pkg, 0.25)
    comp = gmr.GridComposite(pkg, ob, params, grids=tuple(grids), threads=8)
    orc = ob.Oracle(want_p, threads=8)
    rays = smr.camera_rays(pkg, N, 5)
    want, wcoeff = orc.sample_distance(rays, want_coeff=True)
    got, coeff = comp.sample_distance(rays, want_coeff=True)
    assert (want["exited"] == 0).sum() >= N // 10 and (want["exited"] != 0).sum() >= N // 10
    assert set(np.unique(want["gp_id"][want["exited"] == 0])) == {1 - w}
    _same(got, want, pkg.SEG_OUT.names)
    _same(coeff, wcoeff, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
    assert np.array_equal(comp.transmittance(rays), orc.transmittance(rays))


def test_march_inputs_hit_and_miss(pkg, ob):
    """the condition on the rays of tests/test_gpu_grid_mean.py's march: through the 24^3 two-sphere grid the composite alone gives at
    least a quarter hits and at least a quarter misses"""
    import test_gpu_grid_mean as gpu
    for ctx in ("none", "renewal"):
        params, g = gpu.march_case(pkg, ctx)
        comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=8)
        out = comp.sample_distance(smr.camera_rays(pkg, gpu.N_RAYS, gpu.RAY_SEED))
        hits = int((out["exited"] == 0).sum())
        print(ctx, "hits", hits, "misses", gpu.N_RAYS - hits)
        assert hits >= gpu.N_RAYS // 4 and gpu.N_RAYS - hits >= gpu.N_RAYS // 4
