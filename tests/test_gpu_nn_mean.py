"""GPU parity of the neural SDF mean (gpis_network_mean_*, gpis_bake_mean_network, csrc/gpis_nn_mean.hpp), BIT FOR BIT:

1. the evaluator at points against tests/nn_mean_ref.py (the C restatement of NeuralMean, pinned to the reference's Eigen by
   tests/test_nn_mean_cpu.py): value and gradient, networks A-F and Z, inside / on / outside the bounds, with and without a
   transform and offset / scale;
2. the bake: the returned voxels are float(restatement) on the lattice the header specifies, also across launch chunks;
3. a medium baked from network A against a second medium handed the restatement's voxels through gpis_set_mean_grid: the mean, the
   march in three contexts (every gpis_seg_out field, the coefficient records, n_eval / n_seg) and the four-bounce RGB frame, the
   latter also against the fixture the CPU composite recorded (tests/golden/nn_bake_small.npz);
4. the all-zero network baked with its constant against the ORACLE's homogeneous medium (nothing of ours in between);
5. a bake into slot 1 of a CSG pair, a second bake replacing the first, and the refusals.

No tolerance on any device result.  The library had none of these entries before the feature: every test here fails without it."""
import ctypes
import os

import numpy as np
import pytest

import grid_march_ref as gmr
import nn_mean_ref as nmr
import sdf_march_ref as smr
import test_gpu_grid_mean as tgg

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not nmr.available(), reason="no C compiler for the restatement")]

N_RAYS = tgg.N_RAYS
f32 = np.float32


@pytest.fixture(scope="module")
def ref():
    return nmr.NnMeanRef()


@pytest.fixture(scope="module")
def nets(pkg):
    return {n: pkg.load_network(nmr.network_path(n)) for n in nmr.NAMES}


def _same64(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint64).reshape(len(got), -1), np.ascontiguousarray(want).view(np.uint64).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:6], np.asarray(got)[bad[:3]], np.asarray(want)[bad[:3]])


def _same32(got, want, what):
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:6])


# ---- 1. the evaluator at points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", (False, True), ids=("plain", "transform+offset+scale"))
@pytest.mark.parametrize("name", nmr.NAMES)
def test_network_mean_value_and_gradient(pkg, ref, nets, name, placed):
    """2 051 points (not a multiple of 64: the last wave is partly idle) inside, on the faces, at the corners and outside the bounds
    on one, two and three axes"""
    net = nets[name]
    kw = dict(offset=0.3, scale=0.7, transform=nmr.demo_transform()) if placed else {}
    pts = nmr.demo_points(net)
    val, grad = pkg.network_mean(net, pts, **kw)
    wv, wg = ref.mean(net, pts, **kw)
    assert np.isfinite(wv).all() and np.isfinite(wg).all()
    _same64(val, wv, "value")
    _same64(grad, wg, "gradient")
    if name == "Z":
        assert np.array_equal(val, np.full(len(pts), (nmr.Z_CONSTANT + float(f32(0.3))) * float(f32(0.7)) if placed else nmr.Z_CONSTANT)) and not grad.any()
    else:
        assert np.unique(val).size > 500 and grad.any()
    only = pkg.network_mean(net, pts, want_grad=False, **kw)            # the value alone takes the kernel's other branch
    _same64(only, wv, "value alone")


# ---- 2. the bake ----------------------------------------------------------------------------------------------------------------
def _tab(pkg, **kw):
    return gmr.tabulated(pkg, pkg.params_for_config("C0"), **kw)


@pytest.mark.parametrize("name", nmr.NAMES)
def test_bake_on_the_small_odd_grid(pkg, ref, nets, name):
    """(9, 11, 13) voxels at origin (-4, -5, -6) under rotation x non-uniform scale x translation, NeuralMean's own transform, offset
    and scale on top: 1 287 voxels, the last wave partly idle"""
    T = gmr.world_to_index()
    kw = dict(offset=-0.1, scale=1.5, transform=nmr.demo_transform())
    m = pkg.Medium(_tab(pkg))
    vox = m.bake_mean_network(0, nets[name], gmr.DIMS, T, origin=gmr.ORIGIN, return_voxels=True, **kw)
    want = ref.bake(nets[name], gmr.DIMS, pkg.index_to_world(T), origin=gmr.ORIGIN, **kw)
    assert vox.shape == want.shape == (13, 11, 9)
    _same32(vox, want, name)
    # the installed grid is those voxels: the mean of the medium is the tabulated lookup over them
    pts = np.random.default_rng(9).uniform(-1.6, 1.6, (300, 3))
    g = gmr.grid(pkg, want, T, "linear", gmr.ORIGIN)
    _same64(m.mean(pts)[0], gmr.MeanRef(pkg, _tab(pkg), (g, None)).mean(pts)[0], "mean over the baked grid")
    m.close()


@pytest.mark.parametrize("name,n", (("A", 24), ("B", 24), ("F", 24), ("C", 32), ("A", 70)), ids=("A-24", "B-24", "F-24", "C-32-two-chunks", "A-70-two-chunks"))
def test_bake_on_the_rotated_cubes(pkg, ref, nets, name, n):
    """n^3 voxels of size 3 / n, not axis-aligned.  70^3 = 343 000 voxels pass the 2^18 points of one launch; the 150-wide network keeps
    its activations in a 64 MB workspace that bounds a launch to 27 904 points, which 32^3 passes"""
    T = gmr.sphere_world_to_index(n, 3.0 / n)
    m = pkg.Medium(_tab(pkg))
    vox = m.bake_mean_network(0, nets[name], (n, n, n), T, return_voxels=True)
    m.close()
    want = ref.bake(nets[name], (n, n, n), pkg.index_to_world(T))
    _same32(vox, want, (name, n))
    assert np.unique(want).size > n * n


# ---- 3. a baked medium is the medium handed the same voxels -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_voxels(pkg, ref):
    """network A on the 24^3 two-sphere lattice of tests/grid_march_ref.py, from the restatement; computed once, never changed"""
    v = nmr.bake_case_voxels(pkg, ref)
    v.setflags(write=False)
    return v


def _pair(pkg, nets, params, vox):
    """(baked, handed): one medium baked from network A, one handed the restatement's voxels through set_mean_grid"""
    T = gmr.sphere_world_to_index()
    baked, handed = pkg.Medium(params), pkg.Medium(params)
    got = baked.bake_mean_network(0, nets["A"], (24, 24, 24), T, return_voxels=True)
    _same32(got, vox, "bake")
    handed.set_mean_grid(0, vox, T, "linear")
    return baked, handed


def test_baked_medium_mean(pkg, nets, blob_voxels):
    baked, handed = _pair(pkg, nets, _tab(pkg, offset=0.05, scale=0.9), blob_voxels)
    pts = nmr.demo_points(nets["A"])
    (v, i, g), (wv, wi, wg) = baked.mean(pts), handed.mean(pts)
    _same64(v, wv, "value")
    _same64(g, wg, "gradient")
    assert np.array_equal(i, wi) and (v < 0).any() and (v > 0).any()
    baked.close()
    handed.close()


@pytest.mark.parametrize("ctx", ("none", "renewal", "renewal+"))
def test_baked_medium_march(pkg, nets, blob_voxels, ctx):
    """321 camera-like rays, first-scatter and continued segments: every gpis_seg_out field, the coefficient record with its per-ray
    evaluation count, the transmittance and n_eval / n_seg of each batch.  The condition on the case (at least 20 % hits and 20 %
    misses per batch) is asserted on the CPU composite when the fixtures are recorded, and on the device results here."""
    params, _ = tgg.march_case(pkg, ctx)
    baked, handed = _pair(pkg, nets, params, blob_voxels)
    rays = smr.camera_rays(pkg, N_RAYS, tgg.RAY_SEED)
    first = None
    for k in range(2):
        r = rays if k == 0 else tgg._continued(pkg, first, 6)
        handed.reset_counters()
        want, wc = handed.sample_distance(r, want_coeff=True)
        n_sd = handed.counters()
        handed.reset_counters()
        wvis = handed.transmittance(r)
        n_tr = handed.counters()
        first = first if k else want
        hits = int((want["exited"] == 0).sum())
        assert 5 * hits >= N_RAYS and 5 * (N_RAYS - hits) >= N_RAYS, (ctx, k, hits)
        baked.reset_counters()
        got, coeff = baked.sample_distance(r, want_coeff=True)
        assert baked.counters() == n_sd and n_sd[1] == N_RAYS
        tgg._same_records(got, want, pkg.SEG_OUT.names)
        tgg._same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
        baked.reset_counters()
        assert np.array_equal(baked.transmittance(r), wvis) and baked.counters() == n_tr
    baked.close()
    handed.close()


def test_baked_medium_frame(pkg, nets, blob_voxels):
    """the 24 x 20 x 3 four-bounce RGB frame: baked == handed == the CPU composite's fixture"""
    small = dict(np.load(os.path.join(nmr.GOLD, "nn_bake_small.npz")))
    params = np.frombuffer(small["medium"].tobytes(), dtype=pkg.PARAMS).reshape(())
    scene = np.frombuffer(small["scene"].tobytes(), dtype=pkg.SCENE_S).reshape(())
    assert int(params["mean"]["type"]) == pkg.MEAN_TYPE.TABULATED and (int(scene["width"]), int(scene["height"])) == (24, 20)
    baked, handed = _pair(pkg, nets, params, blob_voxels)
    img, segs = baked.render_scene_s_paths_rgb(scene, int(small["max_bounces"]), small["albedo"], want_segs=True)
    wimg, wsegs = handed.render_scene_s_paths_rgb(scene, int(small["max_bounces"]), small["albedo"], want_segs=True)
    baked.close()
    handed.close()
    assert img.shape[-1] == 3 and small["image"].any() and small["seg_count"].any()
    assert np.array_equal(segs, wsegs) and np.array_equal(segs, small["seg_count"]), np.argwhere(segs != small["seg_count"])[:8]
    _same32(img, wimg, "baked vs handed")
    _same32(img, small["image"], "baked vs fixture")


# ---- 4. the constant anchor -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("none", "renewal", "renewal+", "1d_mis"))
def test_zero_network_anchor_against_the_oracle(pkg, ob, nets, name):
    """the constant-grid anchor of tests/test_gpu_grid_mean.py with the grid BAKED: network Z is the constant 0.25 everywhere, so with
    the slot's offset 0.25 and scale 0.5 the medium is the ORACLE's homogeneous mean 0.25 with gradient exactly 0"""
    import test_sdf_march_cpu as cpu
    base = cpu.base(pkg, name)
    hom = np.array(base)
    hom["mean"]["type"], hom["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.25
    orc = ob.Oracle(hom, threads=8)
    m = pkg.Medium(gmr.tabulated(pkg, base, offset=0.25, scale=0.5))
    vox = m.bake_mean_network(0, nets["Z"], (8, 8, 8), gmr.sphere_world_to_index(8, 0.4), return_voxels=True)
    assert np.array_equal(vox, np.full((8, 8, 8), nmr.Z_CONSTANT, f32))
    rays = smr.camera_rays(pkg, N_RAYS, tgg.RAY_SEED)
    want = orc.sample_distance(rays)
    for r in (rays, cpu.continued_rays(pkg, want, 6)):
        orc.reset_counters()
        m.reset_counters()
        w, wc = orc.sample_distance(r, want_coeff=True)
        got, coeff = m.sample_distance(r, want_coeff=True)
        assert (w["exited"] == 0).sum() >= N_RAYS // 10 and (w["exited"] != 0).sum() >= N_RAYS // 10
        tgg._same_records(got, w, pkg.SEG_OUT.names)
        tgg._same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin"))
        assert m.counters()[1] == orc.counters()[1] == N_RAYS
        if name != "1d_mis":
            tgg._same_records(coeff, wc, ("n_evals",))
            assert m.counters()[0] == orc.counters()[0] == int(wc["n_evals"].sum())
        assert np.array_equal(m.transmittance(r), orc.transmittance(r))
    m.close()


# ---- 5. slots, replacement, refusals --------------------------------------------------------------------------------------------
def test_bake_into_slot_1_of_a_csg_pair(pkg, nets, blob_voxels):
    p = gmr.tabulated(pkg, pkg.params_for_config("C0"), slot="mean_additional")
    p["mean"]["type"], p["mean"]["radius"], p["mean"]["center"] = pkg.MEAN_TYPE.SPHERICAL, 0.5, (-0.6, 0.1, 0.2)
    T = gmr.sphere_world_to_index()
    m = pkg.Medium(p)
    got = m.bake_mean_network(1, nets["A"], (24, 24, 24), T, return_voxels=True)
    _same32(got, blob_voxels, "bake into slot 1")
    pts = np.random.default_rng(2).uniform(-1.3, 1.3, (1500, 3))
    v, i, g = m.mean(pts)
    m.close()
    wv, wi, wg = gmr.MeanRef(pkg, p, (None, gmr.grid(pkg, blob_voxels, T, "linear"))).mean(pts)
    assert np.array_equal(i, wi) and set(np.unique(i)) == {0, 1}
    _same64(v, wv, "value")
    _same64(g, wg, "gradient")


def test_second_bake_replaces_the_first(pkg, ref, nets):
    T1, T2 = gmr.world_to_index(), gmr.sphere_world_to_index()
    m = pkg.Medium(_tab(pkg))
    pts = np.random.default_rng(4).uniform(-1.3, 1.3, (400, 3))
    m.bake_mean_network(0, nets["B"], gmr.DIMS, T1, origin=gmr.ORIGIN)                       # no voxels returned: nothing leaves the device
    first = m.mean(pts)[0]
    m.bake_mean_network(0, nets["A"], (24, 24, 24), T2, interpolate="point")
    second, _, grad = m.mean(pts)
    m.close()
    g1 = gmr.grid(pkg, ref.bake(nets["B"], gmr.DIMS, pkg.index_to_world(T1), origin=gmr.ORIGIN), T1, "linear", gmr.ORIGIN)
    g2 = gmr.grid(pkg, nmr.bake_case_voxels(pkg, ref), T2, "point")
    w1 = gmr.MeanRef(pkg, _tab(pkg), (g1, None)).mean(pts)[0]
    w2, _, wg = gmr.MeanRef(pkg, _tab(pkg), (g2, None)).mean(pts)
    assert not np.array_equal(w1, w2)
    _same64(first, w1, "first bake")
    _same64(second, w2, "second bake")
    _same64(grad, wg, "gradient after the second bake")


def test_refusals(pkg, ref, nets):
    INVALID = -1
    L = pkg.load_library().lib
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    T = gmr.world_to_index()
    gd, _ = pkg.variance_grid_desc(np.zeros((13, 11, 9), f32), T, "linear", gmr.ORIGIN)
    i2w = pkg.index_to_world(T)
    a = nets["A"]
    w = np.concatenate([a.weights, np.zeros(4 * 257 + 258 * 257)])        # long enough for every descriptor below
    good = a.desc()
    pts = np.zeros((4, 3))
    val = np.zeros(4)

    def bad(**edit):
        d = np.array(good)
        for k, v in edit.items():
            if k == "dims":
                for idx, pair in v.items():
                    d["dims"][idx] = pair
            else:
                d[k] = v
        return d

    cases = {
        "3 of a point": bad(dims={0: (4, 32), 1: (32, 32)}),                         # dims[0].in != 3
        "takes 32 inputs but layer 0 gives 16": bad(dims={0: (3, 16)}),              # a break in the chain
        "last layer gives 2": bad(dims={2: (32, 2)}),
        "a width is 1 .. 256": bad(dims={0: (3, 257), 1: (257, 32)}),                # width 257
        "n_layers = 1": bad(n_layers=1),
        "n_layers = 17": bad(n_layers=17),
    }
    m = pkg.Medium(_tab(pkg))
    for msg, d in cases.items():
        assert L.gpis_network_mean_host(vp(d), vp(w), 4, vp(pts), vp(val), None) == INVALID and msg.encode() in L.gpis_last_error(), (msg, L.gpis_last_error())
        assert L.gpis_bake_mean_network(m.h, 0, vp(d), vp(w), vp(gd), vp(i2w), None) == INVALID and msg.encode() in L.gpis_last_error(), (msg, L.gpis_last_error())
    # width 256 is built
    wide = pkg.Network([(3, 256), (256, 1)], [-1] * 3, [1] * 3, np.random.default_rng(1).standard_normal(256 * 4 + 257))
    _same64(pkg.network_mean(wide, pts + 0.1, want_grad=False), ref.mean(wide, pts + 0.1, want_grad=False), "width 256")
    # slots: 1 without mean_additional, 2, null pointers, a bad grid descriptor
    assert L.gpis_bake_mean_network(m.h, 1, vp(good), vp(w), vp(gd), vp(i2w), None) == INVALID and b"tabulated" in L.gpis_last_error()
    assert L.gpis_bake_mean_network(m.h, 2, vp(good), vp(w), vp(gd), vp(i2w), None) == INVALID
    for args in ((None, vp(w), vp(gd), vp(i2w)), (vp(good), None, vp(gd), vp(i2w)), (vp(good), vp(w), None, vp(i2w)), (vp(good), vp(w), vp(gd), None)):
        assert L.gpis_bake_mean_network(m.h, 0, *args, None) == INVALID
    for field, value in (("interpolate", 2), ("dims", (9, 0, 13))):
        g2 = np.array(gd)
        g2[field] = value
        assert L.gpis_bake_mean_network(m.h, 0, vp(good), vp(w), vp(g2), vp(i2w), None) == INVALID, (field, value)
    # the refused calls changed nothing: the slot still has no grid (density 0)
    assert np.array_equal(m.mean(np.random.default_rng(5).uniform(-1, 1, (50, 3)))[0], np.zeros(50))
    m.close()
    sph = pkg.Medium(pkg.params_for_config("C0"))                                    # a spherical mean: not a tabulated slot
    assert L.gpis_bake_mean_network(sph.h, 0, vp(good), vp(w), vp(gd), vp(i2w), None) == INVALID and b"tabulated" in L.gpis_last_error()
    sph.close()
    with pytest.raises(ValueError, match="at most 16"):
        pkg.Network([(3, 2)] + [(2, 2)] * 15 + [(2, 1)], [-1] * 3, [1] * 3, np.zeros(8 + 15 * 6 + 3)).desc()
