"""GPU parity of the tabulated mean (GPIS_MEAN_TABULATED, gpis_set_mean_grid, csrc/gpis_grid_mean.hpp), BIT FOR BIT:

1. gpis_mean_* against tests/grid_mean_ref.py (the C restatement of TabulatedMean over a dense array);
2. the evaluators and 3. the march against the composite of tests/grid_march_ref.py (the oracle's noise + that mean), with the
   constant-grid anchor against the ORACLE's own homogeneous-mean medium (nothing of ours in between) and one medium that carries
   both grids;
4. the frame drivers against the composite's fixture (tests/golden/grid_mean_small.npz) and against themselves;
5. the refusals, and a second gpis_set_mean_grid replacing the first.

The grids are numpy formulas (tests/grid_march_ref.py).  No tolerance on any device result.  gpis_create rejected mean type 4 before
this feature: every test here fails without it."""
import ctypes
import math
import os

import numpy as np
import pytest

import grid_march_ref as gmr
import grid_mean_ref
import sdf_march_ref as smr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not grid_mean_ref.available(), reason="no C compiler for the restatement")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_RAYS = 321
RAY_SEED = 5
f32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.ndim else a.view(np.uint8)


def _same_records(got, want, fields):
    for f in fields:
        eq = (_bits(got[f]) == _bits(want[f])).all(axis=1)
        assert eq.all(), (f, int((~eq).sum()), np.nonzero(~eq)[0][:8], got[f][~eq][:3], want[f][~eq][:3])


def _medium(pkg, params, grids=(None, None), transforms=(None, None)):
    m = pkg.Medium(params)
    for w in range(2):
        if grids[w] is not None:
            gmr.set_grid(m, w, grids[w])
        if transforms[w] is not None:
            m.set_mean_transform(w, transforms[w])
    return m


def _check_mean(pkg, params, points, grids=(None, None), transforms=(None, None), want_ids=None):
    m = _medium(pkg, params, grids, transforms)
    val, gid, grad = m.mean(points)
    m.close()
    wv, wi, wg = gmr.MeanRef(pkg, params, grids, transforms).mean(points)
    assert np.array_equal(gid, wi)
    if want_ids is not None:
        assert set(np.unique(wi)) == set(want_ids)
    bad = np.nonzero(val.view(np.uint64) != wv.view(np.uint64))[0]
    assert bad.size == 0, (bad.size, points[bad[:4]], val[bad[:4]], wv[bad[:4]])
    bad = np.nonzero((grad.view(np.uint64) != wg.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, points[bad[:4]], grad[bad[:4]], wg[bad[:4]])
    return wv, wg


# ---- 1. the mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_bounds", (False, True), ids=("bounds=array", "bounds>array"))
@pytest.mark.parametrize("volume", (False, True), ids=("sdf", "volume"))
@pytest.mark.parametrize("interpolate", ("linear", "point"))
def test_mean_on_the_point_classes(pkg, interpolate, volume, wide_bounds):
    """the (9, 11, 13) grid at origin (-4, -5, -6) under rotation x non-uniform scale x translation, on the points of
    tests/test_grid_mean_cpu.py (which asserts that every class of them is non-empty): value and gradient"""
    g = gmr.demo_grid(pkg, interpolate, wide_bounds)
    pts = gmr.demo_points(g)
    params = gmr.tabulated(pkg, pkg.params_for_config("C0"), offset=0.3, scale=0.7, volume=volume)
    v, grad = _check_mean(pkg, params, pts, grids=(g, None))
    assert np.unique(v).size > 100 and grad.any()
    if volume:
        floor = (-math.log(0.0001) + np.float64(f32(0.3))) * np.float64(f32(0.7))
        assert (v == floor).any() and (v < floor).any()           # both sides of max(0.0001, res)


def test_mean_without_a_grid_is_the_background(pkg):
    pts = np.random.default_rng(1).uniform(-1.5, 1.5, (300, 3))
    v, g = _check_mean(pkg, gmr.tabulated(pkg, pkg.params_for_config("C0"), offset=0.5, scale=2.0), pts)
    assert np.array_equal(v, np.full(300, 1.0)) and not g.any()
    _check_mean(pkg, gmr.tabulated(pkg, pkg.params_for_config("C0"), offset=0.5, scale=2.0, volume=True), pts)


def test_mean_csg_pairs_in_both_orders(pkg):
    g = gmr.grid(pkg, gmr.sphere_voxels(), gmr.sphere_world_to_index(), "linear")
    pts = np.random.default_rng(2).uniform(-1.3, 1.3, (1500, 3))
    for partner in ("spherical", "plane"):
        for slot in ("mean", "mean_additional"):
            other = "mean_additional" if slot == "mean" else "mean"
            p = gmr.tabulated(pkg, pkg.params_for_config("C0"), slot=slot)
            p["has_mean_additional"] = 1
            if partner == "spherical":
                p[other]["type"] = pkg.MEAN_TYPE.SPHERICAL
                p[other]["radius"] = 0.5
                p[other]["center"] = (-0.6, 0.1, 0.2)
                T = None
            else:
                p = smr.procedural(pkg, p, "plane", offset=0.3, slot=other)
                T = smr.transform_demo()
            w = 0 if slot == "mean" else 1
            grids, tfs = [None, None], [None, None]
            grids[w], tfs[1 - w] = g, T
            _check_mean(pkg, p, pts, grids=tuple(grids), transforms=tuple(tfs), want_ids=(0, 1))


def test_mean_of_the_other_types_is_unchanged(pkg):
    """types 0-3 through the same out-of-line functions, as tests/sdf_mean_ref.py states them"""
    pts = np.random.default_rng(3).uniform(-1.3, 1.3, (600, 3))
    for typ in (pkg.MEAN_TYPE.HOMOGENEOUS, pkg.MEAN_TYPE.SPHERICAL, pkg.MEAN_TYPE.LINEAR):
        p = pkg.params_for_config("C0")
        p["mean"]["type"] = typ
        p["mean"]["offset"] = 0.125
        p["mean"]["center"] = (0.1, -0.2, 0.05)
        p["mean"]["dir"] = (0.3, 1.0, -0.2)
        p["mean"]["scale"] = 0.7
        p["mean"]["min"] = -0.3
        _check_mean(pkg, p, pts)
    _check_mean(pkg, smr.procedural(pkg, pkg.params_for_config("C0"), "knob", scale=0.5, offset=0.01, minimum=-0.05), pts,
                transforms=(smr.transform_demo(), None))


def test_second_grid_replaces_the_first(pkg):
    g1 = gmr.demo_grid(pkg, "linear")
    g2 = gmr.grid(pkg, gmr.sphere_voxels(), gmr.sphere_world_to_index(), "point")
    pts = np.random.default_rng(4).uniform(-1.3, 1.3, (400, 3))
    params = gmr.tabulated(pkg, pkg.params_for_config("C0"))
    m = pkg.Medium(params)
    m.set_mean_grid(0, gmr.demo_voxels(), gmr.world_to_index(), "linear", origin=gmr.ORIGIN)       # g1's arguments
    first = m.mean(pts)[0]
    m.set_mean_grid(0, gmr.sphere_voxels(), gmr.sphere_world_to_index(), interpolate="point")       # Medium.set_mean_grid: g2's arguments
    second, _, grad = m.mean(pts)
    m.close()
    w1 = gmr.MeanRef(pkg, params, (g1, None)).mean(pts)[0]
    w2, _, wg = gmr.MeanRef(pkg, params, (g2, None)).mean(pts)
    assert np.array_equal(first, w1) and np.array_equal(second, w2) and np.array_equal(grad, wg) and not np.array_equal(w1, w2)


# ---- 2. the evaluators ---------------------------------------------------------------------------------------------------------
def _sphere_grid(pkg, interpolate="linear"):
    """the 24^3 grid of the two united spheres, voxel 0.125, not axis-aligned"""
    return gmr.grid(pkg, gmr.sphere_voxels(), gmr.sphere_world_to_index(), interpolate)


@pytest.mark.parametrize("config", ("world", "iso-ray", "1d-xy"))
def test_evaluators_equal_the_composite(pkg, ob, config):
    base = pkg.params_for_config({"world": "C0", "iso-ray": "C1", "1d-xy": "C2"}[config])
    if config == "1d-xy":
        assert int(base["correlation_xy"]) != 0
    params = gmr.tabulated(pkg, base)
    g = _sphere_grid(pkg)
    comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=8)
    m = _medium(pkg, params, (g, None))
    assert int(m.derived()["fast_path"]) == 0
    q = smr.queries(pkg, 193, 17)
    val, gid = m.eval_value(q)
    wval, wgid = comp.eval_value(q)
    assert np.array_equal(gid, wgid) and np.array_equal(val.view(np.uint32), wval.view(np.uint32)), np.nonzero(val != wval)[0][:8]
    assert (val < 0).any() and (val > 0).any()
    grad = m.eval_gradient(q)
    assert np.array_equal(grad.view(np.uint32), comp.eval_gradient(q).view(np.uint32))
    rng = np.random.default_rng(3)
    tv = rng.normal(0, 0.05, len(q)).astype(f32)
    tg = rng.normal(0, 1, (len(q), 3)).astype(f32)
    co, wco = m.conditioning(q, tv, tg), comp.conditioning(q, tv, tg)
    _same_records(co, wco, ("value_scale", "gradient_scale", "ray_origin"))
    if int(m.derived()["activate_conditioning"]):
        assert co["value_scale"].any()
        q2 = np.array(q)
        q2["coeff"] = wco
        v2, w2 = m.eval_value(q2)[0], comp.eval_value(q2)[0]
        assert np.array_equal(v2.view(np.uint32), w2.view(np.uint32)) and (v2 != val).any()
        assert np.array_equal(m.eval_gradient(q2).view(np.uint32), comp.eval_gradient(q2).view(np.uint32))
    m.close()


def _both_grids_params(pkg):
    p = pkg.params_for_config("C3")
    p["impulse_density"] = 10
    p["grid_nonstationary"] = 1
    p["grid_offset"], p["grid_scale"] = 1.0, 0.5          # variance (sdf + 1) / 2: positive on the whole grid
    return gmr.tabulated(pkg, p, offset=0.05, scale=0.9)


def test_one_medium_with_both_grids(pkg, ob):
    """grid_nonstationary covariance and tabulated mean from the SAME array, two independent device copies: the composite's noise is
    the oracle's with set_variance_grid"""
    vox, T = gmr.sphere_voxels(), gmr.sphere_world_to_index()
    params = _both_grids_params(pkg)
    g = gmr.grid(pkg, vox, T, "linear")
    comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=8)
    comp.noise.set_variance_grid(vox, T, "linear")
    m = _medium(pkg, params, (g, None))
    q = smr.queries(pkg, 193, 19)
    plain, _ = m.eval_value(q)                            # the mean grid alone: the variance lookup still returns 1
    m.set_variance_grid(vox, T, "linear")
    val, gid = m.eval_value(q)
    wval, wgid = comp.eval_value(q)
    assert np.array_equal(gid, wgid) and np.array_equal(val.view(np.uint32), wval.view(np.uint32)), np.nonzero(val != wval)[0][:8]
    assert (val != plain).any()
    assert np.array_equal(m.eval_gradient(q).view(np.uint32), comp.eval_gradient(q).view(np.uint32))
    pts = q["p"].astype(np.float64)
    assert np.array_equal(m.mean(pts)[0], comp.mean(pts)[0])
    # replacing the variance grid leaves the mean grid alone
    m.set_variance_grid(np.full((8, 8, 8), 1.0, f32), gmr.sphere_world_to_index(8, 0.4))
    assert np.array_equal(m.mean(pts)[0], comp.mean(pts)[0])
    m.close()


# ---- 3. the march --------------------------------------------------------------------------------------------------------------
def march_case(pkg, ctx):
    """(params, grid) of the march tests: C0 with step_size 0.02 in the given context, the two-sphere grid as the mean"""
    p = pkg.params_for_config("C0")
    p["step_size"] = 0.02
    if ctx != "none":
        p["single_realization"] = 0
        p["correlation_context"] = pkg.CTX.RENEWAL if ctx == "renewal" else pkg.CTX.RENEWAL_PLUS
    return gmr.tabulated(pkg, p), _sphere_grid(pkg)


def _continued(pkg, first_out, seed):
    idx = np.nonzero((first_out["exited"] == 0) & (first_out["ok"] != 0))[0]
    pick = idx[np.arange(N_RAYS) % len(idx)]
    r = smr.camera_rays(pkg, N_RAYS, seed, first_scatter=False, state=(0.0, first_out["aniso"][pick], first_out["gp_id"][pick]))
    rng = np.random.default_rng(seed + 1)
    d = rng.normal(size=(N_RAYS, 3))
    r["pos"] = first_out["p"][pick]
    r["dir"] = d / np.linalg.norm(d, axis=1)[:, None]
    r["near_t"] = 0
    r["far_t"] = rng.uniform(0.2, 1.2, N_RAYS)
    r["info_t"] = first_out["sample_t"][pick]
    return r


@pytest.mark.parametrize("ctx", ("none", "renewal", "renewal+"))
def test_march_equals_the_composite(pkg, ob, ctx):
    """321 camera-like rays through the 24^3 grid inside the r = 1.5 bound, first-scatter and continued segments: every gpis_seg_out
    field, the coefficient record with its per-ray evaluation count, and n_eval / n_seg of each batch"""
    params, g = march_case(pkg, ctx)
    comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=8)
    rays = smr.camera_rays(pkg, N_RAYS, RAY_SEED)
    batches = []
    first = None
    for k in range(2):
        r = rays if k == 0 else _continued(pkg, first, 6)
        w, wc, trips = comp.sample_distance(r, want_coeff=True, want_trips=True)
        n_sd = comp.last_n_eval
        vis = comp.transmittance(r)
        batches.append((r, w, wc, vis, n_sd, comp.last_n_eval))
        first = first if k else w
        hits = int((w["exited"] == 0).sum())
        print(ctx, "hits %d, exits %d, !ok %d, trips > 1: %d, n_eval %d + %d" % (hits, N_RAYS - hits, (w["ok"] == 0).sum(), (trips > 1).sum(), n_sd, comp.last_n_eval))
        if k == 0:          # the condition on the inputs: the composite alone gives a quarter hits and a quarter misses
            assert hits >= N_RAYS // 4 and N_RAYS - hits >= N_RAYS // 4
        assert hits >= N_RAYS // 10 and N_RAYS - hits >= N_RAYS // 10
    m = _medium(pkg, params, (g, None))
    for r, w, wc, vis, n_sd, n_tr in batches:
        m.reset_counters()
        got, coeff = m.sample_distance(r, want_coeff=True)
        assert m.counters() == (n_sd, N_RAYS)
        _same_records(got, w, pkg.SEG_OUT.names)
        _same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
        m.reset_counters()
        assert np.array_equal(m.transmittance(r), vis)
        assert m.counters() == (n_tr, N_RAYS)
    m.close()


@pytest.mark.parametrize("name", ("none", "renewal", "renewal+", "1d_mis"))
def test_constant_grid_anchor_against_the_oracle(pkg, ob, name):
    """The CPU anchor of tests/test_grid_mean_cpu.py on the device: a constant grid of 0.25 with offset 0.25 and scale 0.5 is the
    homogeneous mean 0.25 with gradient exactly 0, so every gpis_seg_out field and coefficient equals the ORACLE's on that
    medium — no restatement of ours in between.  First-scatter and continued segments.  With 3D sampling the per-ray evaluation
    count (gpis_cond_coeff.n_evals) and the handle's n_eval counter equal the oracle's too; n_seg in every case."""
    import test_sdf_march_cpu as cpu
    base = cpu.base(pkg, name)
    hom = np.array(base)
    hom["mean"]["type"], hom["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.25
    orc = ob.Oracle(hom, threads=8)
    params = gmr.tabulated(pkg, base, offset=0.25, scale=0.5)
    g = gmr.grid(pkg, np.full((8, 8, 8), 0.25, f32), gmr.sphere_world_to_index(8, 0.4), "linear")
    m = _medium(pkg, params, (g, None))
    rays = smr.camera_rays(pkg, N_RAYS, RAY_SEED)
    want = orc.sample_distance(rays)
    for r in (rays, cpu.continued_rays(pkg, want, 6)):
        orc.reset_counters()
        m.reset_counters()
        w, wc = orc.sample_distance(r, want_coeff=True)
        got, coeff = m.sample_distance(r, want_coeff=True)
        assert (w["exited"] == 0).sum() >= N_RAYS // 10 and (w["exited"] != 0).sum() >= N_RAYS // 10
        _same_records(got, w, pkg.SEG_OUT.names)
        _same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin"))
        assert m.counters()[1] == orc.counters()[1] == N_RAYS
        if name != "1d_mis":
            _same_records(coeff, wc, ("n_evals",))
            assert m.counters()[0] == orc.counters()[0] == int(wc["n_evals"].sum())
        assert np.array_equal(m.transmittance(r), orc.transmittance(r))
    m.close()


# ---- 4. frames -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return dict(np.load(os.path.join(GOLD, "grid_mean_small.npz")))


def _frame_medium(pkg, small):
    params = np.frombuffer(small["medium"].tobytes(), dtype=pkg.PARAMS).reshape(())
    assert int(params["mean"]["type"]) == pkg.MEAN_TYPE.TABULATED and int(params["mean_emission"]["enabled"]) != 0
    m = pkg.Medium(params)
    m.set_mean_grid(0, gmr.sphere_voxels(), gmr.sphere_world_to_index(), "linear")          # the public Python entry
    return m


def test_paths_rgb_frame_equals_the_fixture_and_emits_nothing(pkg, small):
    m = _frame_medium(pkg, small)
    scene = np.frombuffer(small["scene"].tobytes(), dtype=pkg.SCENE_S).reshape(())
    pts = np.random.default_rng(8).uniform(-1, 1, (64, 3))
    col, emi = m.mean_color_emission(pts)
    assert not emi.any() and np.unique(col).size > 8            # the emission field is set, and a tabulated primary mean emits 0
    img, segs = m.render_scene_s_paths_rgb(scene, int(small["max_bounces"]), small["albedo"], want_segs=True)
    assert small["image"].any() and small["seg_count"].any()
    assert np.array_equal(segs, small["seg_count"]), np.argwhere(segs != small["seg_count"])[:8]
    assert np.array_equal(img.view(np.uint32), small["image"].view(np.uint32)), np.argwhere(img != small["image"])[:8]
    m.close()


def _lambert(pkg, m, scene):
    """one call of gpis_render_scene_s into zeroed device buffers: (radiance_sum, hit_count)"""
    import torch
    scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    h, w = int(scene["height"]), int(scene["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.call("gpis_render_scene_s", scene, d_rad.data_ptr(), d_hit.data_ptr(), None)
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w), d_hit.cpu().numpy().view(np.uint32).reshape(h, w)


def test_lambert_frame_is_the_sum_of_its_row_ranges(pkg, small):
    m = _frame_medium(pkg, small)
    scene = np.frombuffer(small["scene"].tobytes(), dtype=pkg.SCENE_S).reshape(())
    img, hits = _lambert(pkg, m, scene)
    assert hits.any() and img.any()
    h = int(scene["height"])
    acc, acc_hits = np.zeros_like(img), np.zeros_like(hits)
    for r0, r1 in ((0, 7), (7, 8), (8, h)):
        s = np.array(scene)
        s["y_begin"], s["y_count"] = r0, r1 - r0
        a, b = _lambert(pkg, m, s)
        acc += a
        acc_hits += b
    assert np.array_equal(acc.view(np.uint32), img.view(np.uint32)) and np.array_equal(acc_hits, hits)
    m.close()


def test_adaptive_frame_equals_its_composite(pkg, ob, small):
    """gpis_render_scene_s_adaptive (22 x 14, 48 spp: one uniform pass and two planned ones) against the composite of
    tests/adaptive_ref.py built from per-sample gpis_render_scene_s calls on the same handle, bit for bit"""
    import test_gpu_adaptive as tga
    m = _frame_medium(pkg, small)
    scene = tga._scene(ob)
    want = tga._composite(pkg, m, scene)
    counts = want["counts"]
    assert len(counts) == 3 and (counts[0] == 16).all() and counts[1].max() > 16 and want["hit_count"].any()
    tga._equal(tga._adaptive(pkg, m, scene), want)
    m.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    params = gmr.tabulated(pkg, pkg.params_for_config("C0"))
    g = gmr.demo_grid(pkg, "linear")
    m = _medium(pkg, params, (g, None))
    L = m.L.lib
    UNSUPPORTED, INVALID = -2, -1
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.gpis_build_guide(m.h, 16, 8) == UNSUPPORTED and b"tabulated" in L.gpis_last_error()
    assert L.gpis_fs_sample_distance_batch(m.h, 0, None, None, None, None) == UNSUPPORTED and b"tabulated" in L.gpis_last_error()
    d = np.array(g.desc)
    assert L.gpis_set_mean_grid(m.h, 1, vp(d), vp(g.voxels)) == INVALID and b"tabulated" in L.gpis_last_error()     # no mean_additional
    assert L.gpis_set_mean_grid(m.h, 2, vp(d), vp(g.voxels)) == INVALID
    assert L.gpis_set_mean_grid(m.h, 0, None, vp(g.voxels)) == INVALID and L.gpis_set_mean_grid(m.h, 0, vp(d), None) == INVALID
    for field, value in (("interpolate", 2), ("interpolate", -1), ("dims", (9, 0, 13)), ("dims", (-1, 11, 13))):
        bad = np.array(d)
        bad[field] = value
        assert L.gpis_set_mean_grid(m.h, 0, vp(bad), vp(g.voxels)) == INVALID, (field, value)
    pts = np.random.default_rng(5).uniform(-1, 1, (50, 3))
    assert np.array_equal(m.mean(pts)[0], gmr.MeanRef(pkg, params, (g, None)).mean(pts)[0])          # the refused calls changed nothing
    m.close()
    sph = pkg.Medium(pkg.params_for_config("C0"))
    assert sph.L.lib.gpis_set_mean_grid(sph.h, 0, vp(d), vp(g.voxels)) == INVALID and b"tabulated" in L.gpis_last_error()
    sph.close()
    bad = np.array(params)
    bad["mean"]["type"] = 5
    with pytest.raises(RuntimeError, match="mean type"):
        pkg.Medium(bad)
    with pytest.raises(RuntimeError, match="tabulated"):
        pkg.WeightSpaceMedium(params)
