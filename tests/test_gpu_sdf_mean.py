"""GPU parity of the procedural SDF mean (GPIS_MEAN_PROCEDURAL, csrc/gpis_sdf.hpp), BIT FOR BIT:

1. gpis_mean_* against tests/sdf_mean_ref.py (the C restatement pinned to the reference's compiled SDF functions);
2. the evaluators and 3. the march against the composite of tests/sdf_march_ref.py (the oracle's noise + that mean), with the plane
   anchor against the oracle's own linear-mean medium;
4. the frame drivers against the composite's fixture (tests/golden/sdf_mean_small.npz) and against themselves;
5. the refusals.

No tolerance on any device result.  gpis_create rejected mean type 3 before this feature: every test here fails without it."""
import ctypes
import os

import numpy as np
import pytest

import sdf_march_ref as smr
import sdf_mean_ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sdf_mean_ref.available(), reason="no C compiler for the restatement")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUNCS = sdf_mean_ref.FUNCS
N_RAYS = 321


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.ndim else a.view(np.uint8)


def _same_records(got, want, fields):
    for f in fields:
        eq = (_bits(got[f]) == _bits(want[f])).all(axis=1)
        assert eq.all(), (f, int((~eq).sum()), np.nonzero(~eq)[0][:8], got[f][~eq][:3], want[f][~eq][:3])


@pytest.fixture(scope="module")
def mref():
    return sdf_mean_ref.SdfMeanRef()


@pytest.fixture(scope="module")
def points():
    """the pin points as doubles plus 257 random doubles that are not float-exact"""
    pins = np.load(os.path.join(GOLD, "sdf_mean_pins.npz"))["points"].astype(np.float64)
    extra = np.random.default_rng(41).uniform(-1.3, 1.3, (257, 3))
    assert (extra.astype(np.float32).astype(np.float64) != extra).any(axis=1).all()
    return np.concatenate([pins, extra])


def _check_mean(pkg, mref, params, points, transforms=(None, None), want_ids=None):
    m = pkg.Medium(params)
    for w, T in enumerate(transforms):
        if T is not None:
            m.set_mean_transform(w, T)
    val, gid, grad = m.mean(points)
    m.close()
    wv, wi, wg = mref.mean(params, points, transforms)
    assert np.array_equal(gid, wi)
    if want_ids is not None:
        assert set(np.unique(wi)) == set(want_ids)
    bad = np.nonzero(val.view(np.uint64) != wv.view(np.uint64))[0]
    assert bad.size == 0, (bad.size, points[bad[:4]], val[bad[:4]], wv[bad[:4]])
    bad = np.nonzero((grad.view(np.uint64) != wg.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, points[bad[:4]], grad[bad[:4]], wg[bad[:4]])
    return wv


# ---- 1. the mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("func", FUNCS)
def test_mean_of_every_function(pkg, mref, points, func):
    _check_mean(pkg, mref, smr.procedural(pkg, pkg.params_for_config("C0"), func), points)


def test_mean_scale_offset_min_clipping(pkg, mref, points):
    p = smr.procedural(pkg, pkg.params_for_config("C0"), "knob", scale=0.5, offset=0.01, minimum=-0.05)
    v = _check_mean(pkg, mref, p, points)
    assert (v == np.float64(np.float32(-0.05))).any() and (v > 0).any()


def test_mean_with_transform(pkg, mref, points):
    T = smr.transform_demo()
    p = smr.procedural(pkg, pkg.params_for_config("C0"), "knob_outer")
    plain = mref.mean(p, points)[0]
    v = _check_mean(pkg, mref, p, points, transforms=(T, None))
    assert (v != plain).mean() > 0.9
    # a singular transform inverts to the identity (Mat4f::invert, det == 0)
    S = np.array(T)
    S[:, 0] = 0
    assert np.array_equal(_check_mean(pkg, mref, p, points[:300], transforms=(S, None)), plain[:300])


def test_mean_csg_pairs_in_both_orders(pkg, mref, points):
    # knob first, a sphere of radius 0.5 about (0.7, 0, 0) second
    p = smr.procedural(pkg, pkg.params_for_config("C0"), "knob")
    p["has_mean_additional"] = 1
    p["mean_additional"]["type"] = pkg.MEAN_TYPE.SPHERICAL
    p["mean_additional"]["radius"] = 0.5
    p["mean_additional"]["center"] = (0.7, 0.0, 0.0)
    _check_mean(pkg, mref, p, points, want_ids=(0, 1))
    # the unit sphere first, two_spheres second (with a transform on the second slot)
    q = smr.procedural(pkg, pkg.params_for_config("C0"), "two_spheres", slot="mean_additional")
    _check_mean(pkg, mref, q, points, transforms=(None, smr.transform_demo()), want_ids=(0, 1))


def test_mean_of_the_analytic_types(pkg, mref, points):
    """types 0-2 through the new entry: the analytic means as the C restatement states them (tests/test_sdf_march_cpu.py shows that
    statement reproducing the oracle's march on a linear mean bit for bit)"""
    for typ in (pkg.MEAN_TYPE.HOMOGENEOUS, pkg.MEAN_TYPE.SPHERICAL, pkg.MEAN_TYPE.LINEAR):
        p = pkg.params_for_config("C0")
        p["mean"]["type"] = typ
        p["mean"]["offset"] = 0.125
        p["mean"]["center"] = (0.1, -0.2, 0.05)
        p["mean"]["dir"] = (0.3, 1.0, -0.2)
        p["mean"]["scale"] = 0.7
        p["mean"]["min"] = -0.3
        _check_mean(pkg, mref, p, points[-600:])


# ---- 2. the evaluators ---------------------------------------------------------------------------------------------------------
def _config(pkg, name):
    if name == "world":
        p = pkg.params_for_config("C0")
    elif name == "iso-ray":
        p = pkg.params_for_config("C1")
    elif name == "1d-xy":
        p = pkg.params_for_config("C2")
    elif name == "matern":
        p = pkg.params_for_config("C0")
        p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL
        p["kernel_type"], p["matern_v"] = 1, 2.5
    elif name == "multires":
        p = pkg.params_for_config("C3")
    return p


@pytest.mark.parametrize("func", ("knob", "knob_outer"))
@pytest.mark.parametrize("config", ("world", "iso-ray", "1d-xy", "matern", "multires"))
def test_evaluators_equal_the_composite(pkg, ob, config, func):
    params = smr.procedural(pkg, _config(pkg, config), func)
    comp = smr.SdfComposite(pkg, ob, params, threads=8)
    m = pkg.Medium(params)
    assert int(m.derived()["fast_path"]) == 0
    q = smr.queries(pkg, 193, 17)
    val, gid = m.eval_value(q)
    wval, wgid = comp.eval_value(q)
    assert np.array_equal(gid, wgid) and np.array_equal(val.view(np.uint32), wval.view(np.uint32)), np.nonzero(val != wval)[0][:8]
    assert (val < 0).any() and (val > 0).any()
    grad = m.eval_gradient(q)
    assert np.array_equal(grad.view(np.uint32), comp.eval_gradient(q).view(np.uint32))
    rng = np.random.default_rng(3)
    tv = rng.normal(0, 0.05, len(q)).astype(np.float32)
    tg = rng.normal(0, 1, (len(q), 3)).astype(np.float32)
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


# ---- 3. the march --------------------------------------------------------------------------------------------------------------
def _march_params(pkg, ctx):
    p = pkg.params_for_config("C0")
    p["step_size"] = 0.02
    if ctx != "none":
        p["single_realization"] = 0
        p["correlation_context"] = pkg.CTX.RENEWAL if ctx == "renewal" else pkg.CTX.RENEWAL_PLUS
    return p


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
    """321 camera-like rays through the knob inside the r = 1.5 bound (step_size 0.02: at most 150 steps), first-scatter and
    continued segments: every gpis_seg_out field, the coefficient record with its per-ray evaluation count, and n_eval / n_seg of
    each batch, which the composite counts as the device does (intersectGP's values, the refinement trips, the exit evaluation,
    the conditioning's evaluations and re-evaluations, the gradient)"""
    params = smr.procedural(pkg, _march_params(pkg, ctx), "knob")
    comp = smr.SdfComposite(pkg, ob, params, threads=8)
    rays = smr.camera_rays(pkg, N_RAYS, 5)
    batches = []
    first = None
    for k in range(2):
        r = rays if k == 0 else _continued(pkg, first, 6)
        w, wc, trips = comp.sample_distance(r, want_coeff=True, want_trips=True)
        n_sd = comp.last_n_eval
        vis = comp.transmittance(r)
        batches.append((r, w, wc, vis, n_sd, comp.last_n_eval))
        first = first if k else w
        print(ctx, "hits %d, exits %d, !ok %d, trips > 1: %d, n_eval %d + %d" % ((w["exited"] == 0).sum(), (w["exited"] != 0).sum(), (w["ok"] == 0).sum(),
                                                                                   (trips > 1).sum(), n_sd, comp.last_n_eval))
        assert (w["exited"] == 0).sum() >= N_RAYS // 10 and (w["exited"] != 0).sum() >= N_RAYS // 10 and (trips > 1).any()
    m = pkg.Medium(params)
    for r, w, wc, vis, n_sd, n_tr in batches:
        m.reset_counters()
        got, coeff = m.sample_distance(r, want_coeff=True)
        assert m.counters() == (n_sd, N_RAYS)
        _same_records(got, w, pkg.SEG_OUT.names)
        _same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
        m.reset_counters()
        assert np.array_equal(m.transmittance(r), vis)
        assert m.counters() == (n_tr, N_RAYS)
    # GPIS_OPT_PERSISTENT is inert for such a medium (it is served by the lane-per-ray all-features instance either way): checked once
    m.set_option("persistent", 0)
    got0 = m.sample_distance(rays)
    _same_records(got0, batches[0][1], pkg.SEG_OUT.names)
    m.close()


@pytest.mark.parametrize("name", ("none", "renewal", "renewal+", "1d_mis"))
def test_plane_anchor_against_the_oracle(pkg, ob, name):
    """The CPU anchor of tests/test_sdf_march_cpu.py on the device, same media and rays.  func = plane, scale 1, offset 0 has the
    value of LinearMean(ref 0, dir (0, 1, 0)): the fields that do not depend on the mean's gradient equal the ORACLE's on that
    medium, with nothing of the composite in between — first-scatter segments in every case, continued ones where the conditioning
    takes the value alone (none, Renewal).  Renewal+ and the 1D scheme condition a continued segment on the gradient, which here is
    the one-sided difference and not (0, 1, 0): those continued segments cannot equal the linear medium's, on the device as on
    the CPU, and are compared with the composite instead, in every field."""
    import test_sdf_march_cpu as cpu
    base = cpu.base(pkg, name)
    orc = ob.Oracle(cpu.linear(pkg, base), threads=8)
    rays = smr.camera_rays(pkg, N_RAYS, 5)
    want = orc.sample_distance(rays)
    rays2 = cpu.continued_rays(pkg, want, 6)
    params = smr.procedural(pkg, base, "plane")
    m = pkg.Medium(params)
    value_fields = tuple(f for f in pkg.SEG_OUT.names if f not in cpu.GRADIENT_FIELDS)
    for k, r in enumerate((rays, rays2)):
        got, coeff = m.sample_distance(r, want_coeff=True)
        if k == 1 and name in ("renewal+", "1d_mis"):
            comp = smr.SdfComposite(pkg, ob, params, threads=8)
            w, wc = comp.sample_distance(r, want_coeff=True)
            _same_records(got, w, pkg.SEG_OUT.names)
            _same_records(coeff, wc, ("value_scale", "gradient_scale", "ray_origin"))
            assert np.array_equal(m.transmittance(r), comp.transmittance(r))
            continue
        w = want if k == 0 else orc.sample_distance(r)
        assert (w["exited"] == 0).sum() >= N_RAYS // 4 and (w["exited"] != 0).sum() >= N_RAYS // 10
        _same_records(got, w, value_fields)
        agree = got["ok"] == w["ok"]
        assert agree.mean() > 0.97
        _same_records(got[agree], w[agree], tuple(f for f in cpu.GRADIENT_FIELDS if f != "aniso"))
        assert np.array_equal(m.transmittance(r), orc.transmittance(r))
    m.close()


# ---- 4. frames -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return dict(np.load(os.path.join(GOLD, "sdf_mean_small.npz")))


def _frame_medium(pkg, small):
    params = np.frombuffer(small["params"].tobytes(), dtype=pkg.PARAMS).reshape(())
    m = pkg.Medium(params)
    m.set_mean_transform(0, small["transform"])
    return m


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


def test_paths_rgb_frame_equals_the_fixture(pkg, small):
    m = _frame_medium(pkg, small)
    scene = np.frombuffer(small["scene"].tobytes(), dtype=pkg.SCENE_S).reshape(())
    img, segs = m.render_scene_s_paths_rgb(scene, int(small["max_bounces"]), small["albedo"], want_segs=True)
    assert small["image"].any() and small["seg_count"].any()
    assert np.array_equal(segs, small["seg_count"]), np.argwhere(segs != small["seg_count"])[:8]
    assert np.array_equal(img.view(np.uint32), small["image"].view(np.uint32)), np.argwhere(img != small["image"])[:8]
    m.close()


def test_lambert_frame_is_self_consistent(pkg, small):
    """gpis_render_scene_s on the same medium: hits, whole frame == sum of its row ranges"""
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
    """gpis_render_scene_s_adaptive on the knob medium with the transform, at the smallest settings the entry takes for a real
    schedule (spp_step = threshold = 16, the 22 x 14 frame of tests/adaptive_ref.py at 48 spp: one uniform pass and two planned
    ones): image, sample counts, hit counts, records and info equal the composite of tests/adaptive_ref.py built from per-sample
    gpis_render_scene_s calls on the same handle, bit for bit"""
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
    params = smr.procedural(pkg, pkg.params_for_config("C0"), "knob")
    m = pkg.Medium(params)
    L = m.L.lib
    UNSUPPORTED, INVALID = -2, -1
    assert L.gpis_build_guide(m.h, 16, 8) == UNSUPPORTED and b"procedural" in L.gpis_last_error()
    assert L.gpis_fs_sample_distance_batch(m.h, 0, None, None, None, None) == UNSUPPORTED and b"procedural" in L.gpis_last_error()
    rays = np.zeros(1, dtype=pkg.RAY_IN)
    states = np.zeros(1, dtype=pkg.FS_STATE)
    out = np.zeros(1, dtype=pkg.SEG_OUT)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.gpis_fs_sample_distance_host(m.h, 1, vp(rays), vp(states), vp(out)) == UNSUPPORTED and b"procedural" in L.gpis_last_error()
    assert L.gpis_set_mean_transform(m.h, 1, vp(np.eye(4, dtype=np.float32))) == INVALID and b"procedural" in L.gpis_last_error()
    assert L.gpis_set_mean_transform(m.h, 2, vp(np.eye(4, dtype=np.float32))) == INVALID
    m.close()
    sph = pkg.Medium(pkg.params_for_config("C0"))
    assert sph.L.lib.gpis_set_mean_transform(sph.h, 0, vp(np.eye(4, dtype=np.float32))) == INVALID and b"procedural" in L.gpis_last_error()
    sph.close()
    bad = np.array(params)
    bad["mean"]["func"] = 5
    with pytest.raises(RuntimeError, match="sdf function"):
        pkg.Medium(bad)
    with pytest.raises(RuntimeError, match="procedural"):
        pkg.WeightSpaceMedium(params)
