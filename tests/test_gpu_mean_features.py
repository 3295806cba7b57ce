"""GPU parity of what DevModel::sdf_mean serves beyond the C0 march of one procedural / tabulated mean, BIT FOR BIT:

1. CSG pairs with an out-of-line mean in either slot: evaluators, conditioning, and the C0 march with first-scatter and continued
   segments (path_mean_grad picks the slot from the id path_mean_weight_space returned; gp_id travels through gpis_seg_out);
2. the colour point: gpis_mean_color_emission_* on a procedural mean under a transform (sdf::color_point evaluates the colour at
   T^-1 p) with a ramp and a sandstone colour, and the march's hit weight with the colour on;
3. the knob march outside C0: iso-ray (C1), 1D (C2), Matern 5/2;
4. constant-mean anchors for what the composite cannot express — absorption-only, the variance field, the aniso field,
   use_aniso_mtx, sandstone colour, surf_vol_phase_separate — with a constant tabulated grid and a fully clipped plane as the mean:
   against the device's own homogeneous medium bit for bit, and against the oracle as the parity test of the feature compares.

The references of 1-3 are the composites of tests/mean_features_ref.py (tests/test_mean_features_cpu.py asserts their input
conditions, tests/test_sdf_march_cpu.py pins the composite to the oracle).  No tolerance on any device result."""
import numpy as np
import pytest

import grid_march_ref as gmr
import mean_features_ref as mfr
import sdf_march_ref as smr
import sdf_mean_ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sdf_mean_ref.available(), reason="no C compiler for the restatement")]

N_RAYS = mfr.N_RAYS
f32 = np.float32
COEFF = ("value_scale", "gradient_scale", "ray_origin")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.ndim else a.view(np.uint8)


def _same_records(got, want, fields):
    for f in fields:
        eq = (_bits(got[f]) == _bits(want[f])).all(axis=1)
        assert eq.all(), (f, int((~eq).sum()), np.nonzero(~eq)[0][:8], got[f][~eq][:3], want[f][~eq][:3])


def _same_arrays(got, want, what):
    eq = (_bits(got) == _bits(want)).all(axis=1) if np.ndim(got) else _bits(got) == _bits(want)
    assert eq.all(), (what, int((~eq).sum()), np.nonzero(~eq)[0][:8], got[~eq][:3], want[~eq][:3])


def _medium(pkg, medium):
    params, grids, transforms = medium
    m = pkg.Medium(params)
    for w in range(2):
        if grids[w] is not None:
            gmr.set_grid(m, w, grids[w])
        if transforms[w] is not None:
            m.set_mean_transform(w, transforms[w])
    return m


def _check_evaluators(pkg, m, comp, seed=17):
    """eval_value / eval_gradient / conditioning on 193 queries, and the evaluators again under the conditioning's coefficients"""
    q = smr.queries(pkg, mfr.N_QUERIES, seed)
    val, gid = m.eval_value(q)
    wval, wgid = comp.eval_value(q)
    assert np.array_equal(gid, wgid)
    _same_arrays(val, wval, "value")
    _same_arrays(m.eval_gradient(q), comp.eval_gradient(q), "gradient")
    rng = np.random.default_rng(3)
    tv = rng.normal(0, 0.05, len(q)).astype(f32)
    tg = rng.normal(0, 1, (len(q), 3)).astype(f32)
    co, wco = m.conditioning(q, tv, tg), comp.conditioning(q, tv, tg)
    _same_records(co, wco, COEFF)
    if int(m.derived()["activate_conditioning"]):
        assert co["value_scale"].any()
        q2 = np.array(q)
        q2["coeff"] = wco
        _same_arrays(m.eval_value(q2)[0], comp.eval_value(q2)[0], "conditioned value")
        _same_arrays(m.eval_gradient(q2), comp.eval_gradient(q2), "conditioned gradient")
    return wgid


def _check_march(pkg, m, batches, count_evals=True):
    for b in batches:
        m.reset_counters()
        got, coeff = m.sample_distance(b["rays"], want_coeff=True)
        n_eval, n_seg = m.counters()
        assert n_seg == N_RAYS
        _same_records(got, b["out"], pkg.SEG_OUT.names)
        _same_records(coeff, b["coeff"], COEFF)
        if count_evals:
            _same_records(coeff, b["coeff"], ("n_evals",))
            assert n_eval == b["n_sd"]
        m.reset_counters()
        assert np.array_equal(m.transmittance(b["rays"]), b["vis"])
        n_eval, n_seg = m.counters()
        assert n_seg == N_RAYS and (not count_evals or n_eval == b["n_tr"])


# ---- 1. CSG --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ("none", "renewal", "renewal+"))
@pytest.mark.parametrize("pair", ("knob+sphere", "grid+plane"))
def test_csg_pair_equals_the_composite(pkg, ob, pair, ctx):
    medium = mfr.csg_pair(pkg, mfr.march_base(pkg, ctx), pair)
    comp, batches = mfr.march_reference(pkg, ob, (pair, ctx), medium)
    for k, b in enumerate(batches):
        s = mfr.summary(b)
        assert min(s["hit_ids"]) >= 16 and s["exits"] >= N_RAYS // 10 and (k == 0 or min(s["last_ids"]) >= 16)
    m = _medium(pkg, medium)
    assert int(m.derived()["fast_path"]) == 0
    ids = _check_evaluators(pkg, m, comp)
    assert set(np.unique(ids)) == {0, 1}
    _check_march(pkg, m, batches)
    m.close()


# ---- 2. the colour point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ramp", "sandstone"))
def test_colour_of_a_transformed_procedural_mean(pkg, ob, kind):
    medium = mfr.colour(pkg, mfr.march_base(pkg, "none"), kind)
    comp, batches = mfr.march_reference(pkg, ob, ("colour", kind), medium)
    m = _medium(pkg, medium)
    pts = np.concatenate([np.random.default_rng(8).uniform(-1, 1, (1025, 3)), np.zeros((1, 3))])      # inside the ramp's [-1, 1]
    col, emi = m.mean_color_emission(pts)
    wcol, wemi = comp.mean_color_emission(pts)
    plain, _ = comp.noise.mean_color_emission(pts)
    assert (wcol != plain).any(axis=1).mean() > 0.9            # the colour at T^-1 p is not the colour at p
    _same_arrays(col, wcol, "colour")
    _same_arrays(emi, wemi, "emission")
    w = batches[0]["out"]
    h = (w["exited"] == 0) & (w["ok"] != 0)
    assert h.sum() >= N_RAYS // 10 and len(np.unique(w["weight"][h], axis=0)) >= h.sum() // 2
    _check_march(pkg, m, batches)
    m.close()


# ---- 3. the march outside C0 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("iso-ray", "1d-xy", "matern"))
def test_knob_march_on_the_other_configs(pkg, ob, name):
    """every gpis_seg_out field and coefficient of first-scatter and continued segments; the evaluation counts where the composite
    counts them (3D sampling); n_seg always.  The Matern batch holds segments that fail on a non-finite gradient."""
    medium = (smr.procedural(pkg, mfr.config(pkg, name), "knob"), (None, None), (None, None))
    comp, batches = mfr.march_reference(pkg, ob, ("config", name), medium)
    for b in batches:
        s = mfr.summary(b)
        assert s["hits"] >= N_RAYS // 10 and s["exits"] >= N_RAYS // 10 and s["trips_gt_1"] >= 1
    m = _medium(pkg, medium)
    assert int(m.derived()["fast_path"]) == 0
    _check_march(pkg, m, batches, count_evals=name != "1d-xy")
    m.close()


# ---- 4. constant-mean anchors ----------------------------------------------------------------------------------------------------------
MEAN = 0.25


def _constant_mean(pkg, base, kind):
    """the homogeneous mean 0.25 with gradient exactly 0, said three ways: (params, grids)"""
    if kind == "homogeneous":
        p = np.array(base)
        p["mean"]["type"], p["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, MEAN
        return p, (None, None)
    if kind == "grid":           # the constant grid of test_constant_grid_anchor_against_the_oracle: (0.25 + 0.25) * 0.5
        g = gmr.grid(pkg, np.full((8, 8, 8), 0.25, f32), gmr.sphere_world_to_index(8, 0.4), "linear")
        return gmr.tabulated(pkg, base, offset=0.25, scale=0.5), (g, None)
    # plane with `min` above every value: max(0.25, 0.01 y - 10) = 0.25 at p and at the three points of the one-sided difference
    return smr.procedural(pkg, base, "plane", scale=0.01, offset=-10.0, minimum=MEAN), (None, None)


def _absorption(pkg, cfg):
    p = pkg.params_for_config("C0" if cfg == "C0_perpath" else cfg)
    if cfg == "C0_perpath":
        p["single_realization"] = 0
        p["correlation_context"] = pkg.CTX.RENEWAL_PLUS
    p["sigma_s"] = 0.0
    p["sigma_a"] = (0.5, 1.0, 2.0)
    return p


def _variance(pkg, multires):
    p = pkg.params_for_config("C3")
    p["impulse_density"] = 12
    p["multi_resolution_grid"] = multires
    p["isotropic_3d_sampling"] = multires
    p["correlation_context"] = pkg.CTX.RENEWAL
    p["ls_ramp_type"] = 3
    p["ls_min"], p["ls_max"], p["ls_start"], p["ls_end"] = 0.6, 1.4, -1.2, 1.2
    p["ls_min2"], p["ls_max2"], p["ls_start2"], p["ls_end2"] = 0.8, 1.5, -1.0, 1.0
    for key, typ, lo, hi in (("var", 0, 0.4, 1.8), ("mean_color", 1, 0.2, 0.9), ("mean_emission", 3, 0.1, 2.0)):
        p[key]["enabled"], p[key]["type"] = 1, typ
        p[key]["min"], p[key]["max"], p[key]["start"], p[key]["end"] = lo, hi, -1.0, 1.0
        p[key]["min2"], p[key]["max2"], p[key]["start2"], p[key]["end2"] = 0.5, 1.5, -0.5, 0.5
    return p


def _aniso_field(pkg, iso, multires, ctx):
    p = pkg.params_for_config("C3")
    p["impulse_density"] = 12
    p["isotropic_3d_sampling"] = iso
    p["multi_resolution_grid"] = multires
    p["correlation_context"] = getattr(pkg.CTX, ctx)
    p["aniso"] = (1.0, 0.8, 1.25)
    p["aniso_field"]["enabled"], p["aniso_field"]["type"] = 1, 0
    p["aniso_field"]["min"], p["aniso_field"]["max"] = 0.1, 0.9
    p["aniso_field"]["start"], p["aniso_field"]["end"] = -1.0, 1.0
    return p


def _aniso_mtx(pkg, iso):
    p = pkg.params_for_config("C0")
    p["use_aniso_mtx"] = 1
    p["aniso_mtx"] = np.array([[1.0, 0.2, 0.0], [0.1, 0.8, 0.3], [0.0, -0.2, 1.5]], dtype=f32).ravel()
    p["isotropic_3d_sampling"] = iso
    return p


def _sandstone(pkg):
    p = pkg.params_for_config("C3")
    p["impulse_density"] = 12
    p["multi_resolution_grid"] = 1
    p["isotropic_3d_sampling"] = 1
    p["correlation_context"] = pkg.CTX.RENEWAL
    p["ls_ramp_type"] = 4
    for key, lo, hi in (("var", 0.5, 1.6), ("mean_color", 0.0, 0.0), ("mean_emission", 0.0, 0.0)):
        p[key]["enabled"], p[key]["type"] = 1, 4
        p[key]["min"], p[key]["max"] = lo, hi
    return p


def _phase_separate(pkg):
    import test_grid_oracle_cpu as G
    p = G._params(pkg, 1)
    p["multi_resolution_grid"], p["isotropic_3d_sampling"] = 1, 1
    p["correlation_context"] = pkg.CTX.RENEWAL
    p["surf_vol_phase_separate"], p["surf_vol_phase_amp_thresh"] = 1, 1.4
    return p


# name -> (base parameters, what the parity test of the feature compares with the oracle)
#   "all": every gpis_seg_out field, the coefficients and transmittance (test_absorption_only_branch, test_grid_nonstationary_covariance)
#   "t": no hit / miss flip, t where both agree (test_use_aniso_mtx has no march of its own: this is the toleranced media's comparison)
#   "t+weight": and the weight where exited and ok agree (test_variance_field_btlr_color_emission; test_sandstone_and_rust_noises
#               compares t alone, the weight is compared here too)
#   "t+tr": and transmittance up to max(1, n / 300) differences (test_aniso_field), with the conditioning's coefficients
ANCHORS = {
    "absorption-C0_perpath": (lambda pkg: _absorption(pkg, "C0_perpath"), "all"),
    "absorption-C2": (lambda pkg: _absorption(pkg, "C2"), "all"),
    "variance-multires": (lambda pkg: _variance(pkg, 1), "t+weight"),
    "variance": (lambda pkg: _variance(pkg, 0), "t+weight"),
    "aniso_field-world-renewal+": (lambda pkg: _aniso_field(pkg, 0, 0, "RENEWAL_PLUS"), "t+tr"),
    "aniso_field-iso-multires": (lambda pkg: _aniso_field(pkg, 1, 1, "RENEWAL"), "t+tr"),
    "aniso_mtx-world": (lambda pkg: _aniso_mtx(pkg, 0), "t"),
    "aniso_mtx-iso": (lambda pkg: _aniso_mtx(pkg, 1), "t"),
    "sandstone": (_sandstone, "t+weight"),
    "phase_separate": (_phase_separate, "all"),
}


def _hit_points(rays, out):
    """Vec3d ro + normalised(rd) * t: the point GPM.cpp:316 takes the colour at"""
    rd = rays["dir"].astype(np.float64)
    rd = rd * (1.0 / np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2]))[:, None]
    return rays["pos"].astype(np.float64) + rd * out["t"][:, None]


def _variance_grid():
    import test_grid_oracle_cpu as G
    return G._grid(24, seed=9), G._world_to_index(24)


def _anchor_rays(pkg, orc, absorption):
    """321 camera-like first-scatter segments and 321 continued ones from the oracle's hits (from a scattering twin's for the
    absorption-only media, as test_absorption_only_branch does)"""
    rays = smr.camera_rays(pkg, N_RAYS, 5)
    first = orc.sample_distance(rays)
    hits = (first["exited"] == 0) & (first["ok"] != 0)
    assert hits.sum() >= 16
    return rays, mfr.continued(pkg, first, 6)


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_constant_mean_anchor(pkg, ob, name):
    make, compare = ANCHORS[name]
    base = make(pkg)
    absorption = name.startswith("absorption")
    hom, _ = _constant_mean(pkg, base, "homogeneous")
    orc, dev = ob.Oracle(hom, threads=8), pkg.Medium(hom)
    if name == "phase_separate":
        orc.set_variance_grid(*_variance_grid(), "linear")
        dev.set_variance_grid(*_variance_grid(), "linear")
    twin = orc
    if absorption:
        scat = np.array(hom)
        scat["sigma_s"] = 1.0
        twin = ob.Oracle(scat, threads=8)
    batches = _anchor_rays(pkg, twin, absorption)
    q = smr.queries(pkg, mfr.N_QUERIES, 17, scale=1.3)
    rng = np.random.default_rng(3)
    tv, tg = rng.normal(0, 0.05, len(q)).astype(f32), rng.normal(0, 1, (len(q), 3)).astype(f32)
    pts = np.random.default_rng(8).uniform(-1.4, 1.4, (513, 3))

    def results(m):
        r = dict(value=m.eval_value(q), gradient=m.eval_gradient(q), cond=m.conditioning(q, tv, tg), colour=m.mean_color_emission(pts))
        r["march"] = [m.sample_distance(b, want_coeff=True) + (m.transmittance(b),) for b in batches]
        return r

    want_dev, want_orc = results(dev), results(orc)
    colour_on = int(base["mean_color"]["enabled"]) != 0
    if colour_on:
        assert not base["sigma_a"].any() and (base["sigma_s"] == 1).all() and base["density"] == 1          # weight = colour * 1
        pts32 = pts.astype(f32).astype(np.float64)
        want_dev_narrow, want_orc_narrow = dict(colour=dev.mean_color_emission(pts32)), dict(colour=orc.mean_color_emission(pts32))
        assert (want_orc_narrow["colour"][0] != want_orc["colour"][0]).any()
    dev.close()
    # the oracle's batches are worth comparing with: blocked and unblocked segments, or hits and exits, over the two batches
    outs = np.concatenate([out for out, _, _ in want_orc["march"]])
    if absorption:
        w = outs["weight"][outs["ok"] == 1][:, 0]
        assert (outs["exited"] == 1).all() and (w == 0).sum() >= 32 and (w == 1).sum() >= 32
    else:
        assert (outs["exited"] == 0).sum() >= 32 and (outs["exited"] != 0).sum() >= 32
    for kind in ("grid", "plane"):
        params, grids = _constant_mean(pkg, base, kind)
        m = _medium(pkg, (params, grids, (None, None)))
        if name == "phase_separate":
            m.set_variance_grid(*_variance_grid(), "linear")
        assert int(m.derived()["fast_path"]) == 0
        mv, _, mg = m.mean(pts)
        assert (mv == np.float64(f32(MEAN))).all() and not mg.any()
        got = results(m)
        m.close()
        # (a) the device's own homogeneous medium, bit for bit
        assert np.array_equal(got["value"][1], want_dev["value"][1])
        _same_arrays(got["value"][0], want_dev["value"][0], (kind, "value"))
        _same_arrays(got["gradient"], want_dev["gradient"], (kind, "gradient"))
        _same_records(got["cond"], want_dev["cond"], COEFF + ("n_evals",))
        # a procedural mean takes its colour at T^-1 Vec3f(a) (ProceduralMean::color), with the identity transform at the point narrowed
        # to float: the fully clipped plane has the homogeneous medium's colour at those points, and so have its hits' weights
        narrowed = kind == "plane" and colour_on
        _same_arrays(got["colour"][0], (want_dev_narrow if narrowed else want_dev)["colour"][0], (kind, "colour"))
        if kind == "plane":           # a tabulated primary mean emits 0 (TabulatedMean::emission without an emission grid)
            _same_arrays(got["colour"][1], want_dev["colour"][1], (kind, "emission"))
        else:
            assert not got["colour"][1].any()
        weights = ("weight", "continued_weight")
        for b, (out, coeff, vis), (wout, wcoeff, wvis) in zip(batches, got["march"], want_dev["march"]):
            _same_records(out, wout, tuple(f for f in pkg.SEG_OUT.names if not (narrowed and f in weights)))
            _same_records(coeff, wcoeff, COEFF + ("n_evals",))
            assert np.array_equal(vis, wvis)
            if narrowed:
                h = (wout["exited"] == 0) & (wout["ok"] != 0)
                _same_records(out[~h], wout[~h], weights)
                want_w = orc.mean_color_emission(_hit_points(b[h], wout[h]).astype(f32).astype(np.float64))[0]
                assert h.sum() >= 16 and (want_w != wout["weight"][h]).any()
                for f in weights:
                    _same_arrays(out[f][h], want_w, (kind, f))
        # (b) the oracle, as the parity test of the feature compares
        assert np.array_equal(got["value"][1], want_orc["value"][1])
        assert np.array_equal(got["value"][0], want_orc["value"][0])
        assert np.array_equal(got["gradient"], want_orc["gradient"], equal_nan=True)
        assert np.array_equal(got["colour"][0], (want_orc_narrow if narrowed else want_orc)["colour"][0])
        if compare in ("all", "t+tr"):
            for f in COEFF:
                assert np.array_equal(got["cond"][f], want_orc["cond"][f]), f
        for (out, coeff, vis), (wout, wcoeff, wvis) in zip(got["march"], want_orc["march"]):
            assert np.array_equal(out["exited"], wout["exited"]), "hit / miss flips: %d" % (out["exited"] != wout["exited"]).sum()
            assert np.array_equal(out["t"], wout["t"])
            if compare == "all":
                for f in pkg.SEG_OUT.names:
                    assert np.array_equal(out[f], wout[f], equal_nan=True), f
                for f in ("ray_origin", "n_evals") if int(base["sampling_1d"]) else COEFF + ("n_evals",):
                    assert np.array_equal(coeff[f], wcoeff[f]), f
                assert np.array_equal(vis, wvis)
            elif compare == "t+weight":
                same = (out["ok"] == wout["ok"]) & ~(narrowed & (wout["exited"] == 0))          # the plane's hit weights: see (a)
                assert np.array_equal(out["weight"][same], wout["weight"][same])
            elif compare == "t+tr":
                assert (vis != wvis).sum() <= max(1, len(vis) // 300)
