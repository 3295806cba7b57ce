"""The march composite of tests/sdf_march_ref.py against the frozen oracle, where the oracle can judge it.

(a) With an ANALYTIC mean the composite (noise from the oracle's homogeneous-0 medium + the mean of tests/sdf_mean_ref.py) must
    reproduce the oracle's own sample_distance / transmittance in every field and coefficient, bit for bit: this checks the
    composite's march, conditioning reduction and record filling with nothing procedural in it.
(b) With func = plane, scale = 1, offset = 0 the procedural mean's VALUE equals LinearMean(ref = 0, dir = (0, 1, 0)) exactly, its
    gradient is the one-sided difference instead of (0, 1, 0).  So t, exited, last_val and every field that does not depend on the
    gradient must equal the oracle's on the linear-mean medium bit for bit; the gradient-dependent ones (aniso, through it ok and
    what ok gates) are compared where both gradients agree in the sign tests.  Renewal+ conditions a continued segment on the
    gradient, so there the continued segments of (b) are compared on the exit / hit class only; (a) covers them exactly.

The class counts of each case are recorded below; the conditions on the chosen rays (a quarter hit, a tenth exit, a refinement
with more than one trip) are asserted."""
import numpy as np
import pytest

import sdf_march_ref as smr
import sdf_mean_ref

pytestmark = pytest.mark.skipif(not sdf_mean_ref.available(), reason="no C compiler for the restatement")

N = 321
GRADIENT_FIELDS = ("aniso", "ok", "sample_t", "continued_t", "weight", "continued_weight", "p", "scheme")
# case -> (hits, exits, !ok, segments with more than one refinement trip) of the first-scatter and of the continued batch,
# counted on the oracle's linear-mean medium / the composite's trips
COUNTS = {
    "none": ((89, 232, 20, 59), (229, 92, 141, 70)),
    "renewal": ((93, 228, 20, 61), (220, 101, 121, 76)),
    "renewal+": ((93, 228, 20, 61), (236, 85, 128, 84)),
    "1d_mis": ((98, 223, 38, 71), (237, 84, 144, 85)),
}


def base(pkg, name):
    p = pkg.params_for_config("C2" if name == "1d_mis" else "C0")
    p["step_size"] = 0.02
    if name == "renewal":
        p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL
    elif name == "renewal+":
        p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL_PLUS
    return p


def linear(pkg, p):
    q = np.array(p)
    q["mean"]["type"] = pkg.MEAN_TYPE.LINEAR
    q["mean"]["center"] = 0.0
    q["mean"]["dir"] = (0.0, 1.0, 0.0)
    q["mean"]["scale"] = 1.0
    return q


def continued_rays(pkg, first_out, seed):
    """N continued segments starting at hit points of the first batch, in random directions, with the state the hit left"""
    idx = np.nonzero((first_out["exited"] == 0) & (first_out["ok"] != 0))[0]
    pick = idx[np.arange(N) % len(idx)]
    r = smr.camera_rays(pkg, N, seed, first_scatter=False, state=(0.0, first_out["aniso"][pick], 0))
    rng = np.random.default_rng(seed + 1)
    d = rng.normal(size=(N, 3))
    r["pos"] = first_out["p"][pick]
    r["dir"] = d / np.linalg.norm(d, axis=1)[:, None]
    r["near_t"] = 0
    r["far_t"] = rng.uniform(0.2, 1.2, N)
    r["info_t"] = first_out["sample_t"][pick]
    return r


def _same(a, b, fields, where=None):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        eq = x.view(np.uint8).reshape(len(a), -1) == y.view(np.uint8).reshape(len(b), -1)
        eq = eq.all(axis=1)
        if where is not None:
            eq = eq | ~where
        assert eq.all(), (f, np.nonzero(~eq)[0][:8])


def _counts(out, trips):
    return (int((out["exited"] == 0).sum()), int((out["exited"] != 0).sum()), int((out["ok"] == 0).sum()), int((trips > 1).sum()))


@pytest.fixture(scope="module", params=sorted(COUNTS))
def case(request, pkg, ob):
    name = request.param
    p = base(pkg, name)
    lin = linear(pkg, p)
    orc = ob.Oracle(lin, threads=8)
    rays = smr.camera_rays(pkg, N, 5)
    want, wcoeff = orc.sample_distance(rays, want_coeff=True)
    rays2 = continued_rays(pkg, want, 6)
    want2, wcoeff2 = orc.sample_distance(rays2, want_coeff=True)
    return dict(name=name, p=p, lin=lin, orc=orc, rays=rays, rays2=rays2, want=want, want2=want2, wcoeff=wcoeff, wcoeff2=wcoeff2)


def test_composite_with_the_linear_mean_is_the_oracle(pkg, ob, case):
    comp = smr.SdfComposite(pkg, ob, case["lin"], threads=8)
    fields = pkg.SEG_OUT.names
    for rays, want, wcoeff in ((case["rays"], case["want"], case["wcoeff"]), (case["rays2"], case["want2"], case["wcoeff2"])):
        got, coeff, trips = comp.sample_distance(rays, want_coeff=True, want_trips=True)
        _same(got, want, fields)
        _same(coeff, wcoeff, ("value_scale", "gradient_scale", "ray_origin"))
        if case["name"] != "1d_mis":           # the composite counts the 3D evaluators' noise evaluations as the oracle does, ray by ray
            _same(coeff, wcoeff, ("n_evals",))
        assert np.array_equal(comp.transmittance(rays), case["orc"].transmittance(rays))


def test_plane_mean_is_the_linear_mean(pkg, ob, case):
    comp = smr.SdfComposite(pkg, ob, smr.procedural(pkg, case["p"], "plane"), threads=8)
    # the premise: equal values, different gradients
    pts = np.random.default_rng(3).uniform(-1.5, 1.5, (257, 3))
    v, _, g = comp.mean(pts)
    assert np.array_equal(v, pts[:, 1].astype(np.float32).astype(np.float64)) and not np.array_equal(g[:, 1], np.ones(257))
    assert np.allclose(g, (0, 1, 0), rtol=0, atol=2e-4)
    value_fields = tuple(f for f in pkg.SEG_OUT.names if f not in GRADIENT_FIELDS)
    for k, (rays, want) in enumerate(((case["rays"], case["want"]), (case["rays2"], case["want2"]))):
        got, coeff, trips = comp.sample_distance(rays, want_coeff=True, want_trips=True)
        counts = _counts(want, trips)
        print(case["name"], "first" if k == 0 else "continued", "hits, exits, !ok, trips > 1:", counts)
        assert counts[0] >= N // 4 and counts[1] >= N // 10 and counts[3] >= 1
        if k == 1 and case["name"] in ("renewal+", "1d_mis"):
            # conditioned on the gradient: the two fields differ by the gradients' difference (see the module text)
            assert (got["exited"] == want["exited"]).mean() > 0.97
            continue
        assert counts == COUNTS[case["name"]][k]
        _same(got, want, value_fields)
        agree = (got["ok"] == want["ok"])          # both gradients on the same side of the two sign tests
        assert agree.mean() > 0.97
        _same(got, want, tuple(f for f in GRADIENT_FIELDS if f != "aniso"), where=agree)
        # the two gradients differ by the mean's alone: the one-sided difference of float(y) over eps = 1e-3 is off (0, 1, 0) by at most
        # an ulp of 1.5 (1.2e-7) over eps = 1.2e-4, narrowed to float once more
        assert np.allclose(got["aniso"][agree], want["aniso"][agree], rtol=1e-6, atol=2e-4)
        assert np.array_equal(comp.transmittance(rays), case["orc"].transmittance(rays))


# ---- (c) a CSG pair and a non-finite gradient, on analytic media ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ("none", "renewal+"))
def test_composite_on_an_analytic_csg_pair_is_the_oracle(pkg, ob, name):
    """LinearMean (y, scale 1) united with a sphere of radius 0.5 about (0.7, 0.3, 0): the composite takes value, gradient and the
    conditioning's reduction from the slot the CSG minimum chose and carries gp_id into the continued segments, as the oracle does.
    Both ids occur among the hits and among the continued segments' last_gp_id."""
    import mean_features_ref as mfr
    p = linear(pkg, base(pkg, name))
    p["has_mean_additional"] = 1
    p["mean_additional"]["type"] = pkg.MEAN_TYPE.SPHERICAL
    p["mean_additional"]["radius"] = 0.5
    p["mean_additional"]["center"] = (0.7, 0.3, 0.0)
    orc = ob.Oracle(p, threads=8)
    comp = smr.SdfComposite(pkg, ob, p, threads=8)
    rays = smr.camera_rays(pkg, N, 5)
    first = orc.sample_distance(rays)
    for r in (rays, mfr.continued(pkg, first, 6)):
        want, wcoeff = orc.sample_distance(r, want_coeff=True)
        hit = want["exited"] == 0
        ids = [int((hit & (want["gp_id"] == i)).sum()) for i in (0, 1)]
        last = [int((r["last_gp_id"] == i).sum()) for i in (0, 1)]
        print(name, "hits per gp_id", ids, "last_gp_id", last)
        assert min(ids) >= 16 and (r["first_scatter"].all() or min(last) >= 16)
        got, coeff = comp.sample_distance(r, want_coeff=True)
        _same(got, want, pkg.SEG_OUT.names)
        _same(coeff, wcoeff, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
        assert np.array_equal(comp.transmittance(r), orc.transmittance(r))


def test_composite_with_a_non_finite_gradient_is_the_oracle(pkg, ob):
    """Matern 5/2, Renewal: a continued segment whose refinement falls back to t = 0 evaluates the gradient at the conditioning point,
    where the kernel's derivative is 0 / 0; sampleDistance fails such a segment with aniso = (1, 0, 0) (GPM.cpp:291) and transmittance
    blocks it.  The spherical mean is the oracle's own, so the composite's handling of that class is pinned here."""
    import mean_features_ref as mfr
    p = mfr.config(pkg, "matern")
    orc = ob.Oracle(p, threads=8)
    comp = smr.SdfComposite(pkg, ob, p, threads=8)
    first = orc.sample_distance(smr.camera_rays(pkg, N, 5))
    r = mfr.continued(pkg, first, 22)
    want, wcoeff = orc.sample_distance(r, want_coeff=True)
    failed = (want["ok"] == 0) & (want["exited"] == 0) & (want["t"] == 0) & (want["aniso"] == (1.0, 0.0, 0.0)).all(axis=1)
    assert failed.sum() == 4
    got, coeff = comp.sample_distance(r, want_coeff=True)
    _same(got, want, pkg.SEG_OUT.names)
    _same(coeff, wcoeff, ("value_scale", "gradient_scale", "ray_origin", "n_evals"))
    assert np.array_equal(comp.transmittance(r), orc.transmittance(r))
