"""NEE with an out-of-line mean, on the CPU: the reference of tests/test_gpu_mean_nee.py against the frozen oracle where the oracle
can judge it, and the input conditions of the GPU cases on the reference alone.

(a) SdfComposite.nee_pdf / nee_grad (tests/sdf_march_ref.py) answer through the oracle of a LINEAR stand-in whose gradient is, in
    float, the mean's.  On ANALYTIC media the oracle knows the medium itself, so the two must agree bit for bit: axis-linear means of
    both signs with an arbitrary centre, scale and direction length, with and without `min` clipping, a homogeneous mean, and a CSG
    pair of two axis-linear means (which pins the slot the gradient is taken from).  A general gradient is refused.
(b) The cases of tests/mean_nee_ref.py: the selected queries per class, the CSG ids, pdf > 0 / pdf == 0, and for the plane cases that
    the one-sided difference and the analytic gradient give different results (COUNTS records what was seen; the bounds the issue sets
    are asserted).
(c) The frames: hits and misses on the plane medium, and the constant-grid composite against oracle_render_scene_s_nee."""
import numpy as np
import pytest

import grid_march_ref as gmr
import mean_nee_ref as mnr
import nee_paths_ref as npr
import sdf_march_ref as smr
import sdf_mean_ref

pytestmark = pytest.mark.skipif(not (sdf_mean_ref.available() and npr.available()), reason="no C compiler for the restatements")

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _linear(pkg, base, axis, sign, scale=0.7, length=1.0, minimum=None, slot="mean", center=(0.1, -0.2, 0.05)):
    p = np.array(base)
    d = np.zeros(3)
    d[axis] = sign * length
    mu = p[slot]
    mu["type"], mu["center"], mu["dir"], mu["scale"] = pkg.MEAN_TYPE.LINEAR, center, d, scale
    mu["min"] = -np.finfo(f32).max if minimum is None else minimum
    if slot == "mean_additional":
        p["has_mean_additional"] = 1
    return p


def _check_against_the_medium_itself(pkg, ob, params, seed, want_zero=False, want_ids=False):
    comp = smr.SdfComposite(pkg, ob, params, threads=8)
    orc = ob.Oracle(params, threads=8)
    pts = np.random.default_rng(seed).uniform(-1.3, 1.3, (mnr.N_QUERIES, 3)).astype(f32)
    _, gid, g = comp.mean(pts.astype(np.float64))
    q = smr.nee_queries(pkg, pts, g, seed + 1)
    k, s = comp.nee_standin(q)
    if want_zero:
        assert (k < 0).sum() >= 32 and (k >= 0).sum() >= 32
    if want_ids:
        assert (gid == 0).sum() >= 32 and (gid == 1).sum() >= 32 and len(set(k[k >= 0])) == 2
    pdf, grad = comp.nee_pdf(q), comp.nee_grad(q)
    wpdf, wgrad = orc.nee_pdf(q), orc.nee_grad(q)
    assert (wpdf > 0).sum() >= 64 and (wpdf == 0).sum() >= 16
    assert np.array_equal(_bits(pdf), _bits(wpdf)), np.nonzero(_bits(pdf) != _bits(wpdf))[0][:8]
    assert np.array_equal(_bits(grad), _bits(wgrad)), np.nonzero((_bits(grad) != _bits(wgrad)).any(axis=1))[0][:8]
    return comp, q, pdf, grad


# ---- (a) --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(mnr.FAMILY))
@pytest.mark.parametrize("axis,sign", [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)])
def test_axis_linear_mean_is_its_own_standin(pkg, ob, family, axis, sign):
    """LinearMean along +-e_k, centre (0.1, -0.2, 0.05), scale 0.7 or 1.3, direction given unnormalised"""
    params = _linear(pkg, mnr.c2(pkg, family), axis, sign, scale=0.7 if sign > 0 else 1.3, length=1.0 if axis != 1 else 2.0)
    _check_against_the_medium_itself(pkg, ob, params, seed=3 + axis)


def test_standin_depends_on_the_scale_and_not_on_the_centre(pkg, ob):
    """what makes the comparison a test of the gradient: another scale changes the oracle's NEE, another centre does not"""
    base = mnr.c2(pkg, "renewal+xy-mis")
    comp, q, pdf, grad = _check_against_the_medium_itself(pkg, ob, _linear(pkg, base, 1, 1, scale=0.99853516), seed=7)
    moved = ob.Oracle(_linear(pkg, base, 1, 1, scale=0.99853516, center=(-0.4, 0.3, 0.2)), threads=8)
    assert np.array_equal(_bits(moved.nee_pdf(q)), _bits(pdf)) and np.array_equal(_bits(moved.nee_grad(q)), _bits(grad))
    one = ob.Oracle(_linear(pkg, base, 1, 1, scale=1.0), threads=8)
    assert (_bits(one.nee_grad(q)) != _bits(grad)).any(axis=1).mean() > 0.9 and (_bits(one.nee_pdf(q)) != _bits(pdf)).mean() > 0.2


@pytest.mark.parametrize("family", sorted(mnr.FAMILY))
def test_clipped_linear_and_homogeneous_means(pkg, ob, family):
    base = mnr.c2(pkg, family)
    _check_against_the_medium_itself(pkg, ob, _linear(pkg, base, 2, -1, scale=0.9, minimum=-0.2), seed=11, want_zero=True)
    hom = np.array(base)
    hom["mean"]["type"], hom["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.3
    _check_against_the_medium_itself(pkg, ob, hom, seed=12)


@pytest.mark.parametrize("family", sorted(mnr.FAMILY))
def test_csg_pair_of_axis_linear_means(pkg, ob, family):
    """0.7 (y + 0.2) united with 1.3 (0.3 - x): the gradient comes from the slot the CSG minimum chose, both slots occur"""
    p = _linear(pkg, mnr.c2(pkg, family), 1, 1, scale=0.7, center=(0.0, -0.2, 0.0))
    p = _linear(pkg, p, 0, -1, scale=1.3, slot="mean_additional", center=(0.3, 0.0, 0.0))
    _check_against_the_medium_itself(pkg, ob, p, seed=13, want_ids=True)


def test_general_gradient_is_refused(pkg, ob):
    comp = smr.SdfComposite(pkg, ob, smr.procedural(pkg, mnr.c2(pkg, "none-mis"), "two_spheres"), threads=1)
    pts = np.random.default_rng(5).uniform(-1, 1, (16, 3)).astype(f32)
    q = smr.nee_queries(pkg, pts, np.ones((16, 3)), 6)
    with pytest.raises(ValueError, match="axis-aligned"):
        comp.nee_pdf(q)
    with pytest.raises(ValueError, match="axis-aligned"):
        comp.nee_grad(q)


# ---- (b) --------------------------------------------------------------------------------------------------------------------------
# mean -> (points of the pool that qualify, selected, zero-gradient, non-zero, axes, negative gradients, distinct magnitudes, [id 0, id 1])
COUNTS = {
    "plane": (4096, 512, 0, 512, [1], 0, 9, [512, 0]),
    "plane-x": (4096, 512, 0, 512, [0], 512, 11, [512, 0]),
    "plane-z": (4096, 512, 0, 512, [2], 0, 11, [512, 0]),
    "plane-min": (4096, 512, 256, 256, [1], 0, 7, [512, 0]),
    "knob": (364, 364, 0, 364, [1], 319, 47, [364, 0]),
    "grid-point": (4192, 512, 402, 110, [2], 0, 9, [512, 0]),
    "grid-linear": (4096, 512, 256, 256, [2], 0, 50, [512, 0]),
    "csg-plane-slab": (4096, 512, 170, 342, [0, 1], 99, 28, [172, 340]),
    "csg-slab-plane": (4096, 512, 170, 342, [0, 1], 99, 28, [340, 172]),
}
# pdf > 0 / pdf == 0 / pdf < 0 over the four media: 95 ... 157 / 155 ... 296 / 95 ... 157 of the selected queries.  The queries are synthetic
# (a normal no path would produce next to this ray direction), and the oracle's neePDF is negative on a quarter of them; the device
# is compared on those all the same.


@pytest.mark.parametrize("family", sorted(mnr.FAMILY))
@pytest.mark.parametrize("mean", mnr.MEANS)
def test_case_conditions_hold_on_the_reference(pkg, ob, family, mean):
    r = mnr.reference(pkg, ob, family, mean)
    i, pdf, grad = r["info"], r["pdf"], r["grad"]
    print(family, mean, i, "pdf > 0: %d, pdf == 0: %d, pdf < 0: %d" % ((pdf > 0).sum(), (pdf == 0).sum(), (pdf < 0).sum()))
    assert (i["qualifying"], i["selected"], i["zero"], i["nonzero"], i["axes"], i["negative"], i["magnitudes"], i["ids"]) == COUNTS[mean]
    assert (pdf > 0).sum() >= 64 and (pdf == 0).sum() >= 16 and np.isfinite(pdf).all() and np.isfinite(grad).all()
    if mean == "plane-min":
        assert i["zero"] >= 32 and i["nonzero"] >= 32
    if mean == "knob":
        assert i["selected"] >= 128
    if mean.startswith("grid"):
        assert i["selected"] >= 64 and i["nonzero"] >= 32
    if mean.startswith("csg"):
        assert min(i["ids"]) >= 32 and i["axes"] == [0, 1]
    if mean in ("plane-x", "plane-z"):
        assert i["axes"] == [0 if mean == "plane-x" else 2] and (i["negative"] == i["selected"]) == (mean == "plane-x")
    if mean.startswith("plane"):
        apdf, agrad = mnr.analytic_plane_nee(r["comp"], r["q"], mean)
        assert (_bits(agrad) != _bits(grad)).any()          # a device that took the plane's analytic gradient would be caught


# ---- (c) --------------------------------------------------------------------------------------------------------------------------
def test_plane_frame_has_hits_and_misses(pkg, ob):
    for b, marched in ((2, [1440]), (4, [1440, 311, 142])):
        c = mnr.frame_reference(pkg, ob, b)
        print(b, "marched", c.marched, "hits", c.hits, "light", c.light, "phase", c.phase, "missed the bound", c.n_miss)
        assert c.marched == marched and c.hits[0] == 313 and c.image.any()
        assert c.hits[0] >= c.marched[0] // 10 and c.marched[0] - c.hits[0] >= c.marched[0] // 10


def test_constant_grid_frame_is_the_oracles(pkg, ob):
    """the composite with a constant tabulated grid through NeePathsRef against oracle_render_scene_s_nee on the homogeneous medium"""
    p, grids, hom = mnr.constant_grid_medium(pkg)
    comp = gmr.GridComposite(pkg, ob, p, grids=grids, threads=8)
    surf = pkg.default_surface_s()
    c = npr.NeePathsRef(pkg, ob).compose(comp, npr.frame(ob), surf, 2)
    want = ob.Oracle(hom, threads=8).render_scene_s_nee(npr.frame(ob), surf)
    assert want.any() and np.array_equal(_bits(c.image), _bits(want))
