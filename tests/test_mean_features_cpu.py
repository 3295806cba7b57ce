"""The input conditions of tests/test_gpu_mean_features.py, on the composite alone (tests/mean_features_ref.py): every batch has hits
and exits and a refinement of more than one trip, the CSG pairs put both ids among the hits and among the continued segments'
last_gp_id, the Matern batch holds segments that fail on a non-finite gradient, and a colour field makes the hits' weights differ.
COUNTS records what was seen.  tests/test_sdf_march_cpu.py pins the composite itself to the oracle (a CSG pair and the non-finite
gradient included)."""
import numpy as np
import pytest

import mean_features_ref as mfr
import sdf_march_ref as smr
import sdf_mean_ref

pytestmark = pytest.mark.skipif(not sdf_mean_ref.available(), reason="no C compiler for the restatement")

N = mfr.N_RAYS
# key -> per batch (hits, exits, !ok, trips > 1, hits per gp_id, rays per last_gp_id)
COUNTS = {
    ("knob+sphere", "none"): ((254, 67, 0, 175, [224, 30], [321, 0]), (236, 85, 147, 90, [204, 32], [284, 37])),
    ("knob+sphere", "renewal"): ((256, 65, 3, 164, [226, 30], [321, 0]), (238, 83, 139, 82, [207, 31], [282, 39])),
    ("knob+sphere", "renewal+"): ((256, 65, 3, 164, [226, 30], [321, 0]), (229, 92, 143, 94, [200, 29], [282, 39])),
    ("grid+plane", "none"): ((230, 91, 14, 163, [158, 72], [321, 0]), (220, 101, 119, 96, [159, 61], [233, 88])),
    ("grid+plane", "renewal"): ((234, 87, 17, 147, [162, 72], [321, 0]), (247, 74, 137, 87, [181, 66], [240, 81])),
    ("grid+plane", "renewal+"): ((234, 87, 17, 147, [162, 72], [321, 0]), (212, 109, 125, 85, [154, 58], [240, 81])),
}


def _tuple(s):
    return (s["hits"], s["exits"], s["not_ok"], s["trips_gt_1"], s["hit_ids"], s["last_ids"])


@pytest.mark.parametrize("ctx", ("none", "renewal", "renewal+"))
@pytest.mark.parametrize("pair", ("knob+sphere", "grid+plane"))
def test_csg_batches_hold_both_ids(pkg, ob, pair, ctx):
    _, batches = mfr.march_reference(pkg, ob, (pair, ctx), mfr.csg_pair(pkg, mfr.march_base(pkg, ctx), pair))
    for k, b in enumerate(batches):
        s = mfr.summary(b)
        print(pair, ctx, "first" if k == 0 else "continued", s)
        assert _tuple(s) == COUNTS[pair, ctx][k]
        assert s["hits"] >= N // 10 and s["exits"] >= N // 10 and s["trips_gt_1"] >= 1 and min(s["hit_ids"]) >= 16
    assert min(mfr.summary(batches[1])["last_ids"]) >= 16


@pytest.mark.parametrize("name", ("iso-ray", "1d-xy", "matern"))
def test_other_config_batches(pkg, ob, name):
    medium = (smr.procedural(pkg, mfr.config(pkg, name), "knob"), (None, None), (None, None))
    _, batches = mfr.march_reference(pkg, ob, ("config", name), medium)
    for k, b in enumerate(batches):
        s = mfr.summary(b)
        print(name, "first" if k == 0 else "continued", s)
        assert s["hits"] >= N // 10 and s["exits"] >= N // 10 and s["trips_gt_1"] >= 1
    if name == "matern":
        w = batches[1]["out"]
        failed = (w["ok"] == 0) & (w["exited"] == 0) & (w["t"] == 0) & (w["aniso"] == (1.0, 0.0, 0.0)).all(axis=1)
        assert failed.sum() == 3           # the non-finite gradient at the conditioning point


@pytest.mark.parametrize("kind", ("ramp", "sandstone"))
def test_colour_reaches_the_hit_weight(pkg, ob, kind):
    medium = mfr.colour(pkg, mfr.march_base(pkg, "none"), kind)
    comp, batches = mfr.march_reference(pkg, ob, ("colour", kind), medium)
    w = batches[0]["out"]
    h = (w["exited"] == 0) & (w["ok"] != 0)
    distinct = len(np.unique(w["weight"][h], axis=0))
    print(kind, mfr.summary(batches[0]), "distinct hit weights", distinct)
    assert h.sum() >= N // 10 and distinct >= h.sum() // 2
    if kind == "sandstone":
        assert (w["weight"][h, 0] != w["weight"][h, 2]).any()            # a vector field
    # the colour point: under the transform the colour is taken at T^-1 p, which is not p
    pts = np.random.default_rng(8).uniform(-1, 1, (257, 3))
    col, _ = comp.mean_color_emission(pts)
    plain, _ = comp.noise.mean_color_emission(pts)
    assert (col != plain).any(axis=1).mean() > 0.9
