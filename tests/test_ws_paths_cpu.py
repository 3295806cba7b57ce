"""CPU checks of the weight-space path frame: the declared interface, the pin of the plain-C shade step
(tests/native/ws_paths_shade.c) against the oracle the sparse-convolution path driver is checked against, the non-vacuity of
every GPU case's composite (tests/ws_paths_ref.py: CASES), the context sensitivity of the composite, its recorded fixture and its
own partition invariance."""
import os
import re
import sys

import numpy as np
import pytest

import ws_oracle
import ws_paths_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ws_paths_small.npz")
needs_cc = pytest.mark.skipif(not ws_paths_ref.available(), reason="no C compiler for the restatement")


@pytest.fixture(scope="module")
def ref(pkg):
    return ws_paths_ref.PathsRef(pkg)


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_path_entry_is_declared():
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    assert re.search(r"^int\s+gpis_ws_render_scene_s_paths\s*\(gpis_medium \*m, const gpis_scene_s \*s, int max_path_bounces, float albedo,\s*"
                     r"float \*radiance_sum, void \*stream\);", header, flags=re.M)
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    assert callable(getattr(pkg.WeightSpaceMedium, "render_scene_s_paths", None))
    assert "gpis_ws_render_scene_s_paths" in pkg.GpisLib.SYMBOLS


@needs_cc
def test_shade_step_is_the_oracles(pkg, ob, ref):
    """The composite with the sparse-convolution oracle's sampleDistance / transmittance underneath is
    Oracle.render_scene_s_paths, bit for bit (C0, 16 x 12 x 2, 3 bounces)."""
    orc = ob.Oracle(pkg.params_for_config("C0"), threads=4)
    scene = ob.default_scene_s(16, 12, 2)
    want = orc.render_scene_s_paths(scene, 3, 0.8)
    c = ref.compose(ws_paths_ref.ScMarch(orc), scene, 3, 0.8)
    assert want.any() and c.n_three_hits and c.n_visible and c.n_occluded and c.n_exit_after_hit
    assert np.array_equal(_bits(c.image), _bits(want))
    # and on the frame the weight-space cases use (24 x 16 x 4, fov 60: samples that miss the bound), at 4 bounces, albedo 1
    scene = ws_paths_ref.small_scene(ob)
    want = orc.render_scene_s_paths(scene, 4, 1.0)
    c = ref.compose(ws_paths_ref.ScMarch(orc), scene, 4, 1.0)
    assert c.n_miss and c.max_hits == 4
    assert np.array_equal(_bits(c.image), _bits(want))


@needs_cc
@pytest.mark.parametrize("case", sorted(ws_paths_ref.CASES))
def test_case_is_not_vacuous(pkg, ob, ref, wso, case):
    p, w, scene, max_bounces, albedo, impossible = ws_paths_ref.case_inputs(pkg, ob, case)
    c = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, max_bounces, albedo)
    ws_paths_ref.check_non_vacuous(c, impossible)
    assert c.n_seg == c.n_path_seg + c.n_shadow_seg and c.n_eval > 0
    assert c.image.any() == (c.n_visible > 0)
    if "two_ids" in case or case == "n0":
        assert c.hit_gp_ids == {0, 1}
    if max_bounces == 1:
        assert not c.image.any() and c.n_seg == c.n_samples - c.n_miss       # all zero, and still counts its segments


@needs_cc
def test_contexts_are_exercised(pkg, ob, ref, wso):
    """Per-path realizations, max_bounces >= 2: GLOBAL keeps one realization per path, the other contexts draw a new one per
    segment word, so the composites differ; the three renewing contexts share one rule (WSM:164-173) and agree; a single
    realization does not depend on the context."""
    out = {}
    for ctx in ws_paths_ref.CTXS:
        for single in (0, 1):
            p, w, scene, mb, alb, _ = ws_paths_ref.case_inputs(pkg, ob, "%s-single%d" % (ctx, single))
            out[ctx, single] = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, mb, alb)
    assert not np.array_equal(_bits(out["global", 0].image), _bits(out["renewal", 0].image))
    assert out["global", 0].n_eval != out["renewal", 0].n_eval
    for ctx in ("renewal_plus", "none"):
        assert np.array_equal(_bits(out[ctx, 0].image), _bits(out["renewal", 0].image))
    for ctx in ws_paths_ref.CTXS:
        assert np.array_equal(_bits(out[ctx, 1].image), _bits(out["global", 1].image))
    assert not np.array_equal(_bits(out["global", 1].image), _bits(out["global", 0].image))
    # with one segment per path there is nothing to renew: the contexts cannot be told apart
    p, w, scene, _, alb, _ = ws_paths_ref.case_inputs(pkg, ob, "global-single0")
    p2, w2, _, _, _, _ = ws_paths_ref.case_inputs(pkg, ob, "renewal-single0")
    a = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, 1, alb)
    b = ref.compose(ws_paths_ref.WsMarch(p2, w2, wso), scene, 1, alb)
    assert a.n_eval == b.n_eval and a.n_seg == b.n_seg


@needs_cc
def test_composite_equals_fixture(pkg, ref, wso):
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    w = np.array(g["ws"]).view(pkg.WS_PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    c = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, int(g["max_bounces"]), float(g["albedo"]))
    assert np.array_equal(_bits(c.image), _bits(g["image"])) and g["image"].any()
    assert c.n_eval == int(g["n_eval"]) and c.n_seg == int(g["n_seg"])
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ws_paths_golden as mk
    p2, w2, scene2 = mk.fixture_inputs(pkg)
    assert p2.tobytes() == p.tobytes() and w2.tobytes() == w.tobytes() and np.array(scene2, dtype=pkg.SCENE_S).tobytes() == scene.tobytes()
    assert (mk.MAX_BOUNCES, np.float32(mk.ALBEDO)) == (int(g["max_bounces"]), np.float32(g["albedo"]))


@needs_cc
@pytest.mark.parametrize("kind", ["shards", "rows", "spp", "spp_assoc"])
def test_composite_partition_invariance(pkg, ob, ref, wso, kind):
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=65)
    march = ws_paths_ref.WsMarch(p, w, wso)
    whole_scene, calls = ws_paths_ref.parts(ob, kind)
    whole = ref.compose(march, whole_scene, 3, 0.8)
    acc = None
    for s in calls:
        acc = ref.compose(march, s, 3, 0.8, into=acc)
    assert acc.n_samples == whole.n_samples and acc.n_seg == whole.n_seg and acc.n_eval == whole.n_eval
    assert whole.n_visible and whole.n_occluded and whole.n_miss and whole.n_three_hits
    if kind == "spp_assoc":
        # each call sums its samples from zero and adds the sum to the image once: the accumulated image is the float32 sum of
        # the two calls' images, and differs from the whole frame by the reassociation of five non-negative terms only (at
        # most four roundings of 2^-24 relative on either side: below 1e-6)
        two = ref.compose(march, calls[0], 3, 0.8)
        rest = ref.compose(march, calls[1], 3, 0.8)
        assert np.array_equal(_bits(acc.image), _bits(two.image + rest.image))
        assert np.allclose(acc.image, whole.image, rtol=1e-6, atol=0)
    else:
        assert np.array_equal(_bits(acc.image), _bits(whole.image))
