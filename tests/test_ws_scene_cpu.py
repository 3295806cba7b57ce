"""CPU checks of the weight-space scene-S frame: the declared interface, the CPU composite (tests/ws_scene_ref.py) against its
recorded fixture, and the composite's own partition invariance (shards, row ranges and spp ranges add up to the whole frame, in
float32 and in the same order of addition)."""
import os
import re

import numpy as np
import pytest

import ws_oracle
import ws_scene_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ws_scene_small.npz")
needs_cc = pytest.mark.skipif(not ws_scene_ref.available(), reason="no C compiler for the restatement")


@pytest.fixture(scope="module")
def ref(pkg, ob):
    return ws_scene_ref.SceneRef(pkg, ob)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_frame_entry_is_declared():
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    assert re.search(r"^int\s+gpis_ws_render_scene_s\s*\(gpis_medium \*m, const gpis_scene_s \*s, float \*radiance_sum,\s*uint32_t \*hit_count, void \*stream\);",
                     header, flags=re.M)
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    assert callable(getattr(pkg.WeightSpaceMedium, "render_scene_s", None))
    assert "gpis_ws_render_scene_s" in pkg.GpisLib.SYMBOLS


@needs_cc
def test_composite_equals_fixture(pkg, ref):
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    w = np.array(g["ws"]).view(pkg.WS_PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    c = ref.compose(p, w, scene)
    assert np.array_equal(_bits(c.image), _bits(g["image"]))
    assert np.array_equal(c.hits, g["hits"])
    # the fixture is the configuration its recorder states
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_ws_scene_golden
    p2, w2, scene2 = make_ws_scene_golden.fixture_inputs(pkg)
    assert p2.tobytes() == p.tobytes() and w2.tobytes() == w.tobytes() and np.array(scene2, dtype=pkg.SCENE_S).tobytes() == scene.tobytes()


def _parts(ob, kind):
    """scenes of the calls that together cover small_scene (40 rows here, so that three shards of 8-pixel tiles all get rows)"""
    def base():
        s = ws_scene_ref.small_scene(ob, width=12, height=40, spp=5)
        s["tile_size"] = 8
        return s
    out = []
    if kind == "shards":
        for k in range(3):
            s = base()
            s["shard_index"], s["shard_count"] = k, 3
            out.append(s)
    elif kind == "rows":
        for y0, yc in ((0, 17), (17, 23)):
            s = base()
            s["y_begin"], s["y_count"] = y0, yc
            out.append(s)
    else:
        # "spp": the second call adds ONE sample per pixel, so ((((a0 + a1) + a2) + a3) + a4 is the whole frame's own order;
        # "spp_assoc": (a0 + a1) + ((a2 + a3) + a4), another float32 association than the whole frame's
        for s0, sn in (((0, 4), (4, 1)) if kind == "spp" else ((0, 2), (2, 3))):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    return base(), out


@needs_cc
@pytest.mark.parametrize("kind", ["shards", "rows", "spp", "spp_assoc"])
def test_composite_partition_invariance(pkg, ob, ref, kind):
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=65)
    whole_scene, parts = _parts(ob, kind)
    whole = ref.compose(p, w, whole_scene)
    acc = None
    for s in parts:
        acc = ref.compose(p, w, s, into=acc)
    assert acc.n_samples == whole.n_samples and acc.n_seg == whole.n_seg and acc.n_eval == whole.n_eval
    assert np.array_equal(acc.hits, whole.hits) and whole.n_visible and whole.n_occluded and whole.n_miss
    if kind == "spp_assoc":
        # each call sums its samples from zero and adds the sum to the image once: the accumulated image is the float32 sum of
        # the two calls' images, and differs from the whole frame by the reassociation of five non-negative terms only (at
        # most four roundings of 2^-24 relative on either side: below 1e-6)
        two = ref.compose(p, w, parts[0])
        rest = ref.compose(p, w, parts[1])
        assert np.array_equal(_bits(acc.image), _bits(two.image + rest.image))
        assert np.allclose(acc.image, whole.image, rtol=1e-6, atol=0)
    else:
        assert np.array_equal(_bits(acc.image), _bits(whole.image))
