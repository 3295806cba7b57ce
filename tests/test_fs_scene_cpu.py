"""CPU checks of the function-space scene-S frame (gpis_fs_render_scene_s): the declared and exported interface, the CPU
composite (tests/fs_scene_ref.py) — that no case of the GPU parity test can pass vacuously, that its Python sampler state is the
one the oracle's own stream reaches, and that the composite does not depend on how a frame is cut into calls."""
import os
import re
import subprocess

import numpy as np
import pytest

import fs_scene_ref
import ws_scene_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_cc = pytest.mark.skipif(not fs_scene_ref.available(), reason="no C compiler for the shade step")

# samples, miss, exit, !ok, hit, lit, visible, occluded of each case's composite, as recorded when the cases were chosen
EXPECTED = {
    "renewal-16": (1536, 661, 387, 4, 484, 369, 151, 218),
    "none-12": (1536, 661, 441, 0, 434, 286, 118, 168),
    "global-14": (1536, 661, 393, 2, 480, 371, 214, 157),
    "renewal_plus-32": (1536, 661, 386, 2, 487, 373, 221, 152),
    "global-64": (192, 81, 53, 0, 58, 46, 24, 22),
}


@pytest.fixture(scope="module")
def ref(pkg, ob):
    return fs_scene_ref.FsSceneRef(pkg, ob)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_frame_entry_is_declared():
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    assert re.search(r"^int\s+gpis_fs_render_scene_s\s*\(gpis_medium \*m, const gpis_scene_s \*s, float \*radiance_sum,\s*uint32_t \*hit_count, void \*stream\);",
                     header, flags=re.M)
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    assert callable(getattr(pkg.Medium, "fs_render_scene_s", None))
    assert "gpis_fs_render_scene_s" in pkg.GpisLib.SYMBOLS


def test_library_exports_the_frame_entry(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_fs_render_scene_s$", out, flags=re.M)


@needs_cc
@pytest.mark.parametrize("name", sorted(fs_scene_ref.CASES))
def test_composite_is_not_vacuous(pkg, ob, ref, name):
    p, scene = fs_scene_ref.case(pkg, ob, name)
    c = ref.compose(p, scene)
    fs_scene_ref.assert_non_vacuous(c)
    assert c.image.any() and c.hits.any()
    assert c.n_samples == c.n_miss + c.n_exit + c.n_notok + c.n_hit and c.n_lit == c.n_visible + c.n_occluded
    assert (c.n_samples, c.n_miss, c.n_exit, c.n_notok, c.n_hit, c.n_lit, c.n_visible, c.n_occluded) == EXPECTED[name]


@needs_cc
def test_python_sampler_state_is_the_streams(pkg, ob, ref):
    """The state fs_scene_ref gives the primary segment is where oracle_scene_s_primary's own stream stands after jx, jy: its
    next two draws are the u_jitter and u_shadow that generator reports for the sample."""
    scene = ws_scene_ref.small_scene(ob, 24, 16, 4, spp_begin=3, fov=60.0)
    rays, us, _, _ = ref.base.primary_rays(scene)
    st = ref.primary_states(scene, rays)
    assert len(rays) > 500
    for k in range(0, len(rays), 7):
        s = int(st["sampler_state"][k])
        u0, s = fs_scene_ref.pcg_draw(s)
        u1, s = fs_scene_ref.pcg_draw(s)
        assert _bits(np.float32(u0)) == _bits(rays["u_jitter"][k]) and _bits(np.float32(u1)) == _bits(us[k]), k


def _parts(ob, kind):
    def base():
        s = ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0)
        s["tile_size"] = 4
        return s
    out = []
    if kind == "rows":
        for y0, yc in ((0, 7), (7, 9)):
            s = base()
            s["y_begin"], s["y_count"] = y0, yc
            out.append(s)
    elif kind == "shards":
        for k in range(2):
            s = base()
            s["shard_index"], s["shard_count"] = k, 2
            out.append(s)
    else:
        # "spp": [0, 2) + [2, 4); "spp_last": [0, 3) + [3, 4), which adds ONE sample and so keeps the whole frame's association
        for s0, sn in (((0, 2), (2, 2)) if kind == "spp" else ((0, 3), (3, 1))):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    return base(), out


@needs_cc
@pytest.mark.parametrize("kind", ["rows", "shards", "spp", "spp_last"])
def test_composite_is_invariant_under_cutting(pkg, ob, ref, kind):
    """Rows, shards and an spp cut that adds one last sample are bit-equal to the whole frame.  [0, 2) + [2, 4) cannot be for
    every pixel — float32 addition is not associative — and is held to fs_scene_ref.assert_spp_cut_equals_whole: bit-equal to
    the sum of the two calls' images, bit-equal to the whole frame wherever one range alone contributes, within four roundings
    elsewhere."""
    p = fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04)
    whole_scene, parts = _parts(ob, kind)
    whole = ref.compose(p, whole_scene)
    fs_scene_ref.assert_non_vacuous(whole)
    acc = None
    for s in parts:
        acc = ref.compose(p, s, into=acc)
    assert (acc.n_samples, acc.n_seg, acc.n_hit, acc.n_visible) == (whole.n_samples, whole.n_seg, whole.n_hit, whole.n_visible)
    assert np.array_equal(acc.hits, whole.hits)
    if kind == "spp":
        fs_scene_ref.assert_spp_cut_equals_whole(acc.image, [ref.compose(p, s).image for s in parts], whole.image)
    else:
        assert np.array_equal(_bits(acc.image), _bits(whole.image))
