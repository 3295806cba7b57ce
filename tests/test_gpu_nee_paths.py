"""GPU parity of the multi-bounce conductor NEE / MIS path driver (gpis_render_scene_s_nee_paths): image and per-pixel segment
counts BIT FOR BIT against the CPU composite (tests/nee_paths_ref.py: the oracle's batch entries bounce level by bounce level
around the plain-C shade step), against gpis_render_scene_s_nee where the two estimators coincide, and against itself under row
ranges, shards, spp ranges, chunks and tuning options; the degenerate frames, the counters and the refusals.  No tolerance on any
device result: images are compared as uint32 views."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import nee_paths_ref as npr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not npr.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(img, segs, want_img, want_segs):
    assert np.array_equal(segs, want_segs), np.argwhere(segs != want_segs)[:8]
    assert np.array_equal(_bits(img), _bits(want_img)), np.argwhere(_bits(img) != _bits(want_img))[:8]


def _medium(pkg, name):
    params, surf, guide = npr.CASES[name](pkg)
    m = pkg.Medium(params)
    if guide:
        m.build_guide(16, 8)
    return m, surf


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _raw(pkg, m, scene, surf, max_bounces, d_rad, d_seg=None):
    """the C entry's return value"""
    s, f = np.array(scene, dtype=pkg.SCENE_S).reshape(()), np.array(surf, dtype=pkg.SURFACE_S).reshape(())
    return m.L.lib.gpis_render_scene_s_nee_paths(m.h, _vp(s), _vp(f), int(max_bounces), ctypes.c_void_p(d_rad.data_ptr()),
                                                 ctypes.c_void_p(d_seg.data_ptr()) if d_seg is not None else None, None)


def _accumulate(pkg, m, scenes, surf, max_bounces):
    """several driver calls into ONE pair of device buffers"""
    import torch
    h, w = int(scenes[0]["height"]), int(scenes[0]["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        m.L.check(_raw(pkg, m, s, surf, max_bounces, d_rad, d_seg), "gpis_render_scene_s_nee_paths")
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w), d_seg.cpu().numpy().view(np.uint32).reshape(h, w)


def test_library_exports_the_entry(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_render_scene_s_nee_paths$", out, flags=re.M)
    assert callable(getattr(pkg.Medium, "render_scene_s_nee_paths", None))


@pytest.mark.parametrize("name", npr.PIN_CASES)
def test_two_bounces_equal_the_single_interaction_driver(pkg, ob, name):
    """C2 has weight[0] == 1, so max_path_bounces = 2 is gpis_render_scene_s_nee on the same handle — and the composite."""
    import torch
    m, surf = _medium(pkg, name)
    scene = npr.frame(ob)
    img, segs = m.render_scene_s_nee_paths(scene, surf, 2, want_segs=True)
    d_rad = torch.zeros(npr.H * npr.W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m.call("gpis_render_scene_s_nee", np.array(scene, dtype=pkg.SCENE_S), np.array(surf, dtype=pkg.SURFACE_S), d_rad.data_ptr(), None)
    torch.cuda.synchronize()
    single = d_rad.cpu().numpy().reshape(npr.H, npr.W)
    m.close()
    assert single.any() and np.array_equal(_bits(img), _bits(single))
    want = npr.reference(pkg, ob, name, 2)
    _equal(img, segs, want.image, want.seg_count)


@pytest.mark.parametrize("name", sorted(npr.CASES))
def test_frame_equals_composite(pkg, ob, name):
    """max_path_bounces 1, 3, 4 and 6 on every medium and surface of nee_paths_ref.CASES."""
    m, surf = _medium(pkg, name)
    scene = npr.frame(ob)
    for max_bounces in npr.BOUNCES:
        want = npr.reference(pkg, ob, name, max_bounces)
        img, segs = m.render_scene_s_nee_paths(scene, surf, max_bounces, want_segs=True)
        print("%s, %d bounces: marched %s, hits %s, light %s, phase %s" % (name, max_bounces, want.marched, want.hits, want.light, want.phase))
        if max_bounces == 1:
            assert not want.image.any() and not want.seg_count.any()
        else:
            assert want.image.any() and len(want.hits) == max_bounces - 1 and want.hits[-1] > 0
        _equal(img, segs, want.image, want.seg_count)
    # without the counts
    assert np.array_equal(_bits(m.render_scene_s_nee_paths(scene, surf, npr.BOUNCES[-1])), _bits(want.image))
    m.close()


def test_fixture(pkg):
    """the device against the recorded composites: needs no oracle"""
    g = np.load(npr.GOLDEN)
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    for name in sorted(npr.CASES):
        m = pkg.Medium(np.array(g[name + "/params"]).view(pkg.PARAMS).reshape(()))
        if int(g[name + "/guide"]):
            m.build_guide(16, 8)
        surf = np.array(g[name + "/surface"]).view(pkg.SURFACE_S).reshape(())
        img, segs = m.render_scene_s_nee_paths(scene, surf, int(g["max_path_bounces"]), want_segs=True)
        m.close()
        assert g[name + "/image"].any()
        _equal(img, segs, g[name + "/image"], g[name + "/seg_count"])


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_frame_is_the_sum_of_its_parts(pkg, ob, kind):
    """Two row ranges and three shards of 4-pixel tile rows partition the pixels: the calls add up to the whole frame, bit for bit.
    The spp ranges {0} and {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2, which float32 does not make equal:
    there the counts equal the whole frame's and the image equals, bit for bit, the composite cut the same way."""
    m, surf = _medium(pkg, "mis")
    whole = npr.reference(pkg, ob, "mis", 4)
    scenes = npr.parts(ob, kind)
    img, segs = _accumulate(pkg, m, scenes, surf, 4)
    m.close()
    if kind != "spp":
        _equal(img, segs, whole.image, whole.seg_count)
    else:
        params, _, _ = npr.CASES["mis"](pkg)
        ref, orc, cut = npr.NeePathsRef(pkg, ob), ob.Oracle(params, threads=16), None
        for s in scenes:
            cut = ref.compose(orc, s, surf, 4, into=cut)
        assert np.array_equal(cut.seg_count, whole.seg_count)
        _equal(img, segs, cut.image, whole.seg_count)


def test_chunked_frame_equals_the_frame_in_one_chunk(pkg, ob):
    """96 x 96 x 8 = 73 728 samples in chunks of 2^16 against the same frame in one chunk, device against device."""
    m, surf = _medium(pkg, "mis")
    scene = ob.default_scene_s(96, 96, 8)
    one, one_segs = m.render_scene_s_nee_paths(scene, surf, 4, want_segs=True)
    m.set_option("chunk_log2", 16)
    got, got_segs = m.render_scene_s_nee_paths(scene, surf, 4, want_segs=True)
    m.close()
    assert one.any() and one_segs.sum() > 96 * 96 * 8
    _equal(got, got_segs, one, one_segs)


def test_tuning_options_change_nothing(pkg, ob):
    """the lane-per-ray kernels in place of the persistent march, and on a guided handle either form of the march"""
    for name, options in (("mis", (("persistent", 0),)), ("single", (("march_form", "resident"), ("march_form", "wave")))):
        m, surf = _medium(pkg, name)
        want = npr.reference(pkg, ob, name, 4)
        for key, value in options:
            m.set_option(key, value)
            img, segs = m.render_scene_s_nee_paths(npr.frame(ob), surf, 4, want_segs=True)
            _equal(img, segs, want.image, want.seg_count)
        m.close()


def test_degenerate_frames(pkg, ob):
    m, surf = _medium(pkg, "mis")
    # a camera that looks away from the bounding sphere: nothing is marched
    away = npr.frame(ob)
    away["cam_pos"] = (0.0, 0.0, -4.0)
    img, segs = m.render_scene_s_nee_paths(away, surf, 4, want_segs=True)
    assert not img.any() and not segs.any()
    # a wide field of view: some samples miss the bound, their neighbours do not
    wide = npr.frame(ob)
    wide["cam_fov_deg"] = 60.0
    params, _, _ = npr.CASES["mis"](pkg)
    want = npr.NeePathsRef(pkg, ob).compose(ob.Oracle(params, threads=16), wide, surf, 4)
    img, segs = m.render_scene_s_nee_paths(wide, surf, 4, want_segs=True)
    assert 0 < want.n_miss < want.n_samples
    _equal(img, segs, want.image, want.seg_count)
    # a black light: the shadow segments are marched all the same
    dark = np.array(surf, dtype=pkg.SURFACE_S)
    dark["cap_radiance"] = 0.0
    img, segs = m.render_scene_s_nee_paths(npr.frame(ob), dark, 4, want_segs=True)
    m.close()
    want = npr.reference(pkg, ob, "mis", 4)
    assert not img.any() and want.light[0] + want.phase[0] > 0 and np.array_equal(segs, want.seg_count)


def test_counters_see_every_segment(pkg, ob):
    m, surf = _medium(pkg, "mis")
    m.reset_counters()
    _, segs = m.render_scene_s_nee_paths(npr.frame(ob), surf, 4, want_segs=True)
    n_seg = m.counters()[1]
    m.close()
    assert n_seg == int(segs.sum()) == npr.reference(pkg, ob, "mis", 4).n_seg


def test_refusals(pkg, ob):
    import torch
    m, surf = _medium(pkg, "mis")
    scene = npr.frame(ob)
    d_rad = torch.zeros(npr.H * npr.W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert _raw(pkg, m, scene, surf, 0, d_rad) == -1 and "invalid argument" in m.L.last_error()
    bad = np.array(surf, dtype=pkg.SURFACE_S)
    bad["cap_cos"] = 1.0
    assert _raw(pkg, m, scene, bad, 4, d_rad) == -1
    rows = np.array(scene, dtype=pkg.SCENE_S)
    rows["y_begin"], rows["y_count"] = 10, npr.H
    assert _raw(pkg, m, rows, surf, 4, d_rad) == -1
    ws = pkg.WeightSpaceMedium(pkg.params_for_config("C1"))
    assert _raw(pkg, ws, scene, surf, 4, d_rad) == -1
    ws.close()
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any()
    m.close()
