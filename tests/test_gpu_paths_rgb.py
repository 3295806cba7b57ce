"""GPU parity of the RGB multi-bounce path driver with the medium's emission (gpis_render_scene_s_paths_rgb): image and per-pixel
segment counts BIT FOR BIT against the CPU composite (tests/paths_rgb_ref.py: the oracle's batch entries bounce level by bounce
level around the plain-C shade step), against gpis_render_scene_s_paths where the two estimators coincide, and against itself
under row ranges, shards, spp ranges, chunks and tuning options; the degenerate frames, the counters and the refusals.  No
tolerance on any device result: images are compared as uint32 views."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import paths_rgb_ref as prr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not prr.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(img, segs, want_img, want_segs):
    assert np.array_equal(segs, want_segs), np.argwhere(segs != want_segs)[:8]
    assert np.array_equal(_bits(img), _bits(want_img)), np.argwhere(_bits(img) != _bits(want_img))[:8]


def _medium(pkg, name, emission=True):
    params, albedo, guide = prr.CASES[name](pkg)
    m = pkg.Medium(params if emission else prr.without_emission(params))
    if guide:
        m.build_guide(*prr.GUIDE)
    return m, albedo


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _raw(pkg, m, scene, max_bounces, albedo, d_rad, d_seg=None):
    """the C entry's return value"""
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    alb = None if albedo is None else _vp(np.ascontiguousarray(albedo, dtype=np.float32))
    return m.L.lib.gpis_render_scene_s_paths_rgb(m.h, _vp(s), int(max_bounces), alb, ctypes.c_void_p(d_rad.data_ptr()) if d_rad is not None else None,
                                                 ctypes.c_void_p(d_seg.data_ptr()) if d_seg is not None else None, None)


def _accumulate(pkg, m, scenes, max_bounces, albedo):
    """several driver calls into ONE pair of device buffers"""
    import torch
    h, w = int(scenes[0]["height"]), int(scenes[0]["width"])
    d_rad = torch.zeros(3 * h * w, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        m.L.check(_raw(pkg, m, s, max_bounces, albedo, d_rad, d_seg), "gpis_render_scene_s_paths_rgb")
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w, 3), d_seg.cpu().numpy().view(np.uint32).reshape(h, w)


def test_library_exports_the_entry(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_render_scene_s_paths_rgb$", out, flags=re.M)
    assert callable(getattr(pkg.Medium, "render_scene_s_paths_rgb", None))


@pytest.mark.parametrize("name", sorted(prr.CASES))
def test_frame_equals_composite(pkg, ob, name):
    """max_path_bounces 1, 2 and 4 on every medium of paths_rgb_ref.CASES."""
    m, albedo = _medium(pkg, name)
    scene = prr.frame(ob)
    if name == "rust":
        # the fbm behind the emission first, at the composite's own hit points: a failure here names field_vec, not the driver
        c = prr.reference(pkg, ob, name, 4)
        pts = np.concatenate([lv.points[lv.hit.astype(bool)] for lv in c.levels])
        want_e = np.concatenate([lv.e[lv.hit.astype(bool)] for lv in c.levels])
        col, emi = m.mean_color_emission(pts)
        col_o, emi_o = ob.Oracle(prr.CASES[name](pkg)[0], threads=16).mean_color_emission(pts)
        assert len(pts) > 1000 and np.array_equal(_bits(emi_o), _bits(want_e))
        assert np.array_equal(_bits(emi), _bits(emi_o)), "field_vec: emission differs on %d of %d hit points" % ((emi != emi_o).any(axis=1).sum(), len(pts))
        assert np.array_equal(_bits(col), _bits(col_o)), "field_vec: colour differs on %d of %d hit points" % ((col != col_o).any(axis=1).sum(), len(pts))
    E = name in prr.EMISSIVE_CASES
    for max_bounces in prr.BOUNCES:
        want = prr.reference(pkg, ob, name, max_bounces)
        img, segs = m.render_scene_s_paths_rgb(scene, max_bounces, albedo, want_segs=True)
        print("%s, %d bounces: marched %s, hits %s, shadow %s" % (name, max_bounces, want.marched, want.hits, want.shadow))
        assert img.shape == (prr.H, prr.W, 3) and img.dtype == np.float32 and segs.dtype == np.uint32
        if max_bounces == 1 and not E:
            assert not want.image.any() and not want.seg_count.any()
        else:
            assert want.image.any() and want.hits[-1] > 0
        _equal(img, segs, want.image, want.seg_count)
    # without the counts
    assert np.array_equal(_bits(m.render_scene_s_paths_rgb(scene, prr.BOUNCES[-1], albedo)), _bits(want.image))
    m.close()


@pytest.mark.parametrize("name", prr.PIN_CASES)
def test_channel_0_is_the_mono_driver(pkg, ob, name):
    """without emission and with albedo[0] == albedo, channel 0 is gpis_render_scene_s_paths on the same handle, bit for bit"""
    import torch
    m, albedo = _medium(pkg, name, emission=False)
    scene = prr.frame(ob)
    for max_bounces in prr.BOUNCES:
        img = m.render_scene_s_paths_rgb(scene, max_bounces, albedo)
        d_rad = torch.zeros(prr.H * prr.W, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.call("gpis_render_scene_s_paths", np.array(scene, dtype=pkg.SCENE_S), max_bounces, float(np.float32(albedo[0])), d_rad.data_ptr(), None)
        torch.cuda.synchronize()
        mono = d_rad.cpu().numpy().reshape(prr.H, prr.W)
        assert mono.any() == (max_bounces > 1)
        assert np.array_equal(_bits(img[:, :, 0]), _bits(mono))
        assert np.array_equal(_bits(img), _bits(prr.reference(pkg, ob, name, max_bounces, emission=False).image))
    # a scalar albedo is broadcast
    m2, _ = _medium(pkg, "grey")
    assert np.array_equal(_bits(m2.render_scene_s_paths_rgb(scene, 4, 0.8)), _bits(prr.reference(pkg, ob, "grey", 4).image))
    m2.close()
    m.close()


def test_fixture(pkg):
    """the device against the recorded composites: needs no oracle"""
    g = np.load(prr.GOLDEN)
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    for name in sorted(prr.CASES):
        m = pkg.Medium(np.array(g[name + "/params"]).view(pkg.PARAMS).reshape(()))
        if int(g[name + "/guide"]):
            m.build_guide(*prr.GUIDE)
        img, segs = m.render_scene_s_paths_rgb(scene, int(g["max_path_bounces"]), g[name + "/albedo"], want_segs=True)
        m.close()
        assert g[name + "/image"].any()
        _equal(img, segs, g[name + "/image"], g[name + "/seg_count"])


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_frame_is_the_sum_of_its_parts(pkg, ob, kind):
    """Two row ranges and three shards of 4-pixel tile rows partition the pixels: the calls add up to the whole frame, bit for bit.
    The spp ranges {0} and {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2, which float32 does not make equal:
    there the counts equal the whole frame's and the image equals, bit for bit, the composite cut the same way."""
    name = "c1-emission"
    m, albedo = _medium(pkg, name)
    whole = prr.reference(pkg, ob, name, 4)
    scenes = prr.parts(ob, kind)
    img, segs = _accumulate(pkg, m, scenes, 4, albedo)
    m.close()
    if kind != "spp":
        _equal(img, segs, whole.image, whole.seg_count)
    else:
        ref, orc, cut = prr.PathsRgbRef(pkg, ob), ob.Oracle(prr.CASES[name](pkg)[0], threads=16), None
        for s in scenes:
            cut = ref.compose(orc, s, 4, albedo, into=cut)
        assert np.array_equal(cut.seg_count, whole.seg_count)
        _equal(img, segs, cut.image, whole.seg_count)


def test_chunked_frame_equals_the_frame_in_one_chunk(pkg, ob):
    """96 x 96 x 8 = 73 728 samples in chunks of 2^16 against the same frame in one chunk, device against device."""
    m, albedo = _medium(pkg, "c1-emission")
    scene = ob.default_scene_s(96, 96, 8)
    one, one_segs = m.render_scene_s_paths_rgb(scene, 4, albedo, want_segs=True)
    m.set_option("chunk_log2", 16)
    got, got_segs = m.render_scene_s_paths_rgb(scene, 4, albedo, want_segs=True)
    m.close()
    assert one.any() and one_segs.sum() > 96 * 96 * 8
    _equal(got, got_segs, one, one_segs)


@pytest.mark.parametrize("name", ["c1-emission", "sigma", "ramp", "rust"])
def test_tuning_options_change_nothing(pkg, ob, name):
    """Regrouping of the secondary segments on and off, before the wavefront march or not, either form of the march on the guided
    handles, and the lane-per-ray kernels in place of the persistent march on the per-path medium: the same bits and counts."""
    m, albedo = _medium(pkg, name)
    want = prr.reference(pkg, ob, name, 4)
    guided = prr.CASES[name](pkg)[2]
    forms = ("resident", "wave") if guided else (None,)
    for form in forms:
        if form:
            m.set_option("march_form", form)
        for sort, presort in ((1, 1), (1, 0), (0, 1), (0, 0)):
            m.set_option("paths_sort", sort)
            m.set_option("paths_presort", presort)
            img, segs = m.render_scene_s_paths_rgb(prr.frame(ob), 4, albedo, want_segs=True)
            _equal(img, segs, want.image, want.seg_count)
    if name == "rust":
        m.set_option("paths_sort", 1)
        m.set_option("paths_presort", 1)
        for persistent in (0, 1):
            m.set_option("persistent", persistent)
            img, segs = m.render_scene_s_paths_rgb(prr.frame(ob), 4, albedo, want_segs=True)
            _equal(img, segs, want.image, want.seg_count)
    m.close()


def test_degenerate_frames(pkg, ob):
    name = "ramp"
    m, albedo = _medium(pkg, name)
    # a camera that looks away from the bounding sphere: nothing is marched
    away = prr.frame(ob)
    away["cam_pos"] = (0.0, 0.0, -4.0)
    img, segs = m.render_scene_s_paths_rgb(away, 4, albedo, want_segs=True)
    assert not img.any() and not segs.any()
    # a wide field of view: some samples miss the bound, their neighbours do not
    wide = prr.frame(ob)
    wide["cam_fov_deg"] = 60.0
    want = prr.PathsRgbRef(pkg, ob).compose(ob.Oracle(prr.CASES[name](pkg)[0], threads=16), wide, 4, albedo)
    img, segs = m.render_scene_s_paths_rgb(wide, 4, albedo, want_segs=True)
    m.close()
    assert 0 < want.n_miss < want.n_samples
    _equal(img, segs, want.image, want.seg_count)


@pytest.mark.parametrize("name", ["c1-emission", "sigma"])
def test_counters_see_every_segment(pkg, ob, name):
    m, albedo = _medium(pkg, name)
    m.reset_counters()
    _, segs = m.render_scene_s_paths_rgb(prr.frame(ob), 4, albedo, want_segs=True)
    n_seg = m.counters()[1]
    m.close()
    assert n_seg == int(segs.sum()) == prr.reference(pkg, ob, name, 4).n_seg


def test_refusals(pkg, ob):
    import torch
    m, albedo = _medium(pkg, "ramp")
    scene = prr.frame(ob)
    d_rad = torch.zeros(3 * prr.H * prr.W, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(prr.H * prr.W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for bad_bounces in (0, -3):
        assert _raw(pkg, m, scene, bad_bounces, albedo, d_rad, d_seg) == -1
        assert "invalid argument" in m.L.last_error() and "max_path_bounces >= 1" in m.L.last_error()
    assert _raw(pkg, m, scene, 4, None, d_rad, d_seg) == -1 and "albedo" in m.L.last_error()
    assert _raw(pkg, m, scene, 4, albedo, None, d_seg) == -1 and "radiance_sum3" in m.L.last_error()
    rows = np.array(scene, dtype=pkg.SCENE_S)
    rows["y_begin"], rows["y_count"] = 10, prr.H
    assert _raw(pkg, m, rows, 4, albedo, d_rad, d_seg) == -1 and "scene_args_ok" in m.L.last_error()
    shard = np.array(scene, dtype=pkg.SCENE_S)
    shard["shard_index"], shard["shard_count"] = 2, 2
    assert _raw(pkg, m, shard, 4, albedo, d_rad, d_seg) == -1 and "scene_args_ok" in m.L.last_error()
    ws = pkg.WeightSpaceMedium(pkg.params_for_config("C1"))
    assert _raw(pkg, ws, scene, 4, albedo, d_rad, d_seg) == -1 and "std_handle" in m.L.last_error()
    ws.close()
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any() and not d_seg.cpu().numpy().any()
    m.close()
