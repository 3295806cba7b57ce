"""GPU parity of the RGB conductor NEE / MIS path driver (gpis_render_scene_s_nee_paths_rgb): image (H, W, 3) and per-pixel segment
counts BIT FOR BIT against the CPU composite (tests/nee_paths_rgb_ref.py: the oracle's batch entries bounce level by bounce level
around the plain-C shade step), against gpis_render_scene_s_nee_paths where colour cannot matter, and against itself under row
ranges, shards, spp ranges, chunks and tuning options; the degenerate frames, the counters and the refusals.  No tolerance on any
device result: images are compared as uint32 views."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import nee_paths_ref as npr
import nee_paths_rgb_ref as rgb

pytestmark = pytest.mark.gpu

ENTRY = "gpis_render_scene_s_nee_paths_rgb"


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not rgb.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(img, segs, want_img, want_segs):
    assert img.shape == want_img.shape
    assert np.array_equal(segs, want_segs), np.argwhere(segs != want_segs)[:8]
    assert np.array_equal(_bits(img), _bits(want_img)), np.argwhere(_bits(img) != _bits(want_img))[:8]


def _medium(pkg, name, emission=True):
    params, surf = rgb.CASES[name](pkg)
    return pkg.Medium(params if emission else rgb.without_emission(params)), surf


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _raw(pkg, m, scene, surf, max_bounces, d_rad, d_seg=None):
    """the C entry's return value"""
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    f = None if surf is None else np.array(surf, dtype=pkg.SURFACE_RGB_S).reshape(())
    return getattr(m.L.lib, ENTRY)(m.h, _vp(s), _vp(f), int(max_bounces), ctypes.c_void_p(d_rad.data_ptr()) if d_rad is not None else None,
                                   ctypes.c_void_p(d_seg.data_ptr()) if d_seg is not None else None, None)


def _accumulate(pkg, m, scenes, surf, max_bounces):
    """several driver calls into ONE pair of device buffers"""
    import torch
    h, w = int(scenes[0]["height"]), int(scenes[0]["width"])
    d_rad = torch.zeros(3 * h * w, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        m.L.check(_raw(pkg, m, s, surf, max_bounces, d_rad, d_seg), ENTRY)
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w, 3), d_seg.cpu().numpy().view(np.uint32).reshape(h, w)


def test_library_exports_the_entries(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for name in ("gpis_render_scene_s_nee_paths_rgb", "gpis_render_scene_s_nee_paths_rgb_adaptive", "gpis_default_surface_rgb"):
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    assert callable(getattr(pkg.Medium, "render_scene_s_nee_paths_rgb", None))
    assert callable(getattr(pkg.Medium, "render_scene_s_nee_paths_rgb_adaptive", None))
    s = np.zeros((), dtype=pkg.SURFACE_RGB_S)
    pkg.load_library().lib.gpis_default_surface_rgb(_vp(s))
    assert pkg.SURFACE_RGB_S.itemsize == 64 and s.tobytes() == pkg.default_surface_rgb().tobytes()
    assert float(s["cap_cos"]) == float(pkg.default_surface_s()["cap_cos"])


@pytest.mark.parametrize("name", sorted(rgb.CASES))
def test_frame_equals_composite(pkg, ob, name):
    """max_path_bounces 1, 2 and 4 on every case of nee_paths_rgb_ref.CASES, the emissive medium (first-hit emission at 1) included"""
    m, surf = _medium(pkg, name)
    scene = rgb.frame(ob)
    for max_bounces in rgb.BOUNCES:
        want = rgb.reference(pkg, ob, name, max_bounces)
        img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, max_bounces, want_segs=True)
        print("%s, %d bounces: marched %s, hits %s, light %s, phase %s" % (name, max_bounces, want.marched, want.hits, want.light, want.phase))
        if max_bounces == 1 and name != rgb.EMISSIVE_CASE:
            assert not want.image.any() and not want.seg_count.any()
        else:
            assert want.image.any() and want.seg_count.any()
        _equal(img, segs, want.image, want.seg_count)
    # without the counts
    assert np.array_equal(_bits(m.render_scene_s_nee_paths_rgb(scene, surf, rgb.BOUNCES[-1])), _bits(want.image))
    m.close()


@pytest.mark.parametrize("name", rgb.GREY_CASES)
def test_equal_channels_equal_the_mono_entry(pkg, ob, name):
    m, surf = _medium(pkg, name)
    mono = npr._surface(pkg, cap_cos=float(surf["cap_cos"]))
    scene = rgb.frame(ob)
    want, want_segs = m.render_scene_s_nee_paths(scene, mono, 4, want_segs=True)
    img, segs = m.render_scene_s_nee_paths_rgb(scene, rgb.grey_surface(pkg, mono), 4, want_segs=True)
    m.close()
    assert want.any()
    for c in range(3):
        _equal(img[..., c], segs, want, want_segs)


@pytest.mark.parametrize("name", rgb.GREY_CASES)
def test_copper_channel_equals_the_mono_entry_of_its_surface(pkg, ob, name):
    m, surf = _medium(pkg, name)
    scene = rgb.frame(ob)
    img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, 4, want_segs=True)
    for c in range(3):
        want, want_segs = m.render_scene_s_nee_paths(scene, rgb.channel_surface(pkg, surf, c), 4, want_segs=True)
        assert want.any()
        _equal(img[..., c], segs, want, want_segs)
    m.close()
    assert not np.array_equal(img[..., 0], img[..., 1]) and not np.array_equal(img[..., 1], img[..., 2])


def test_emissive_medium_without_its_emission_and_channel_0(pkg, ob):
    """the colour medium with mean_emission switched off against its composite; with a grey surface channel 0 (weight[0]) is the
    mono entry's, and without the emission max_path_bounces = 1 adds zeros and marches nothing"""
    m, surf = _medium(pkg, rgb.EMISSIVE_CASE, emission=False)
    scene = rgb.frame(ob)
    want = rgb.reference(pkg, ob, rgb.EMISSIVE_CASE, 4, emission=False)
    img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, 4, want_segs=True)
    _equal(img, segs, want.image, want.seg_count)
    mono = npr._surface(pkg)
    want, want_segs = m.render_scene_s_nee_paths(scene, mono, 4, want_segs=True)
    img, segs = m.render_scene_s_nee_paths_rgb(scene, rgb.grey_surface(pkg, mono), 4, want_segs=True)
    _equal(img[..., 0], segs, want, want_segs)
    assert not np.array_equal(img[..., 0], img[..., 1])
    img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, 1, want_segs=True)
    m.close()
    assert not img.any() and not segs.any()


def test_fixture(pkg):
    """the device against the recorded composites: needs no oracle"""
    g = np.load(rgb.GOLDEN)
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    for name in sorted(rgb.CASES):
        m = pkg.Medium(np.array(g[name + "/params"]).view(pkg.PARAMS).reshape(()))
        surf = np.array(g[name + "/surface"]).view(pkg.SURFACE_RGB_S).reshape(())
        img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, int(g["max_path_bounces"]), want_segs=True)
        assert g[name + "/image"].any()
        _equal(img, segs, g[name + "/image"], g[name + "/seg_count"])
        if name == rgb.EMISSIVE_CASE:
            img, segs = m.render_scene_s_nee_paths_rgb(scene, surf, 1, want_segs=True)
            assert g["first_hit/image"].any() and int(g["first_hit/seg_count"].max()) == rgb.SPP
            _equal(img, segs, g["first_hit/image"], g["first_hit/seg_count"])
        m.close()


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_frame_is_the_sum_of_its_parts(pkg, ob, kind):
    """Two row ranges and two shards of 4-pixel tile rows partition the pixels: the calls add up to the whole frame, bit for bit.
    The spp ranges {0} and {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2, which float32 does not make equal:
    there the counts equal the whole frame's and the image equals, bit for bit, the composite cut the same way."""
    name = rgb.EMISSIVE_CASE
    m, surf = _medium(pkg, name)
    whole = rgb.reference(pkg, ob, name, 4)
    scenes = rgb.parts(ob, kind)
    img, segs = _accumulate(pkg, m, scenes, surf, 4)
    m.close()
    if kind != "spp":
        _equal(img, segs, whole.image, whole.seg_count)
    else:
        params, _ = rgb.CASES[name](pkg)
        ref, orc, cut = rgb.NeePathsRgbRef(pkg, ob), ob.Oracle(params, threads=16), None
        for s in scenes:
            cut = ref.compose(orc, s, surf, 4, into=cut)
        assert np.array_equal(cut.seg_count, whole.seg_count)
        _equal(img, segs, cut.image, whole.seg_count)


def test_chunked_frame_equals_the_frame_in_one_chunk(pkg, ob):
    """990 samples in chunks of 2^8 (85 pixels: four chunks, the last one short, the colour planes 255 floats apart) against the
    composite, which is the frame in one chunk"""
    name = rgb.EMISSIVE_CASE
    m, surf = _medium(pkg, name)
    want = rgb.reference(pkg, ob, name, 4)
    m.set_option("chunk_log2", 8)
    got, got_segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), surf, 4, want_segs=True)
    m.close()
    _equal(got, got_segs, want.image, want.seg_count)


def test_tuning_options_change_nothing(pkg, ob):
    """the lane-per-ray kernels in place of the persistent march, and on a guided handle either form of the march"""
    m, surf = _medium(pkg, "mis")
    want = rgb.reference(pkg, ob, "mis", 4)
    m.set_option("persistent", 0)
    img, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), surf, 4, want_segs=True)
    m.close()
    _equal(img, segs, want.image, want.seg_count)
    # nee_paths_ref's single-realization medium on the guided kernels
    params, mono, guide = npr.CASES["single"](pkg)
    assert guide
    m = pkg.Medium(params)
    m.build_guide(16, 8)
    surf = rgb.copper(pkg, cap_cos=float(mono["cap_cos"]))
    want = None
    for form in ("auto", "resident", "wave"):
        m.set_option("march_form", form)
        img, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), surf, 4, want_segs=True)
        if want is None:
            want = (img, segs)
            assert img.any()
        _equal(img, segs, *want)
    m.close()


def test_degenerate_frames(pkg, ob):
    m, surf = _medium(pkg, "mis")
    # a camera that looks away from the bounding sphere: nothing is marched
    away = rgb.frame(ob)
    away["cam_pos"] = (0.0, 0.0, -4.0)
    img, segs = m.render_scene_s_nee_paths_rgb(away, surf, 4, want_segs=True)
    assert img.shape == (rgb.H, rgb.W, 3) and not img.any() and not segs.any()
    # a wide field of view: some samples miss the bound, their neighbours do not
    wide = rgb.frame(ob)
    wide["cam_fov_deg"] = 60.0
    params, _ = rgb.CASES["mis"](pkg)
    want = rgb.NeePathsRgbRef(pkg, ob).compose(ob.Oracle(params, threads=16), wide, surf, 4)
    img, segs = m.render_scene_s_nee_paths_rgb(wide, surf, 4, want_segs=True)
    assert 0 < want.n_miss < want.n_samples
    _equal(img, segs, want.image, want.seg_count)
    # a black light: the shadow segments are marched all the same, as the mono entry marches them
    full = rgb.reference(pkg, ob, "mis", 4)
    img, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), rgb.copper(pkg, cap_radiance=(0.0, 0.0, 0.0)), 4, want_segs=True)
    dark = npr._surface(pkg, cap_radiance=0.0)
    _, mono_segs = m.render_scene_s_nee_paths(rgb.frame(ob), dark, 4, want_segs=True)
    assert not img.any() and full.light[0] + full.phase[0] > 0 and np.array_equal(segs, full.seg_count) and np.array_equal(segs, mono_segs)
    # a light that is black in two channels
    img, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), rgb.copper(pkg, cap_radiance=(0.0, 15.0, 0.0)), 4, want_segs=True)
    m.close()
    assert np.array_equal(segs, full.seg_count) and not img[..., 0].any() and not img[..., 2].any()
    assert np.array_equal(_bits(img[..., 1]), _bits(full.image[..., 1]))


def test_zero_channels(pkg, ob):
    """albedo zero everywhere ends every path at its first hit without a shadow segment; albedo zero in two channels marches what the
    full surface marches"""
    m, _ = _medium(pkg, "nee")
    for albedo in ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
        surf = rgb.copper(pkg, albedo=albedo)
        want = rgb.reference(pkg, ob, "nee", 4, surface=surf)
        img, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), surf, 4, want_segs=True)
        _equal(img, segs, want.image, want.seg_count)
    m.close()


def test_counters_see_every_segment(pkg, ob):
    m, surf = _medium(pkg, rgb.EMISSIVE_CASE)
    m.reset_counters()
    _, segs = m.render_scene_s_nee_paths_rgb(rgb.frame(ob), surf, 4, want_segs=True)
    n_seg = m.counters()[1]
    m.close()
    assert n_seg == int(segs.sum()) == rgb.reference(pkg, ob, rgb.EMISSIVE_CASE, 4).n_seg


def test_refusals(pkg, ob):
    import torch
    m, surf = _medium(pkg, "mis")
    scene = rgb.frame(ob)
    d_rad = torch.zeros(3 * rgb.H * rgb.W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert _raw(pkg, m, scene, surf, 0, d_rad) == -1 and "invalid argument" in m.L.last_error()
    assert _raw(pkg, m, scene, None, 4, d_rad) == -1
    assert _raw(pkg, m, scene, surf, 4, None) == -1
    for cap_cos in (1.0, -1.0, 1.5):
        assert _raw(pkg, m, scene, rgb.copper(pkg, cap_cos=cap_cos), 4, d_rad) == -1
    rows = np.array(scene, dtype=pkg.SCENE_S)
    rows["y_begin"], rows["y_count"] = 10, rgb.H
    assert _raw(pkg, m, rows, surf, 4, d_rad) == -1
    shard = np.array(scene, dtype=pkg.SCENE_S)
    shard["shard_index"], shard["shard_count"] = 2, 2
    assert _raw(pkg, m, shard, surf, 4, d_rad) == -1
    ws = pkg.WeightSpaceMedium(pkg.params_for_config("C1"))
    assert _raw(pkg, ws, scene, surf, 4, d_rad) == -1
    ws.close()
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any()
    assert _raw(pkg, m, scene, surf, 4, d_rad) == 0
    torch.cuda.synchronize()
    assert d_rad.cpu().numpy().any()
    m.close()
