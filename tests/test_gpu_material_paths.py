"""GPU parity of the RGB path driver whose material is chosen per hit by the GP id (gpis_render_scene_s_material_paths_rgb and its
adaptive form): image (H, W, 3) and per-pixel segment counts BIT FOR BIT against the CPU composite (tests/material_paths_ref.py: the
oracle's batch entries bounce level by bounce level around the plain-C step of both materials) on media whose hits carry both ids,
against gpis_render_scene_s_nee_paths_rgb where the materials cannot matter, and against itself under row ranges, shards, spp
ranges, chunks and tuning options; the degenerate frames, the counters and the refusals; the adaptive entry against the schedule
over per-sample calls of the uniform one.  No tolerance on any device result: images are compared as uint32 views."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import adaptive_paths_rgb_ref as apr
import adaptive_ref as ar
import material_paths_ref as mp
import nee_paths_rgb_ref as rgb
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

ENTRY = "gpis_render_scene_s_material_paths_rgb"
ADAPTIVE = ENTRY + "_adaptive"


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not mp.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(img, segs, want_img, want_segs):
    assert img.shape == want_img.shape
    assert np.array_equal(segs, want_segs), np.argwhere(segs != want_segs)[:8]
    assert np.array_equal(_bits(img), _bits(want_img)), np.argwhere(_bits(img) != _bits(want_img))[:8]


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _raw(pkg, m, scene, mats, max_bounces, d_rad, d_seg=None):
    """the C entry's return value"""
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    t = None if mats is None else np.array(mats, dtype=pkg.MATERIALS_S).reshape(())
    return getattr(m.L.lib, ENTRY)(m.h, _vp(s), _vp(t), int(max_bounces), ctypes.c_void_p(d_rad.data_ptr()) if d_rad is not None else None,
                                   ctypes.c_void_p(d_seg.data_ptr()) if d_seg is not None else None, None)


def _accumulate(pkg, m, scenes, mats, max_bounces):
    """several driver calls into ONE pair of device buffers"""
    import torch
    h, w = int(scenes[0]["height"]), int(scenes[0]["width"])
    d_rad = torch.zeros(3 * h * w, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        m.L.check(_raw(pkg, m, s, mats, max_bounces, d_rad, d_seg), ENTRY)
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w, 3), d_seg.cpu().numpy().view(np.uint32).reshape(h, w)


def test_library_exports_the_entries(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for name in (ENTRY, ADAPTIVE, "gpis_default_materials"):
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    assert callable(getattr(pkg.Medium, "render_scene_s_material_paths_rgb", None))
    assert callable(getattr(pkg.Medium, "render_scene_s_material_paths_rgb_adaptive", None))
    t = np.zeros(1, dtype=pkg.MATERIALS_S)
    t.view(np.uint8)[:] = 0xAB                  # the entry sets every byte
    pkg.load_library().lib.gpis_default_materials(_vp(t))
    assert pkg.MATERIALS_S.itemsize == 224 and t.tobytes() == pkg.default_materials().tobytes()


@pytest.mark.parametrize("name", sorted(mp.CASES))
def test_frame_equals_composite(pkg, ob, name):
    """max_path_bounces 1, 3 and 4 on every case of material_paths_ref.CASES: C2 made CSG under the three schemes and the three
    tables, C1 made CSG on the guided kernels, the emissive colour medium made CSG (first-hit emission at 1), and the
    surf_vol_phase_separate medium.  The composite of every case sees both ids at the first bounce."""
    m = mp.medium(pkg, name)
    mats = mp.CASES[name](pkg)[1]
    scene = mp.frame(ob)
    for max_bounces in mp.BOUNCES:
        want = mp.reference(pkg, ob, name, max_bounces)
        img, segs = m.render_scene_s_material_paths_rgb(scene, mats, max_bounces, want_segs=True)
        print("%s, %d bounces: marched %s, hits %s, ids %s, light %s, phase %s" % (name, max_bounces, want.marched, want.hits, want.ids, want.light, want.phase))
        if max_bounces == 1 and name != mp.EMISSIVE_CASE:
            assert not want.image.any() and not want.seg_count.any()
        else:
            assert want.image.any() and want.seg_count.any()
            assert max_bounces == 1 or (want.ids[0][0] >= 100 and want.ids[0][1] >= 100)
        _equal(img, segs, want.image, want.seg_count)
    # without the counts
    assert np.array_equal(_bits(m.render_scene_s_material_paths_rgb(scene, mats, mp.BOUNCES[-1])), _bits(want.image))
    m.close()


@pytest.mark.parametrize("name", ["mis/cu-la", "nee/cu-la", "uni/cu-la", "single/cu-la", mp.EMISSIVE_CASE])
def test_equal_conductors_equal_the_conductor_entry(pkg, ob, name):
    """GPU against GPU: a table whose entries all are one conductor gives gpis_render_scene_s_nee_paths_rgb's frame, on media whose
    hits carry both ids"""
    m = mp.medium(pkg, name)
    surf = rgb.copper(pkg, cap_cos=float(mp.CASES[name](pkg)[1]["cap_cos"]))
    scene = mp.frame(ob)
    want, want_segs = m.render_scene_s_nee_paths_rgb(scene, surf, 4, want_segs=True)
    assert want.any()
    for n in (1, 2, 4):
        img, segs = m.render_scene_s_material_paths_rgb(scene, mp.table_of_surface(pkg, surf, n), 4, want_segs=True)
        _equal(img, segs, want, want_segs)
    m.close()


def test_one_material_equals_the_padded_table_where_every_id_is_0(pkg, ob):
    """GPU against GPU on media without a second mean: n_materials = 1 against the table padded with other materials; and on the
    CSG medium an id beyond the table takes material[0]"""
    for name in sorted(mp.PLAIN_CASES):
        params, surf = mp.PLAIN_CASES[name](pkg)
        m = pkg.Medium(params)
        for first in (mp.conductor(pkg, surf["eta"], surf["k"], surf["albedo"]), mp.lambert(pkg)):
            kw = {"cap_cos": float(surf["cap_cos"]), "cap_radiance": surf["cap_radiance"]}
            one = mp.table(pkg, [first], **kw)
            padded = mp.table(pkg, [first, mp.lambert(pkg, (0.1, 0.2, 0.3)), mp.conductor(pkg, albedo=(0.5, 0.5, 0.5)), mp.lambert(pkg)], **kw)
            want, want_segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), one, 4, want_segs=True)
            img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), padded, 4, want_segs=True)
            assert want.any()
            _equal(img, segs, want, want_segs)
        m.close()
    m = mp.medium(pkg, "mis/cu-la")
    la = mp.lambert(pkg)
    want = mp.reference(pkg, ob, "mis/cu-la", 4, mats=mp.table(pkg, [la, la]))
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mp.table(pkg, [la]), 4, want_segs=True)
    m.close()
    _equal(img, segs, want.image, want.seg_count)


def test_fixture(pkg):
    """the device against the recorded composites: needs no oracle"""
    g = np.load(mp.GOLDEN)
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    for name in sorted(mp.CASES):
        m = pkg.Medium(np.array(g[name + "/params"]).view(pkg.PARAMS).reshape(()))
        if name in mp.GRID_CASES:
            m.set_variance_grid(g["grid/voxels"], g["grid/world_to_index"], "linear")
        if int(g[name + "/guide"]):
            m.build_guide(16, 8)
        mats = np.array(g[name + "/materials"]).view(pkg.MATERIALS_S).reshape(())
        img, segs = m.render_scene_s_material_paths_rgb(scene, mats, int(g["max_path_bounces"]), want_segs=True)
        assert g[name + "/image"].any()
        _equal(img, segs, g[name + "/image"], g[name + "/seg_count"])
        if name == mp.EMISSIVE_CASE:
            img, segs = m.render_scene_s_material_paths_rgb(scene, mats, 1, want_segs=True)
            assert g["first_hit/image"].any() and int(g["first_hit/seg_count"].max()) == mp.SPP
            _equal(img, segs, g["first_hit/image"], g["first_hit/seg_count"])
        m.close()


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_frame_is_the_sum_of_its_parts(pkg, ob, kind):
    """Two row ranges and three shards of 4-pixel tile rows partition the pixels: the calls add up to the whole frame, bit for bit.
    The spp ranges {0} and {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2, which float32 does not make equal:
    there the counts equal the whole frame's and the image equals, bit for bit, the composite cut the same way."""
    name = mp.EMISSIVE_CASE
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    whole = mp.reference(pkg, ob, name, 4)
    scenes = mp.parts(ob, kind)
    img, segs = _accumulate(pkg, m, scenes, mats, 4)
    m.close()
    if kind != "spp":
        _equal(img, segs, whole.image, whole.seg_count)
    else:
        ref, orc, cut = mp.MaterialPathsRef(pkg, ob), mp.oracle(pkg, ob, name), None
        for s in scenes:
            cut = ref.compose(orc, s, mats, 4, into=cut)
        assert np.array_equal(cut.seg_count, whole.seg_count)
        _equal(img, segs, cut.image, whole.seg_count)


def test_chunked_frame_equals_the_frame_in_one_chunk(pkg, ob):
    """1440 samples in chunks of 2^8 (85 pixels: six chunks, the last one short, the colour planes 255 floats apart) against the
    composite, which is the frame in one chunk"""
    name = mp.EMISSIVE_CASE
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    want = mp.reference(pkg, ob, name, 4)
    m.set_option("chunk_log2", 8)
    got, got_segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 4, want_segs=True)
    m.close()
    _equal(got, got_segs, want.image, want.seg_count)


def test_tuning_options_change_nothing(pkg, ob):
    """the lane-per-ray kernels in place of the persistent march, and on the guided handle either form of the march"""
    name = "mis/cu-la"
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    want = mp.reference(pkg, ob, name, 4)
    m.set_option("persistent", 0)
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 4, want_segs=True)
    m.close()
    _equal(img, segs, want.image, want.seg_count)
    name = "single/cu-la"
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    want = mp.reference(pkg, ob, name, 4)
    for form in ("auto", "resident", "wave"):
        m.set_option("march_form", form)
        img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 4, want_segs=True)
        _equal(img, segs, want.image, want.seg_count)
    m.close()


def test_one_bounce_with_and_without_emission(pkg, ob):
    """max_path_bounces = 1: first-hit emission on the emissive medium; without the emission zeros, and nothing marched"""
    name = mp.EMISSIVE_CASE
    params, mats, _ = mp.CASES[name](pkg)
    want = mp.reference(pkg, ob, name, 1)
    m = pkg.Medium(params)
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 1, want_segs=True)
    m.close()
    assert want.image.any() and int(want.seg_count.max()) == mp.SPP
    _equal(img, segs, want.image, want.seg_count)
    m = pkg.Medium(rgb.without_emission(params))
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 1, want_segs=True)
    m.close()
    assert img.shape == (mp.H, mp.W, 3) and not img.any() and not segs.any()


def test_degenerate_frames(pkg, ob):
    name = "mis/la-cu"
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    # a camera that looks away from the bounding sphere: nothing is marched
    away = mp.frame(ob)
    away["cam_pos"] = (0.0, 0.0, -4.0)
    img, segs = m.render_scene_s_material_paths_rgb(away, mats, 4, want_segs=True)
    assert img.shape == (mp.H, mp.W, 3) and not img.any() and not segs.any()
    # a wide field of view: some samples miss the bound, their neighbours do not
    wide = mp.frame(ob)
    wide["cam_fov_deg"] = 60.0
    want = mp.MaterialPathsRef(pkg, ob).compose(mp.oracle(pkg, ob, name), wide, mats, 4)
    img, segs = m.render_scene_s_material_paths_rgb(wide, mats, 4, want_segs=True)
    assert 0 < want.n_miss < want.n_samples
    _equal(img, segs, want.image, want.seg_count)
    # a black light: the shadow segments are marched all the same; black in two channels: the third is the full light's
    full = mp.reference(pkg, ob, name, 4)
    dark = np.array(mats).copy()
    dark["cap_radiance"] = 0.0
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), dark, 4, want_segs=True)
    assert not img.any() and full.light[0] + full.phase[0] > 0 and np.array_equal(segs, full.seg_count)
    dark["cap_radiance"] = (0.0, 15.0, 0.0)
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), dark, 4, want_segs=True)
    assert np.array_equal(segs, full.seg_count) and not img[..., 0].any() and not img[..., 2].any()
    assert np.array_equal(_bits(img[..., 1]), _bits(full.image[..., 1]))
    # a black Lambert material: no light segment and no bounce at its hits
    black = mp.table(pkg, [mp.lambert(pkg, (0.0, 0.0, 0.0)), mp.conductor(pkg)])
    want = mp.reference(pkg, ob, name, 4, mats=black)
    img, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), black, 4, want_segs=True)
    m.close()
    assert want.image.any() and int(want.seg_count.sum()) < full.n_seg
    _equal(img, segs, want.image, want.seg_count)


def test_counters_see_every_segment(pkg, ob):
    name = mp.EMISSIVE_CASE
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    m.reset_counters()
    _, segs = m.render_scene_s_material_paths_rgb(mp.frame(ob), mats, 4, want_segs=True)
    n_seg = m.counters()[1]
    m.close()
    assert n_seg == int(segs.sum()) == mp.reference(pkg, ob, name, 4).n_seg


def test_refusals(pkg, ob):
    import torch
    name = "mis/cu-la"
    m, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    scene = mp.frame(ob)
    d_rad = torch.zeros(3 * mp.H * mp.W, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def changed(**kw):
        t = np.array(mats).copy()
        for k, v in kw.items():
            t[k] = v
        return t

    assert _raw(pkg, m, scene, mats, 0, d_rad) == -1 and "invalid argument" in m.L.last_error()
    assert _raw(pkg, m, scene, None, 4, d_rad) == -1
    assert _raw(pkg, m, scene, mats, 4, None) == -1
    for cap_cos in (1.0, -1.0, 1.5):
        assert _raw(pkg, m, scene, changed(cap_cos=cap_cos), 4, d_rad) == -1
    for n in (0, 5, 2 ** 31):
        assert _raw(pkg, m, scene, changed(n_materials=n), 4, d_rad) == -1, n
    for bad in (2, -1):
        t = changed()
        t["material"][1]["type"] = bad
        assert _raw(pkg, m, scene, t, 4, d_rad) == -1, bad
    rows = np.array(scene, dtype=pkg.SCENE_S)
    rows["y_begin"], rows["y_count"] = 10, mp.H
    assert _raw(pkg, m, rows, mats, 4, d_rad) == -1
    shard = np.array(scene, dtype=pkg.SCENE_S)
    shard["shard_index"], shard["shard_count"] = 2, 2
    assert _raw(pkg, m, shard, mats, 4, d_rad) == -1
    ws = pkg.WeightSpaceMedium(pkg.params_for_config("C1"))
    assert _raw(pkg, ws, scene, mats, 4, d_rad) == -1
    ws.close()
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any()
    # a type outside the enum in an entry beyond n_materials is not read
    t = changed()
    t["material"][3]["type"] = 7
    assert _raw(pkg, m, scene, t, 4, d_rad) == 0
    torch.cuda.synchronize()
    assert d_rad.cpu().numpy().any()
    m.close()


# ---- the adaptive entry: every sample is a pure function of (x, y, k, scene_seed), so an adaptive frame is, pixel by pixel, a
# concatenation of spp ranges the uniform entry renders: per-sample values and segment counts from that entry (one call per k), the
# schedule from tests/adaptive_ref.py's plain-C plan, clamp and luminance from tests/adaptive_paths_rgb_ref.py.  22 x 14 at 32 spp in
# steps of 16: one uniform and one planned pass.
AW, AH, ASPP = ar.SMALL_W, ar.SMALL_H, 32


def _ascene(ob, spp=ASPP, **fields):
    scene = ob.default_scene_s(AW, AH, spp)
    scene["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        scene[k] = v
    return scene


class Buffers:
    """device buffers of one adaptive frame; fill != 0 makes a write visible"""
    def __init__(self, w, h, fill=0):
        import torch
        self.w, self.h, self.vw, self.vh = w, h, (w + 3) // 4, (h + 3) // 4
        self.rad = torch.full((3 * h * w,), float(fill), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.seg = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.rec = torch.full((self.vh * self.vw * ar.RECORD.itemsize,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {"radiance_sum": self.rad.cpu().numpy().reshape(self.h, self.w, 3), "sample_count": self.cnt.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "seg_count": self.seg.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "records": self.rec.cpu().numpy().view(ar.RECORD).reshape(self.vh, self.vw)}


def _status(pkg, med, scene, adaptive, mats, bounces, b, rad=True, cnt=True, seg=True, rec=True, info=True):
    """the adaptive entry's return value, on raw pointers"""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    t = None if mats is None else np.array(mats, dtype=pkg.MATERIALS_S)
    inf = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    st = getattr(med.L.lib, ADAPTIVE)(med.h, _vp(sc), _vp(ad), _vp(t), int(bounces), vp(b.rad.data_ptr()) if rad else None,
                                      vp(b.cnt.data_ptr()) if cnt else None, vp(b.seg.data_ptr()) if seg else None,
                                      vp(b.rec.data_ptr()) if rec else None, _vp(inf) if info else None, vp(stream_ptr()))
    return st, inf


def _adaptive(pkg, med, scene, mats, bounces=4, adaptive=None):
    b = Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, scene, ar.default_adaptive() if adaptive is None else adaptive, mats, bounces, b)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, scene, mats, bounces=4, into=None):
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, seg = into or (torch.zeros(3 * h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    med.call(ENTRY, np.array(scene, dtype=pkg.SCENE_S), np.array(mats, dtype=pkg.MATERIALS_S), int(bounces), rad.data_ptr(), seg.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w, 3), seg.cpu().numpy().view(np.uint32).reshape(h, w)


def _equal_frames(got, want):
    for k in apr.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


@pytest.mark.parametrize("name,bounces", [("mis/cu-la", 4), (mp.EMISSIVE_CASE, 4), (mp.EMISSIVE_CASE, 1)])
def test_adaptive_frame_equals_the_schedule_over_per_sample_calls(pkg, ob, name, bounces):
    if not apr.available():
        pytest.skip("no C compiler for the restatement")
    med, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    scene = _ascene(ob)
    want = apr.frame(ar.default_adaptive(), AW, AH, ASPP, apr.per_sample_rgb(lambda one: _uniform(pkg, med, one, mats, bounces), scene))
    counts = want["counts"]
    print(name, bounces, want["info"], "counts per pass", [(int(c.min()), int(c.max())) for c in counts], "clamped", int(want["clamped"].sum()))
    # a real schedule: a uniform pass of 16, then a planned pass with tiles at one sample and tiles above the step
    assert len(counts) == 2 and (counts[0] == 16).all() and (counts[1] == 1).any() and (counts[1] > ASPP - 16).any()
    assert want["radiance_sum"].max() > 0 and want["seg_count"].max() > 0 and not want["clamped"].any()
    got = _adaptive(pkg, med, scene, mats, bounces)
    _equal_frames(got, want)
    if bounces == 4 and name == "mis/cu-la":           # and through the binding; then chunks of 2^8 samples and the lane-per-ray kernels
        rad, cnt, segs, rec, info = med.render_scene_s_material_paths_rgb_adaptive(scene, mats, bounces, want_segs=True, want_records=True)
        _equal_frames({"radiance_sum": rad, "sample_count": cnt, "seg_count": segs, "records": rec, "info": info}, got)
        med.set_option("chunk_log2", 8)
        _equal_frames(_adaptive(pkg, med, scene, mats, bounces), got)
        med.set_option("chunk_log2", 0)
        med.set_option("persistent", 0)
        _equal_frames(_adaptive(pkg, med, scene, mats, bounces), got)
    med.close()


def test_adaptive_threshold_at_or_above_the_spp_is_uniform(pkg, ob):
    """With threshold >= S every pass is uniform: the image is the sequence of the passes' uniform calls accumulated into one
    buffer, bit for bit (nothing is clamped), and every pixel has S samples."""
    import torch
    name = mp.EMISSIVE_CASE
    med, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    for S, step in ((16, 16), (32, 16), (24, 16)):
        scene = _ascene(ob, S)
        got = _adaptive(pkg, med, scene, mats, adaptive=ar.default_adaptive(spp_step=step, threshold=64))
        into = (torch.zeros(3 * AH * AW, dtype=torch.float32, device="cuda"), torch.zeros(AH * AW, dtype=torch.int32, device="cuda"))
        passes = 0
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, part, mats, into=into)
            passes += 1
        assert want[0].max() > 0 and want[0].max() <= 65536
        assert np.array_equal(_bits(got["radiance_sum"]), _bits(want[0])) and np.array_equal(got["seg_count"], want[1])
        assert (got["sample_count"] == S).all() and (got["records"]["sample_index"] == S).all()
        assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (passes, 0, AW * AH * S)
    med.close()


def test_adaptive_refusals(pkg, ob):
    import ws_oracle
    name = "mis/cu-la"
    med, mats = mp.medium(pkg, name), mp.CASES[name](pkg)[1]
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    ok, good = _ascene(ob, 16), ar.default_adaptive()

    def changed(**kw):
        t = np.array(mats).copy()
        for k, v in kw.items():
            t[k] = v
        return t

    bad_type = changed()
    bad_type["material"][0]["type"] = 2
    cases = {
        "bounces 0": (med, ok, good, mats, 0, {}),
        "no table": (med, ok, good, None, 4, {}),
        "cap_cos 1": (med, ok, good, changed(cap_cos=1.0), 4, {}),
        "cap_cos -1": (med, ok, good, changed(cap_cos=-1.0), 4, {}),
        "no materials": (med, ok, good, changed(n_materials=0), 4, {}),
        "five materials": (med, ok, good, changed(n_materials=5), 4, {}),
        "a type outside the enum": (med, ok, good, bad_type, 4, {}),
        "no image": (med, ok, good, mats, 4, {"rad": False}),
        "weight-space handle": (ws, ok, good, mats, 4, {}),
        "rows": (med, _ascene(ob, 16, y_begin=1, y_count=AH - 1), good, mats, 4, {}),
        "shards": (med, _ascene(ob, 16, shard_count=2), good, mats, 4, {}),
        "spp_step 0": (med, ok, ar.default_adaptive(spp_step=0), mats, 4, {}),
        "threshold 1": (med, ok, ar.default_adaptive(threshold=1), mats, 4, {}),
        "no settings": (med, ok, None, mats, 4, {}),
        "no sample counts": (med, ok, good, mats, 4, {"cnt": False}),
        "no samples": (med, _ascene(ob, 0), good, mats, 4, {}),
    }
    for what, (handle, scene, adaptive, t, bounces, missing) in cases.items():
        b = Buffers(AW, AH, fill=7)
        st, info = _status(pkg, handle, scene, adaptive, t, bounces, b, **missing)
        assert st == -1, (what, st)
        out = b.host()
        assert (out["radiance_sum"] == 7).all() and (out["sample_count"] == 7).all() and (out["seg_count"] == 7).all(), what
        assert (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), what
    assert _status(pkg, med, ok, good, mats, 4, Buffers(AW, AH))[0] == 0
    ws.close()
    med.close()
