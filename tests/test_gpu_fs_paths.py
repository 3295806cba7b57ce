"""GPU parity of the function-space multi-bounce path driver (gpis_fs_render_scene_s_paths): image and per-pixel segment counts
BIT FOR BIT against the CPU composite (tests/fs_paths_ref.py: the camera step of the scene composite, the CPU restatement of the
medium on gpis_fs_state VALUES, the split shade step), the invariance of the image under row ranges, shards, spp ranges, chunks
and repeated calls, the sharing of the workspace and state slots with the sibling entries, and the refusals.  No tolerance on any
device result: images are compared as uint32 views.  The one place float32 itself does not allow bit equality — a frame cut
into two spp ranges against the uncut frame — is held to fs_scene_ref.assert_spp_cut_equals_whole, and bit for bit to the
composite cut the same way.

The composite a device image is held to conditions every path segment on the context the PREVIOUS PATH segment left and never
forks the sampler; tests/test_fs_paths_cpu.py shows that either mistake changes the image (in-place shadow segments under
Renewal, Renewal+ and Global; a forked sampler under every context), so a kernel that ran the shadow segment in place on the
path's slot, or that restored the sampler after it, fails these comparisons.  Every case asserts its non-vacuity on the composite
(fs_paths_ref.check_non_vacuous)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fs_paths_ref
import fs_scene_ref
import ws_scene_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fs_paths_small.npz")


@pytest.fixture(scope="module")
def ref(pkg, ob):
    if not fs_paths_ref.available():
        pytest.skip("no C compiler for the shade step")
    return fs_paths_ref.FsPathsRef(pkg, ob, threads=16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(img, segs, want):
    assert np.array_equal(segs, want.segs), np.argwhere(segs != want.segs)[:8]
    assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]


def _check_frame(pkg, ref, p, scene, max_bounces, albedo, impossible=()):
    want = ref.compose(p, scene, max_bounces, albedo)
    fs_paths_ref.check_non_vacuous(want, impossible)
    m = pkg.Medium(p)
    img, segs = m.fs_render_scene_s_paths(scene, max_bounces, albedo, want_segs=True)
    m.close()
    _equal(img, segs, want)
    return want


def test_library_exports_the_path_entry(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_fs_render_scene_s_paths$", out, flags=re.M)
    assert callable(getattr(pkg.Medium, "fs_render_scene_s_paths", None))


@pytest.mark.parametrize("name", sorted(fs_paths_ref.CASES))
def test_frame_equals_composite(pkg, ob, ref, name):
    """The four contexts at 3 bounces, 64 points under Global, max_bounces 1 / 2 / 4, albedo 1, an anisotropic covariance, the
    homogeneous mean and an absorption-only medium (fs_paths_ref.CASES)."""
    p, scene, max_bounces, albedo, impossible = fs_paths_ref.case(pkg, ob, name)
    want = _check_frame(pkg, ref, p, scene, max_bounces, albedo, impossible)
    if name in fs_paths_ref.THREE_HITS:
        assert want.n_three_hits > 0
    if max_bounces == 1:
        assert not want.image.any()


def test_fixture(pkg):
    """the device against the recorded composite: needs no C compiler"""
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    m = pkg.Medium(p)
    img, segs = m.fs_render_scene_s_paths(scene, int(g["max_bounces"]), float(g["albedo"]), want_segs=True)
    m.close()
    assert g["image"].any() and np.array_equal(_bits(img), _bits(g["image"])) and np.array_equal(segs, g["segs"])


def test_every_workgroup_takes_several_samples(pkg, ob, ref):
    import torch
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 4        # one one-wave workgroup per SIMD
    want = _check_frame(pkg, ref, fs_scene_ref.fs_params(pkg, "NONE", 12, 0.0), ws_scene_ref.small_scene(ob, 48, 32, 3, fov=60.0), 3, 0.8)
    assert want.n_samples == 4608 >= 3 * resident + 17


def _call(pkg, m, scene, max_bounces, albedo, d_rad, d_seg=None):
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    m.L.check(m.L.lib.gpis_fs_render_scene_s_paths(m.h, s.ctypes.data_as(ctypes.c_void_p), int(max_bounces), ctypes.c_float(albedo),
                                                   ctypes.c_void_p(d_rad.data_ptr()), ctypes.c_void_p(d_seg.data_ptr()) if d_seg is not None else None,
                                                   None), "gpis_fs_render_scene_s_paths")


def _accumulate(pkg, m, scenes, max_bounces, albedo, want_segs=True):
    """several driver calls into ONE pair of device buffers"""
    import torch
    s0 = np.array(scenes[0], dtype=pkg.SCENE_S).reshape(())
    h, w = int(s0["height"]), int(s0["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(h * w, dtype=torch.int32, device="cuda") if want_segs else None
    torch.cuda.synchronize()
    for s in scenes:
        _call(pkg, m, s, max_bounces, albedo, d_rad, d_seg)
    torch.cuda.synchronize()
    rad = d_rad.cpu().numpy().reshape(h, w)
    return (rad, d_seg.cpu().numpy().view(np.uint32).reshape(h, w)) if want_segs else rad


def _parts(ob, kind):
    def base(spp_begin=0):
        s = ws_scene_ref.small_scene(ob, 24, 16, 4, spp_begin=spp_begin, fov=60.0)
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
    elif kind == "spp":
        for s0, sn in ((0, 2), (2, 2)):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    elif kind == "spp_last":           # the second call adds ONE sample: the whole frame's own order of addition
        for s0, sn in ((0, 3), (3, 1)):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    else:                              # "spp_begin": one call that does not start at sample 0
        return base(5), [base(5)]
    return base(), out


@pytest.mark.parametrize("kind", ["rows", "shards", "spp", "spp_last", "spp_begin"])
@pytest.mark.parametrize("ctx,n,step", [("RENEWAL_PLUS", 16, 0.04), ("GLOBAL", 14, 0.05)])
def test_cutting(pkg, ob, ref, kind, ctx, n, step):
    p = fs_scene_ref.fs_params(pkg, ctx, n, step)
    whole_scene, parts = _parts(ob, kind)
    m = pkg.Medium(p)
    whole, whole_segs = m.fs_render_scene_s_paths(whole_scene, 3, 0.8, want_segs=True)
    got, got_segs = _accumulate(pkg, m, parts, 3, 0.8)
    part_imgs = [m.fs_render_scene_s_paths(s, 3, 0.8) for s in parts] if kind == "spp" else None
    m.close()
    want = ref.compose(p, whole_scene, 3, 0.8)
    fs_paths_ref.check_non_vacuous(want)
    _equal(whole, whole_segs, want)
    acc = None
    for s in parts:
        acc = ref.compose(p, s, 3, 0.8, into=acc)
    _equal(got, got_segs, acc)                                     # the composite, cut the same way
    assert np.array_equal(got_segs, whole_segs)
    if kind == "spp":
        fs_scene_ref.assert_spp_cut_equals_whole(got, part_imgs, whole)
    else:
        assert np.array_equal(_bits(got), _bits(whole))


def test_chunked_frame(pkg, ob, ref):
    """96 x 64 x 12 = 73 728 samples in chunks of 2^16: two chunks (the second one 8 192 samples), against the same frame in one
    chunk, and both against the composite of the whole frame (a few seconds on the CPU for this medium)."""
    p = fs_scene_ref.fs_params(pkg, "NONE", 12, 0.0)
    scene = ws_scene_ref.small_scene(ob, 96, 64, 12, fov=60.0)
    assert 96 * 64 * 12 > 2 ** 16
    m = pkg.Medium(p)
    assert m.get_option("chunk_log2") == 0
    one, one_segs = m.fs_render_scene_s_paths(scene, 3, 0.8, want_segs=True)
    m.set_option("chunk_log2", 16)
    two, two_segs = m.fs_render_scene_s_paths(scene, 3, 0.8, want_segs=True)
    m.close()
    assert one.any() and one_segs.any() and np.array_equal(_bits(two), _bits(one)) and np.array_equal(two_segs, one_segs)
    want = ref.compose(p, scene, 3, 0.8)
    fs_paths_ref.check_non_vacuous(want)
    _equal(two, two_segs, want)


def test_two_calls_accumulate(pkg, ob, ref):
    """x + x is exact in float32, so two calls into one buffer give twice the single call's image, and the composite's"""
    p, scene, max_bounces, albedo, _ = fs_paths_ref.case(pkg, ob, "renewal-16")
    want = ref.compose(p, scene, max_bounces, albedo)
    m = pkg.Medium(p)
    twice, segs2 = _accumulate(pkg, m, [scene, scene], max_bounces, albedo)
    m.close()
    assert want.image.any() and np.array_equal(_bits(twice), _bits(want.image + want.image)) and np.array_equal(segs2, want.segs + want.segs)


def test_seg_count_may_be_null(pkg, ob, ref):
    p, scene, max_bounces, albedo, _ = fs_paths_ref.case(pkg, ob, "none-12")
    want = ref.compose(p, scene, max_bounces, albedo)
    m = pkg.Medium(p)
    img = _accumulate(pkg, m, [scene], max_bounces, albedo, want_segs=False)
    m.close()
    assert want.image.any() and np.array_equal(_bits(img), _bits(want.image))


def test_interleaved_with_the_sibling_entries(pkg, ob, ref):
    """gpis_fs_render_scene_s and gpis_fs_sample_distance_batch on the same handle and stream, between two path frames: the
    workspace, the path slots (k_fs_scene's) and the record array are shared, and no call sees what another left there."""
    p, scene, max_bounces, albedo, _ = fs_paths_ref.case(pkg, ob, "renewal_plus-32")
    want = ref.compose(p, scene, max_bounces, albedo)
    want_scene = ref.scene_ref.compose(p, scene)
    c = want_scene.last
    m = pkg.Medium(p)
    img0, segs0 = m.fs_render_scene_s_paths(scene, max_bounces, albedo, want_segs=True)
    simg, shits = m.fs_render_scene_s(scene, want_hits=True)
    img1, segs1 = m.fs_render_scene_s_paths(scene, max_bounces, albedo, want_segs=True)
    seg, st1 = m.fs_sample_distance(c["rays"], c["states"])
    img2, segs2 = m.fs_render_scene_s_paths(scene, max_bounces, albedo, want_segs=True)
    simg2 = m.fs_render_scene_s(scene)
    m.close()
    for img, segs in ((img0, segs0), (img1, segs1), (img2, segs2)):
        _equal(img, segs, want)
    assert np.array_equal(_bits(simg), _bits(want_scene.image)) and np.array_equal(shits, want_scene.hits) and np.array_equal(_bits(simg2), _bits(simg))
    assert seg.tobytes() == c["seg"].tobytes() and st1.tobytes() == c["states_after"].tobytes()


def test_refusals(pkg, ob):
    import torch
    import ws_oracle
    L = pkg.load_library()
    scene = np.array(ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0), dtype=pkg.SCENE_S).reshape(())
    d_rad = torch.zeros(24 * 16, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(24 * 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sp, rp, cp = scene.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rad.data_ptr()), ctypes.c_void_p(d_seg.data_ptr())
    f = ctypes.c_float(0.8)
    entry = L.lib.gpis_fs_render_scene_s_paths
    good = pkg.Medium(fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04))
    wp, ww = ws_oracle.ws_params(pkg, n_basis=8)
    ws = pkg.WeightSpaceMedium(wp, ww)
    matern = fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04)
    matern["kernel_type"], matern["matern_v"] = 1, 2.5                 # GPIS_KERNEL_MATERN: a sparse-convolution-only medium
    sc = pkg.Medium(matern)
    assert entry(good.h, sp, 0, f, rp, cp, None) == -1                 # GPIS_ERR_INVALID_ARG: max_path_bounces >= 1
    assert entry(good.h, sp, -2, f, rp, cp, None) == -1
    assert entry(ws.h, sp, 3, f, rp, cp, None) == -1                   # a weight-space handle
    assert entry(sc.h, sp, 3, f, rp, cp, None) == -1                   # what gpis_fs_render_scene_s refuses
    assert L.lib.gpis_fs_render_scene_s(sc.h, sp, rp, cp, None) == -1
    assert entry(None, sp, 3, f, rp, cp, None) == -1
    assert entry(good.h, None, 3, f, rp, cp, None) == -1
    assert entry(good.h, sp, 3, f, None, cp, None) == -1
    bad = scene.copy()
    bad["spp_count"] = 0
    assert entry(good.h, bad.ctypes.data_as(ctypes.c_void_p), 3, f, rp, cp, None) == -1
    # the sibling path entries keep their own refusals
    assert L.lib.gpis_ws_render_scene_s_paths(good.h, sp, 3, f, rp, None) == -1
    assert L.lib.gpis_render_scene_s_paths(ws.h, sp, 3, f, rp, None) == -1
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any() and not d_seg.cpu().numpy().any()
    assert entry(good.h, sp, 3, f, rp, cp, None) == 0                  # the handle still renders
    torch.cuda.synchronize()
    ws.close()
    sc.close()
    good.close()
    assert d_rad.cpu().numpy().any() and d_seg.cpu().numpy().any()
