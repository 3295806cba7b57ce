"""GPU parity of the function-space scene-S frame driver (gpis_fs_render_scene_s): image and hit counts BIT FOR BIT against the
CPU composite (tests/fs_scene_ref.py: the oracle's primary rays, the CPU restatement of the medium, the shared shade step and
pixel sum), the invariance of the image under row ranges, shards, spp ranges, chunks and repeated calls, the agreement of the
batch entries with the fused kernel (they run the same march code), and the refusals.  No tolerance on any device result: images
are compared as uint32 views.  The one place float32 itself does not allow bit equality — a frame cut into two spp ranges against
the uncut frame — is held to fs_scene_ref.assert_spp_cut_equals_whole, and bit for bit to the composite cut the same way.

Every case asserts on the composite that it holds a sample that misses the bounding sphere, one that leaves the medium, a hit, a
visible and an occluded shadow segment, so none can pass vacuously.  The homogeneous mean (offset 0.05) produces all five classes
in scene S as well (most of its non-hits end !ok rather than exited: the field is positive at the chord's start)."""
import ctypes

import numpy as np
import pytest

import fs_scene_ref
import ws_scene_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(pkg, ob):
    if not fs_scene_ref.available():
        pytest.skip("no C compiler for the shade step")
    return fs_scene_ref.FsSceneRef(pkg, ob, threads=16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_frame(pkg, ref, p, scene):
    want = ref.compose(p, scene)
    fs_scene_ref.assert_non_vacuous(want)
    m = pkg.Medium(p)
    img, hits = m.fs_render_scene_s(scene, want_hits=True)
    m.close()
    assert np.array_equal(hits, want.hits), np.argwhere(hits != want.hits)[:8]
    assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]
    return want


@pytest.mark.parametrize("name", sorted(fs_scene_ref.CASES))
def test_frame_equals_composite(pkg, ob, ref, name):
    """The 24 x 16 x 4 frames hold 1 536 samples, more than the 1 024 resident workgroups of a 256-CU part: the fetch wraps."""
    p, scene = fs_scene_ref.case(pkg, ob, name)
    _check_frame(pkg, ref, p, scene)


def test_every_workgroup_takes_several_samples(pkg, ob, ref):
    want = _check_frame(pkg, ref, fs_scene_ref.fs_params(pkg, "NONE", 12, 0.0), ws_scene_ref.small_scene(ob, 48, 32, 3, fov=60.0))
    assert want.n_samples == 4608


def test_anisotropic_covariance(pkg, ob, ref):
    _check_frame(pkg, ref, fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04, aniso=(1.0, 0.7, 1.4)), ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0))


def test_homogeneous_mean(pkg, ob, ref):
    want = _check_frame(pkg, ref, fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04, mean="HOMOGENEOUS", offset=0.05),
                        ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0))
    assert want.n_notok > 0


def _call(pkg, m, scene, d_rad, d_hit=None):
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    m.L.check(m.L.lib.gpis_fs_render_scene_s(m.h, s.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rad.data_ptr()),
                                             ctypes.c_void_p(d_hit.data_ptr()) if d_hit is not None else None, None), "gpis_fs_render_scene_s")


def _accumulate(pkg, m, scenes):
    """several driver calls into ONE pair of device buffers"""
    import torch
    s0 = np.array(scenes[0], dtype=pkg.SCENE_S).reshape(())
    h, w = int(s0["height"]), int(s0["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        _call(pkg, m, s, d_rad, d_hit)
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w), d_hit.cpu().numpy().view(np.uint32).reshape(h, w)


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
@pytest.mark.parametrize("ctx,n,step", [("RENEWAL", 16, 0.04), ("GLOBAL", 14, 0.05)])
def test_cutting(pkg, ob, ref, kind, ctx, n, step):
    p = fs_scene_ref.fs_params(pkg, ctx, n, step)
    whole_scene, parts = _parts(ob, kind)
    m = pkg.Medium(p)
    whole, whole_hits = m.fs_render_scene_s(whole_scene, want_hits=True)
    got, got_hits = _accumulate(pkg, m, parts)
    part_imgs = [m.fs_render_scene_s(s) for s in parts] if kind == "spp" else None
    m.close()
    want = ref.compose(p, whole_scene)
    fs_scene_ref.assert_non_vacuous(want)
    assert np.array_equal(_bits(whole), _bits(want.image)) and np.array_equal(whole_hits, want.hits)
    acc = None
    for s in parts:
        acc = ref.compose(p, s, into=acc)
    assert np.array_equal(_bits(got), _bits(acc.image)) and np.array_equal(got_hits, acc.hits)      # the composite, cut the same way
    assert np.array_equal(got_hits, whole_hits)
    if kind == "spp":
        fs_scene_ref.assert_spp_cut_equals_whole(got, part_imgs, whole)
    else:
        assert np.array_equal(_bits(got), _bits(whole))


def test_two_calls_accumulate(pkg, ob, ref):
    p, scene = fs_scene_ref.case(pkg, ob, "renewal-16")
    want = ref.compose(p, scene)
    m = pkg.Medium(p)
    twice, hits2 = _accumulate(pkg, m, [scene, scene])
    m.close()
    assert want.image.any() and np.array_equal(_bits(twice), _bits(want.image + want.image)) and np.array_equal(hits2, want.hits + want.hits)


def test_chunked_frame(pkg, ob, ref):
    """96 x 64 x 12 = 73 728 samples in chunks of 2^16: two chunks (the second one 8 192 samples), against the same frame in
    one chunk and against the composite — the whole image (the composite of this frame takes about two seconds)."""
    p = fs_scene_ref.fs_params(pkg, "NONE", 12, 0.0)
    scene = ws_scene_ref.small_scene(ob, 96, 64, 12, fov=60.0)
    m = pkg.Medium(p)
    assert m.get_option("chunk_log2") == 0
    one, one_hits = m.fs_render_scene_s(scene, want_hits=True)
    m.set_option("chunk_log2", 16)
    two, two_hits = m.fs_render_scene_s(scene, want_hits=True)
    m.close()
    assert one.any() and np.array_equal(_bits(two), _bits(one)) and np.array_equal(two_hits, one_hits)
    want = ref.compose(p, scene)
    fs_scene_ref.assert_non_vacuous(want)
    assert want.n_samples == 73728 > 2 ** 16
    assert np.array_equal(_bits(two), _bits(want.image)) and np.array_equal(two_hits, want.hits)


def test_batch_entries_agree_with_the_fused_kernel(pkg, ob, ref):
    """k_fs_march and k_fs_scene call the same fs_sample_distance_one / fs_transmittance_one: the batch entries on the
    composite's rays and states give the composite's records, states included, and their image is the fused image."""
    p, scene = fs_scene_ref.case(pkg, ob, "renewal_plus-32")
    want = ref.compose(p, scene)
    c = want.last
    m = pkg.Medium(p)
    seg, st1 = m.fs_sample_distance(c["rays"], c["states"])
    assert seg.tobytes() == c["seg"].tobytes()
    assert np.array_equal(st1["sampler_state"], c["states_after"]["sampler_state"])
    idx = np.nonzero(c["lit"])[0]
    vis = np.zeros(len(seg), dtype=np.uint8)
    vis[idx], _ = m.fs_transmittance(c["shadow"][idx], st1[idx])
    assert np.array_equal(vis, c["vis"])
    img, hits = m.fs_render_scene_s(scene, want_hits=True)
    m.close()
    sc = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    staged = np.zeros_like(want.image)
    staged_hits = np.zeros_like(want.hits)
    _p = ws_scene_ref._p
    ref.base.lib.ws_scene_sum(_p(sc), len(seg), _p(c["pix"]), _p(c["cosl"]), _p(c["hit"]), _p(c["lit"]), _p(vis), _p(staged), _p(staged_hits))
    assert staged.any() and np.array_equal(_bits(staged), _bits(img)) and np.array_equal(staged_hits, hits)


def test_refusals(pkg, ob):
    import torch
    import ws_oracle
    scene = ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0)
    d_rad = torch.zeros(24 * 16, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(24 * 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = fs_scene_ref.fs_params(pkg, "RENEWAL", 16, 0.04)

    wp, ww = ws_oracle.ws_params(pkg, n_basis=8)
    ws = pkg.WeightSpaceMedium(wp, ww)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):            # GPIS_ERR_INVALID_ARG
        _call(pkg, ws, scene, d_rad, d_hit)
    ws.close()
    for key, value in (("fs_sample_points", 65), ("nonstationary", 1)):
        bad = good.copy()
        bad[key] = value
        with pytest.raises(RuntimeError):
            m = pkg.Medium(bad)
            try:
                _call(pkg, m, scene, d_rad, d_hit)
            finally:
                m.close()
    m = pkg.Medium(good)
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(()).copy()
    s["y_begin"], s["y_count"] = 10, 7
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        _call(pkg, m, s, d_rad, d_hit)
    s = np.array(scene, dtype=pkg.SCENE_S).reshape(()).copy()
    s["spp_count"] = 0
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        _call(pkg, m, s, d_rad, d_hit)
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any() and not d_hit.cpu().numpy().any()
    _call(pkg, m, scene, d_rad, d_hit)                           # the handle still renders
    torch.cuda.synchronize()
    m.close()
    assert d_rad.cpu().numpy().any()
