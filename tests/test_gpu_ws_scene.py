"""GPU parity of the weight-space scene-S frame driver (gpis_ws_render_scene_s): image and hit counts bit for bit against the CPU
composite (tests/ws_scene_ref.py) and the recorded fixture tests/golden/ws_scene_small.npz, the counters against the composite's
work, and the invariance of the image under shards, row ranges, spp ranges and repeated calls.  No tolerance anywhere: images are
compared as uint32 views.

The conditions that keep a case from passing vacuously are asserted on the composite's outputs: every case holds a sample that
misses the bounding sphere, one that leaves the medium without a hit, a hit whose shadow ray is occluded and a hit whose shadow
ray is visible.  absorption_only is the one exception, by construction and not by its inputs: sampleDistance of an
absorption-only medium reports exited = 1 for every segment (GPM.cpp:304-312), so the frame has no hit and no shadow ray whatever
the scene; that case asserts the miss and the exit, and that the composite indeed holds no hit."""
import ctypes
import os
import struct
import time

import numpy as np
import pytest

import ws_oracle
import ws_scene_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_scene_small.npz")
CTXS = ["global", "renewal_plus", "renewal", "none"]
TWO_SPHERE_LIGHT = (-1.0, -0.3, 0.2)      # the second sphere of the CSG mean shadows the first (needed where the field is the mean alone)

# name -> (ws_params keywords, scene keywords, light)
CASES = {}
for _c in CTXS:
    for _s in (0, 1):
        CASES["%s-single%d" % (_c, _s)] = (dict(ctx=_c, single=_s), {}, None)
CASES["finite_differences"] = (dict(ctx="renewal", normal=1), {}, None)
CASES["finite_differences-single"] = (dict(ctx="none", single=1, normal=1), {}, None)
CASES["two_ids"] = (dict(ctx="renewal", mean_additional=True), {}, None)
CASES["absorption_only"] = (dict(ctx="renewal_plus", absorption_only=True), {}, None)
CASES["n0"] = (dict(ctx="renewal", n_basis=0, mean_additional=True), {}, TWO_SPHERE_LIGHT)
CASES["n65"] = (dict(ctx="renewal", n_basis=65), {}, None)
CASES["spp3"] = (dict(ctx="global", n_basis=65), dict(spp=3), None)                    # not a multiple of 4
CASES["spp8_from5"] = (dict(ctx="renewal", n_basis=65), dict(spp=8, spp_begin=5), None)   # a multiple of 4, spp_begin > 0


@pytest.fixture(scope="module")
def ref(pkg, ob):
    if not ws_scene_ref.available():
        pytest.skip("no C compiler for the restatement (the fixture test still runs)")
    return ws_scene_ref.SceneRef(pkg, ob)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(ob, scene_kw, light):
    s = ws_scene_ref.small_scene(ob, **scene_kw)
    if light is not None:
        s["light_dir"] = light
    return s


def _non_vacuous(c, kw):
    assert c.n_miss > 0 and c.n_exit > 0, (c.n_miss, c.n_exit)
    if kw.get("absorption_only"):
        assert c.n_hit == 0 and c.n_lit == 0              # see the module docstring
        return
    assert c.n_occluded > 0 and c.n_visible > 0, (c.n_occluded, c.n_visible)
    if kw.get("mean_additional"):
        assert c.hit_gp_ids == {0, 1}, c.hit_gp_ids


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_equals_composite(pkg, ob, ref, case):
    kw, scene_kw, light = CASES[case]
    p, w = ws_oracle.ws_params(pkg, **kw)
    scene = _scene(ob, scene_kw, light)
    want = ref.compose(p, w, scene)
    _non_vacuous(want, kw)
    m = pkg.WeightSpaceMedium(p, w)
    m.reset_counters()
    img, hits = m.render_scene_s(scene, want_hits=True)
    c = m.counters()
    m.close()
    assert np.array_equal(hits, want.hits)
    assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]
    # realization reuse and dynamic fetch changed no work the reference does
    assert c["n_eval"] == want.n_eval and c["n_seg"] == want.n_seg and c["n_spec"] >= c["n_eval"], (c, want.n_eval, want.n_seg)


def _accumulate(pkg, m, scenes):
    """several driver calls into ONE pair of device buffers"""
    import torch
    s0 = np.array(scenes[0], dtype=pkg.SCENE_S).reshape(())
    h, w = int(s0["height"]), int(s0["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    d_hit = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        s = np.array(s, dtype=pkg.SCENE_S).reshape(())
        m.L.check(m.L.lib.gpis_ws_render_scene_s(m.h, s.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rad.data_ptr()),
                                                 ctypes.c_void_p(d_hit.data_ptr()), None), "gpis_ws_render_scene_s")
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w), d_hit.cpu().numpy().view(np.uint32).reshape(h, w)


def _parts(ob, kind):
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
        # "spp": the second call adds one sample per pixel, which is the whole frame's own order of addition;
        # "spp_assoc": (a0 + a1) + ((a2 + a3) + a4): compared with the composite accumulated through the same calls
        for s0, sn in (((0, 4), (4, 1)) if kind == "spp" else ((0, 2), (2, 3))):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    return base(), out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["shards", "rows", "spp", "spp_assoc"])
@pytest.mark.parametrize("ctx,single", [("renewal", 0), ("global", 0), ("none", 1)])
def test_partition_invariance(pkg, ob, ref, kind, ctx, single):
    p, w = ws_oracle.ws_params(pkg, ctx=ctx, single=single, n_basis=65)
    whole_scene, parts = _parts(ob, kind)
    m = pkg.WeightSpaceMedium(p, w)
    whole, whole_hits = m.render_scene_s(whole_scene, want_hits=True)
    got, got_hits = _accumulate(pkg, m, parts)
    m.close()
    assert whole.any() and np.array_equal(got_hits, whole_hits)
    if kind == "spp_assoc":
        acc = None
        for s in parts:
            acc = ref.compose(p, w, s, into=acc)
        assert np.array_equal(_bits(got), _bits(acc.image))
    else:
        assert np.array_equal(_bits(got), _bits(whole))
        want = ref.compose(p, w, whole_scene)
        assert np.array_equal(_bits(whole), _bits(want.image))


@pytest.mark.gpu
def test_two_calls_accumulate(pkg, ob):
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=65)
    scene = ws_scene_ref.small_scene(ob)
    m = pkg.WeightSpaceMedium(p, w)
    img, hits = m.render_scene_s(scene, want_hits=True)
    twice, hits2 = _accumulate(pkg, m, [scene, scene])
    m.close()
    assert img.any() and np.array_equal(_bits(twice), _bits(img + img)) and np.array_equal(hits2, hits + hits)


@pytest.mark.gpu
def test_fixture(pkg):
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    w = np.array(g["ws"]).view(pkg.WS_PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    m = pkg.WeightSpaceMedium(p, w)
    img, hits = m.render_scene_s(scene, want_hits=True)
    m.close()
    assert np.array_equal(_bits(img), _bits(g["image"])) and np.array_equal(hits, g["hits"])
    assert g["image"].any() and g["hits"].any()


@pytest.mark.gpu
def test_global_context_reuses_the_primary_realization(pkg, ob, ref):
    """Under context GLOBAL the device marches the shadow segment through the realization it built for the primary segment; the
    composite builds the shadow segment's realization anew (pss.w = 0 either way).  Same image, same work."""
    p, w = ws_oracle.ws_params(pkg, ctx="global", single=0, n_basis=300)
    scene = ws_scene_ref.small_scene(ob, spp=6)
    rays, us, pix, miss = ref.primary_rays(scene)
    seg, _ = ref.wso.sample_distance(p, w, rays)
    shadow, cosl, hit, lit = ref.shade(scene, rays, seg, us)
    idx = np.nonzero(lit)[0]
    assert len(idx) > 50
    # the composite's shadow rays carry segment 1, and their realizations are those of segment 0
    assert (shadow["segment"][idx] == 1).all()
    pss1 = np.stack([shadow["pixel"][idx[:4], 0], shadow["pixel"][idx[:4], 1], shadow["spp"][idx[:4]], shadow["segment"][idx[:4]]], 1)
    pss0 = pss1.copy()
    pss0[:, 3] = 0
    assert np.array_equal(ref.wso.basis(p, w, pss1), ref.wso.basis(p, w, pss0))
    want = ref.compose(p, w, scene)
    _non_vacuous(want, {})
    m = pkg.WeightSpaceMedium(p, w)
    m.reset_counters()
    img, hits = m.render_scene_s(scene, want_hits=True)
    c = m.counters()
    m.close()
    assert np.array_equal(_bits(img), _bits(want.image)) and np.array_equal(hits, want.hits)
    assert c["n_eval"] == want.n_eval and c["n_seg"] == want.n_seg


@pytest.mark.gpu
def test_refusals(pkg, ob):
    import torch
    L = pkg.load_library()
    scene = np.array(ws_scene_ref.small_scene(ob), dtype=pkg.SCENE_S).reshape(())
    n = int(scene["width"]) * int(scene["height"])
    d_rad = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sp, rp = scene.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rad.data_ptr())
    p, w = ws_oracle.ws_params(pkg, n_basis=8)
    ws = pkg.WeightSpaceMedium(p, w)
    sc = pkg.Medium(pkg.params_for_config("C0"))
    assert L.lib.gpis_ws_render_scene_s(sc.h, sp, rp, None, None) == -1          # GPIS_ERR_INVALID_ARG
    assert L.lib.gpis_render_scene_s(ws.h, sp, rp, None, None) == -1             # as before this entry existed
    assert L.lib.gpis_ws_render_scene_s(ws.h, None, rp, None, None) == -1
    assert L.lib.gpis_ws_render_scene_s(ws.h, sp, None, None, None) == -1
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any()
    ws.close()
    sc.close()


@pytest.mark.gpu
def test_argument_beyond_restated_range_is_unsupported(pkg, ob, ref):
    """The construction of test_gpu_ws.py's argument-range test (one basis function of a single realization, read back from the
    restatement, the argument computed on the host), with a length scale so small that the first point the reference evaluates
    on the central primary ray already lies beyond the restated range of cos."""
    p, w = ws_oracle.ws_params(pkg, ctx="none", single=1, n_basis=1, sigma=1e-6, length_scale=1e-9)
    b = ref.wso.basis(p, w, np.zeros((1, 4), dtype=np.uint32))[0, 0]          # d.x, d.y, d.z, omega, phi, w of the one function
    d, om, ph = b[:3], float(b[3]), float(b[4])
    T = struct.unpack("<d", struct.pack("<Q", 0x419921FB00000000))[0]          # smallest |x| cos_glibc does not restate
    scene = ws_scene_ref.small_scene(ob)
    rays, _, _, _ = ref.primary_rays(scene)
    r = rays[len(rays) // 2]
    q = r["pos"].astype(np.float64) + float(r["near_t"]) * r["dir"].astype(np.float64)      # the march's first point (f0)
    arg = ((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]) * om + ph
    assert np.isfinite(arg) and abs(arg) >= T, arg
    m = pkg.WeightSpaceMedium(p, w)
    with pytest.raises(RuntimeError, match=r"\(-2\).*105414350"):
        m.render_scene_s(scene)
    m.close()
    p["length_scale"] = 0.05
    m = pkg.WeightSpaceMedium(p, w)
    m.render_scene_s(scene)                      # the flag does not outlive the refused call's handle; a sane medium renders
    m.close()
