"""GPU parity of the weight-space path driver (gpis_ws_render_scene_s_paths): image and counters (n_eval, n_seg) bit for bit
against the CPU composite (tests/ws_paths_ref.py) and the recorded fixture tests/golden/ws_paths_small.npz, and the invariance
of the image under shards, row ranges, spp ranges and repeated calls.  No tolerance anywhere: images are compared as uint32 views.

The cases are ws_paths_ref.CASES; what keeps each from passing vacuously (a sample that misses the bound, a path of three hits,
an exit after a hit, a path ended by its bounce, a visible and an occluded NEE ray) is asserted on the composite here and, without
a GPU, in tests/test_ws_paths_cpu.py, together with the classes a case cannot hold by construction."""
import ctypes
import os

import numpy as np
import pytest

import ws_oracle
import ws_paths_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_paths_small.npz")


@pytest.fixture(scope="module")
def ref(pkg):
    if not ws_paths_ref.available():
        pytest.skip("no C compiler for the restatement (the fixture test still runs)")
    return ws_paths_ref.PathsRef(pkg)


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(pkg, p, w, scene, max_bounces, albedo):
    m = pkg.WeightSpaceMedium(p, w)
    m.reset_counters()
    img = m.render_scene_s_paths(scene, max_bounces, albedo)
    c = m.counters()
    m.close()
    return img, c


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ws_paths_ref.CASES))
def test_frame_equals_composite(pkg, ob, ref, wso, case):
    p, w, scene, max_bounces, albedo, impossible = ws_paths_ref.case_inputs(pkg, ob, case)
    want = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, max_bounces, albedo)
    ws_paths_ref.check_non_vacuous(want, impossible)
    img, c = _render(pkg, p, w, scene, max_bounces, albedo)
    print(case, "image sum", float(img.sum()), "want", float(want.image.sum()), c, "want", want.n_eval, want.n_seg)
    assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]
    # realization reuse and dynamic fetch changed no work the reference does
    assert c["n_eval"] == want.n_eval and c["n_seg"] == want.n_seg and c["n_spec"] >= c["n_eval"], (c, want.n_eval, want.n_seg)
    if max_bounces == 1:
        assert not img.any() and c["n_seg"] > 0


def _accumulate(pkg, m, scenes, max_bounces, albedo):
    """several driver calls into ONE device buffer"""
    import torch
    s0 = np.array(scenes[0], dtype=pkg.SCENE_S).reshape(())
    h, w = int(s0["height"]), int(s0["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for s in scenes:
        s = np.array(s, dtype=pkg.SCENE_S).reshape(())
        m.L.check(m.L.lib.gpis_ws_render_scene_s_paths(m.h, s.ctypes.data_as(ctypes.c_void_p), int(max_bounces), ctypes.c_float(albedo),
                                                       ctypes.c_void_p(d_rad.data_ptr()), None), "gpis_ws_render_scene_s_paths")
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["shards", "rows", "spp", "spp_assoc"])
@pytest.mark.parametrize("ctx,single", [("renewal", 0), ("global", 0), ("none", 1)])
def test_partition_invariance(pkg, ob, ref, wso, kind, ctx, single):
    p, w = ws_oracle.ws_params(pkg, ctx=ctx, single=single, n_basis=65)
    march = ws_paths_ref.WsMarch(p, w, wso)
    whole_scene, calls = ws_paths_ref.parts(ob, kind)
    m = pkg.WeightSpaceMedium(p, w)
    whole = m.render_scene_s_paths(whole_scene, 3, 0.8)
    got = _accumulate(pkg, m, calls, 3, 0.8)
    m.close()
    assert whole.any()
    if kind == "spp_assoc":
        acc = None
        for s in calls:
            acc = ref.compose(march, s, 3, 0.8, into=acc)
        assert np.array_equal(_bits(got), _bits(acc.image))
    else:
        assert np.array_equal(_bits(got), _bits(whole))
        want = ref.compose(march, whole_scene, 3, 0.8)
        assert np.array_equal(_bits(whole), _bits(want.image))


@pytest.mark.gpu
def test_two_calls_accumulate(pkg, ob):
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=65)
    scene = ws_paths_ref.small_scene(ob)
    m = pkg.WeightSpaceMedium(p, w)
    img = m.render_scene_s_paths(scene, 3, 0.8)
    twice = _accumulate(pkg, m, [scene, scene], 3, 0.8)
    m.close()
    assert img.any() and np.array_equal(_bits(twice), _bits(img + img))


@pytest.mark.gpu
@pytest.mark.parametrize("ctx", ["renewal", "global"])
def test_every_wave_walks_several_samples(pkg, ob, ref, wso, ctx):
    """3 x (resident waves) + 17 samples: every wave fetches several samples of different cost (misses, one-hit exits, three-hit
    paths) from the counter, in an order that differs from run to run.  One row of one sample per pixel."""
    import torch
    resident = torch.cuda.get_device_properties(0).multi_processor_count * 8       # two one-wave workgroups per SIMD
    p, w = ws_oracle.ws_params(pkg, ctx=ctx, n_basis=65)
    scene = ws_paths_ref.small_scene(ob, width=3 * resident + 17, height=1, spp=1)
    want = ref.compose(ws_paths_ref.WsMarch(p, w, wso), scene, 3, 0.8)
    ws_paths_ref.check_non_vacuous(want)
    assert want.n_samples == 3 * resident + 17
    img, c = _render(pkg, p, w, scene, 3, 0.8)
    assert np.array_equal(_bits(img), _bits(want.image))
    assert c["n_eval"] == want.n_eval and c["n_seg"] == want.n_seg


@pytest.mark.gpu
def test_fixture(pkg):
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    w = np.array(g["ws"]).view(pkg.WS_PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    img, c = _render(pkg, p, w, scene, int(g["max_bounces"]), float(g["albedo"]))
    assert g["image"].any() and np.array_equal(_bits(img), _bits(g["image"]))
    assert c["n_eval"] == int(g["n_eval"]) and c["n_seg"] == int(g["n_seg"])


@pytest.mark.gpu
def test_refusals(pkg, ob):
    import torch
    L = pkg.load_library()
    scene = np.array(ws_paths_ref.small_scene(ob), dtype=pkg.SCENE_S).reshape(())
    n = int(scene["width"]) * int(scene["height"])
    d_rad = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sp, rp = scene.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rad.data_ptr())
    f = ctypes.c_float(0.8)
    p, w = ws_oracle.ws_params(pkg, n_basis=8)
    ws = pkg.WeightSpaceMedium(p, w)
    sc = pkg.Medium(pkg.params_for_config("C0"))
    assert L.lib.gpis_ws_render_scene_s_paths(sc.h, sp, 3, f, rp, None) == -1          # GPIS_ERR_INVALID_ARG: not a ws handle
    assert L.lib.gpis_render_scene_s_paths(ws.h, sp, 3, f, rp, None) == -1             # as before this entry existed
    assert L.lib.gpis_ws_render_scene_s_paths(ws.h, sp, 0, f, rp, None) == -1          # max_path_bounces >= 1
    assert L.lib.gpis_ws_render_scene_s_paths(ws.h, sp, -2, f, rp, None) == -1
    assert L.lib.gpis_ws_render_scene_s_paths(ws.h, None, 3, f, rp, None) == -1
    assert L.lib.gpis_ws_render_scene_s_paths(ws.h, sp, 3, f, None, None) == -1
    torch.cuda.synchronize()
    assert not d_rad.cpu().numpy().any()
    ws.close()
    sc.close()
