"""The Lambert frame driver's primary march does not evaluate the state of segments that exit ("Wavefront driver";
k_guided_sample_distance_noexit).  That may not move a bit of the image or of the hit counts, whatever the frame's shape, the
light, the chunking or the sharding; the option GPIS_OPT_SCENE_EXIT_STATE only changes how many evaluations run."""
import ctypes

import numpy as np
import pytest

from gpu_util import stream_ptr, scene_rays

pytestmark = pytest.mark.gpu

LIGHTS = {"default": None, "view_axis": (0.0, 0.0, 1.0), "behind": (0.0, 0.0, -1.0)}


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return pkg, ob


@pytest.fixture(scope="module")
def c1(env):
    """one guided C1 handle and its oracle, shared: every test leaves the options at their defaults"""
    pkg, ob = env
    params = pkg.params_for_config("C1")
    med = pkg.Medium(params)
    med.build_guide(16, 8)
    return med, ob.Oracle(params, threads=16)


_oracle_frames = {}


def _scene(ob, w, h, spp, light="default"):
    scene = ob.default_scene_s(w, h, spp)
    if LIGHTS[light] is not None:
        scene["light_dir"] = LIGHTS[light]
    return scene


def _want(orc, cfg, scene, key):
    """the oracle's frame, computed once per (configuration, shape, light)"""
    k = (cfg,) + key
    if k not in _oracle_frames:
        _oracle_frames[k] = orc.render_scene_s(scene, want_hits=True)
    return _oracle_frames[k]


def _render(pkg, med, scene, parts=None):
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    hits = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    for part in (parts or [scene]):
        sc = np.array(part, dtype=pkg.SCENE_S)
        med.call("gpis_render_scene_s", sc.ctypes.data_as(ctypes.c_void_p), rad.data_ptr(), hits.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w), hits.cpu().numpy().reshape(h, w).astype(np.uint32)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("spp", [8, 5, 64])
def test_oracle_parity_c1(env, c1, spp):
    """spp 5: 25 920 samples, no multiple of 256, the waves straddle pixels and k_scene_accumulate takes its scalar path; spp 64: one
    pixel per wave, as in the benchmark."""
    pkg, ob = env
    med, orc = c1
    assert med.get_option("scene_exit_state") == 0
    scene = _scene(ob, 96, 54, spp)
    got, want = _render(pkg, med, scene), _want(orc, "C1", scene, (96, 54, spp, "default"))
    assert want[0].max() > 0 and want[1].sum() > 0
    assert _same(got, want)


def test_oracle_parity_c0(env):
    pkg, ob = env
    params = pkg.params_for_config("C0")
    med, orc = pkg.Medium(params), ob.Oracle(params, threads=16)
    med.build_guide(16, 8)
    scene = _scene(ob, 96, 96, 4)
    want = orc.render_scene_s(scene, want_hits=True)
    assert want[0].max() > 0
    assert _same(_render(pkg, med, scene), want)


def test_exit_state_changes_nothing_but_work(env, c1):
    """Both settings of the option render the oracle's frame; the lean march saves exactly one value and one gradient evaluation per
    primary segment that exits, and nothing else moves.  The exits are counted by the oracle, segment by segment: the hit_count
    sum cannot stand in for "valid - exits", because a crossing whose sampled gradient faces away from the ray ends with ok = 0
    (GPM.cpp:283-300) — it is no hit for the estimator, yet its march evaluated the gradient at the crossing in both forms
    (96x54x8: 41 472 valid samples, 36 897 hits, 4 436 exits, 139 crossings with ok = 0; 8 872 evaluations saved)."""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 8)
    want = _want(orc, "C1", scene, (96, 54, 8, "default"))
    rays = scene_rays(ob, orc, scene)[0]                  # the bounding-sphere test of every sample, on the host
    seg = orc.sample_distance(rays)
    ok, exited = seg["ok"] != 0, seg["exited"] != 0
    n_valid, n_hit, n_exit, n_bad = len(rays), int(want[1].sum()), int((ok & exited).sum()), int((~ok).sum())
    assert 0 < n_hit < n_valid <= 96 * 54 * 8          # at 16:9 and fov 35 every pixel of this frame looks into the bounding sphere
    assert n_hit == int((ok & ~exited).sum()) and not (~ok & exited).any() and n_valid - n_hit == n_exit + n_bad and n_exit > 0
    work = {}
    try:
        for exit_state in (0, 1):
            med.set_option("scene_exit_state", exit_state)
            med.reset_counters()
            assert _same(_render(pkg, med, scene), want), exit_state
            sd, tr = med.kernel_profile(0), med.kernel_profile(1)
            work[exit_state] = {"sd_eval": sd[2], "sd_seg": sd[3], "tr_eval": tr[2], "tr_seg": tr[3], "guide": med.guide_steps()}
    finally:
        med.set_option("scene_exit_state", 0)
    print(n_valid, n_hit, n_exit, n_bad, work)
    lean, full = work[0], work[1]
    assert lean["sd_seg"] == full["sd_seg"] == n_valid
    assert (lean["tr_eval"], lean["tr_seg"], lean["guide"]) == (full["tr_eval"], full["tr_seg"], full["guide"])
    assert full["sd_eval"] - lean["sd_eval"] == 2 * n_exit


def test_guided_equals_unguided(env):
    pkg, ob = env
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(6, 32)
    scene = _scene(ob, 96, 54, 8)
    guided = _render(pkg, med, scene)
    assert med.guide_steps() > 0
    med.drop_guide()
    assert _same(_render(pkg, med, scene), guided)
    assert guided[0].max() > 0


def test_chunks_shards_and_frames(env):
    pkg, ob = env
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(16, 8)
    w, h = 96, 54
    scene = _scene(ob, w, h, 16)
    first = _render(pkg, med, scene)          # the handle's first frame: the first-frame workspace plan
    second = _render(pkg, med, scene)         # the steady-state plan, and whatever the first frame left in the workspace
    assert first[0].max() > 0 and _same(first, second)
    med.set_option("chunk_log2", 16)          # 82 944 samples: two chunks
    assert _same(_render(pkg, med, scene), first)
    med.set_option("chunk_log2", 0)
    rows = []
    for y0, yc in ((0, h // 3), (h // 3, h - h // 3)):
        part = scene.copy()
        part["y_begin"], part["y_count"] = y0, yc
        rows.append(part)
    assert _same(_render(pkg, med, scene, rows), first)
    shards = []
    for r in range(3):
        part = scene.copy()
        part["shard_index"], part["shard_count"] = r, 3
        shards.append(part)
    assert _same(_render(pkg, med, scene, shards), first)


@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_light_directions(env, c1, light):
    """many, most and almost no shadow rays per wave of the transmittance batch"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 8, light)
    want = _want(orc, "C1", scene, (96, 54, 8, light))
    med.reset_counters()
    got = _render(pkg, med, scene)
    n_shadow, n_hit = med.kernel_profile(1)[3], int(want[1].sum())
    print(light, "hits", n_hit, "shadow rays", n_shadow)
    if light == "view_axis":
        assert n_shadow > 0.9 * n_hit
    elif light == "behind":
        assert n_shadow < 0.1 * n_hit
    assert _same(got, want)


def test_new_instance_keeps_the_budget(pkg):
    """k_guided_sample_distance_noexit: no more scratch and no lower occupancy (VGPR allocation granule of 8, 512 per SIMD) than the
    instance it stands in for"""
    from test_kernel_resources import _kernels
    k = _kernels(pkg.library_path())
    for small_arg in ("ILb0E", "ILb1E"):
        old = [v for n, v in k.items() if "k_guided_sample_distance" + small_arg in n]
        new = [v for n, v in k.items() if "k_guided_sample_distance_noexit" + small_arg in n]
        assert len(old) == 1 and len(new) == 1, (small_arg, sorted(k))
        old, new = old[0], new[0]
        waves = lambda v: 512 // (8 * ((v["vgpr_count"] + 7) // 8))
        assert new["private_segment_fixed_size"] <= old["private_segment_fixed_size"], (old, new)
        assert waves(new) >= waves(old), (old, new)
        assert new["group_segment_fixed_size"] <= old["group_segment_fixed_size"], (old, new)
