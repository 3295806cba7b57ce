"""The Lambert frame driver passes 32-byte ray and hit records between its kernels wherever the resident guided march without exit
state runs ("Wavefront driver"; GPIS_OPT_SCENE_COMPACT, k_scene_primary_c / k_guided_sample_distance_scene /
k_scene_shade_c / k_guided_transmittance_scene).  The records drop what no kernel reads and move the camera position and the light
direction into the launch; no evaluation changes.  So the image, the hit counts and every work counter are those of the full-record
body and of the oracle, whatever the frame's shape, camera, light, chunking or sharding."""
import numpy as np
import pytest

from gpu_util import scene_rays
from test_gpu_scene_lean import LIGHTS, _render, _same, _scene, _want

pytestmark = pytest.mark.gpu


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
    assert med.get_option("scene_compact") == 1 and med.get_option("scene_exit_state") == 0
    return med, ob.Oracle(params, threads=16)


def _work(med):
    sd, tr = med.kernel_profile(0), med.kernel_profile(1)
    return {"sd_eval": sd[2], "sd_seg": sd[3], "tr_eval": tr[2], "tr_seg": tr[3], "guide": med.guide_steps()}


@pytest.mark.parametrize("spp", [8, 5, 64])
def test_oracle_parity_c1(env, c1, spp):
    """spp 5: 25 920 samples, no multiple of 256, the waves straddle pixels and k_scene_accumulate takes its scalar path; spp 64: one
    pixel per wave, as in the benchmark."""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, spp)
    got, want = _render(pkg, med, scene), _want(orc, "C1", scene, (96, 54, spp, "default"))
    assert want[0].max() > 0 and want[1].sum() > 0
    assert _same(got, want)


def test_oracle_parity_c0(env):
    pkg, ob = env
    params = pkg.params_for_config("C0")
    med, orc = pkg.Medium(params), ob.Oracle(params, threads=16)
    med.build_guide(16, 8)
    assert med.get_option("scene_compact") == 1
    scene = _scene(ob, 96, 96, 4)
    want = orc.render_scene_s(scene, want_hits=True)
    assert want[0].max() > 0
    assert _same(_render(pkg, med, scene), want)


def test_compact_changes_no_evaluation(env, c1):
    """option off = option on: the image, the hit counts, and every work counter — evaluations and segments of both marches and the
    certified guide steps"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 8)
    want = _want(orc, "C1", scene, (96, 54, 8, "default"))
    work = {}
    try:
        for compact in (1, 0):
            med.set_option("scene_compact", compact)
            med.reset_counters()
            assert _same(_render(pkg, med, scene), want), compact
            work[compact] = _work(med)
    finally:
        med.set_option("scene_compact", 1)
    print(work)
    assert work[1]["sd_seg"] > 0 and work[1]["tr_seg"] > 0 and work[1]["guide"] > 0
    assert work[1] == work[0]


def test_off_axis_camera(env, c1):
    """the camera position reaches the primary march as a kernel argument: off the axis and further away"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 8)
    scene["cam_pos"] = (0.3, -0.2, 6.0)
    want = orc.render_scene_s(scene, want_hits=True)
    assert want[0].max() > 0 and want[1].sum() > 0
    assert _same(_render(pkg, med, scene), want)


def test_samples_that_miss_the_bound(env, c1):
    """at fov 70 the corners of the 16:9 frame look past the bounding sphere (radius 1.5 at distance 4: half-angle 22 degrees, the
    frame's half-width 35): those samples carry flag 0 through every kernel"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 4)
    scene["cam_fov_deg"] = 70.0
    n_inside = len(scene_rays(ob, orc, scene)[0])
    print("inside the bound:", n_inside, "of", 96 * 54 * 4)
    assert 0 < n_inside < 96 * 54 * 4
    want = orc.render_scene_s(scene, want_hits=True)
    assert want[0].max() > 0 and want[1].sum() > 0
    med.reset_counters()
    got = _render(pkg, med, scene)
    assert med.kernel_profile(0)[3] == n_inside          # primary segments marched
    assert _same(got, want)


@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_light_directions(env, c1, light):
    """the light direction reaches the shadow march as a kernel argument; many, most and almost no shadow rays per wave"""
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


def test_chunks_shards_and_frames(env):
    pkg, ob = env
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(16, 8)
    assert med.get_option("scene_compact") == 1
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


def test_full_record_body_in_two_chunks(env):
    """64 x 64 at 32 spp = 131 072 samples: two chunks at GPIS_OPT_CHUNK_LOG2 = 16, the smallest.  The chunked frame of the full-record
    body is the frame rendered as one chunk, bit for bit (the compact body in two chunks: test_chunks_shards_and_frames)."""
    pkg, ob = env
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(16, 8)
    scene = _scene(ob, 64, 64, 32)
    compact = _render(pkg, med, scene)
    med.set_option("scene_compact", 0)
    whole = _render(pkg, med, scene)
    assert whole[0].max() > 0 and whole[1].sum() > 0 and _same(whole, compact)
    med.set_option("chunk_log2", 16)
    assert _same(_render(pkg, med, scene), whole)
    med.set_option("scene_compact", 1)
    assert _same(_render(pkg, med, scene), whole)


def test_fall_backs_on_the_same_handle(env):
    """the full-record body after the compact one has used the workspace, and the compact one again after it: with the exit state
    switched on, and without a guide"""
    pkg, ob = env
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(16, 8)
    scene = _scene(ob, 96, 54, 8)
    compact = _render(pkg, med, scene)
    assert compact[0].max() > 0 and compact[1].sum() > 0
    med.set_option("scene_exit_state", 1)
    assert _same(_render(pkg, med, scene), compact)
    med.set_option("scene_exit_state", 0)
    assert _same(_render(pkg, med, scene), compact)
    med.drop_guide()
    assert _same(_render(pkg, med, scene), compact)
