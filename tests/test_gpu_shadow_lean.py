"""The lean form of the guided transmittance march ("Lean shadow march"; GPIS_OPT_SHADOW_LEAN, k_shadow_lean /
k_shadow_lean_scene).  Visibility depends on whether a step's sign differs from sign0, not on where inside the step the crossing
lies, and a continued segment never reads its start value: the lean instances evaluate exactly only at the steps the guide cannot
decide and keep only signs.  That may not move a bit of any frame or of any visibility flag; it only changes how many evaluations
run, and by how many is pinned below (for a batch of continued segments n_eval + n_guide = sum(1 + K_i), K_i = the march steps
of segment i up to and including its crossing step)."""
import numpy as np
import pytest

from gpu_util import scene_rays, shadow_rays_from
from test_gpu_scene_lean import LIGHTS, _render, _same, _scene, _want

gpu = pytest.mark.gpu


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
    assert med.get_option("shadow_lean") == 1 and med.get_option("scene_compact") == 1
    return med, ob.Oracle(params, threads=16)


def _work(med):
    sd, tr = med.kernel_profile(0), med.kernel_profile(1)
    return {"sd_eval": sd[2], "sd_seg": sd[3], "tr_eval": tr[2], "tr_seg": tr[3], "guide": med.guide_steps()}


def _both_settings(pkg, med, scene, want):
    work = {}
    try:
        for lean in (1, 0):
            med.set_option("shadow_lean", lean)
            med.reset_counters()
            assert _same(_render(pkg, med, scene), want), lean
            work[lean] = _work(med)
    finally:
        med.set_option("shadow_lean", 1)
    print(work)
    return work


@gpu
@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("spp", [8, 5, 64])
def test_frame_identity(env, c1, spp, light):
    """the oracle's image and hit counts with the option on and off; the same shadow segments, strictly fewer evaluations in them
    with the option on, and a primary march that does not notice (spp 5: the waves straddle pixels; spp 64: one pixel per wave)"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, spp, light)
    want = _want(orc, "C1", scene, (96, 54, spp, light))
    assert want[0].max() > 0 and want[1].sum() > 0
    work = _both_settings(pkg, med, scene, want)
    assert work[1]["tr_seg"] == work[0]["tr_seg"] > 0
    assert work[1]["tr_eval"] < work[0]["tr_eval"]
    assert (work[1]["sd_eval"], work[1]["sd_seg"]) == (work[0]["sd_eval"], work[0]["sd_seg"])


@gpu
def test_frame_identity_full_records(env, c1):
    """the full-record body of the frame driver: its shadow march is the batch instance k_shadow_lean under the driver's mask"""
    pkg, ob = env
    med, orc = c1
    scene = _scene(ob, 96, 54, 8)
    want = _want(orc, "C1", scene, (96, 54, 8, "default"))
    try:
        med.set_option("scene_compact", 0)
        full = _both_settings(pkg, med, scene, want)
    finally:
        med.set_option("scene_compact", 1)
    compact = _both_settings(pkg, med, scene, want)
    assert full == compact and full[1]["tr_eval"] < full[0]["tr_eval"]


# ---- the batch ABI ------------------------------------------------------------------------------------------------------------

_batches = {}


def _shadow_batch(pkg, ob, cfg):
    """shadow segments of a 480x270x2 scene (every 6th pixel) and the oracle's visibility for them, computed once per configuration;
    C1: 5 015 segments, 2 265 visible and 2 750 occluded; C0: 4 921, 2 739 and 2 182"""
    if cfg not in _batches:
        params = pkg.params_for_config(cfg)
        orc = ob.Oracle(params, threads=16)
        scene = ob.default_scene_s(480, 270, 2)
        rays, us = scene_rays(ob, orc, scene, step=6)
        sh = shadow_rays_from(ob, scene, rays, us, orc.sample_distance(rays))
        assert (sh["first_scatter"] == 0).all() and (sh["near_t"] == 0).all()
        _batches[cfg] = (params, orc, rays, sh, orc.transmittance(sh))
    return _batches[cfg]


def _variants(sh, vis, n_inf_visible):
    """the batch as the estimator traces it, and what else the ABI allows for the same rays"""
    out = {"as given": sh}
    fs = sh.copy()
    fs["first_scatter"] = 1                        # the start value is used: sign0 = sign(f(near_t)), no adopting step
    out["first_scatter"] = fs
    empty = sh.copy()
    empty["far_t"] = empty["near_t"]               # no step is taken: visible
    out["far_t = near_t"] = empty
    # far_t = inf: near_t + 2000 (GPM.cpp:349-351), 200 000 steps for a visible segment — a few rays only
    pick = np.concatenate([np.flatnonzero(vis == 1)[:n_inf_visible], np.flatnonzero(vis == 0)[:3]])
    inf = sh[pick].copy()
    inf["far_t"] = np.inf
    out["far_t = inf"] = inf
    return out


def _check_variants(med, orc, sh, vis, n_inf_visible):
    for name, batch in _variants(sh, vis, n_inf_visible).items():
        want = vis if name == "as given" else orc.transmittance(batch)
        for lean in (1, 0):
            med.set_option("shadow_lean", lean)
            got = med.transmittance(batch)
            print(name, "lean", lean, len(batch), "segments,", int(got.sum()), "visible")
            assert np.array_equal(got, want), (name, lean)
        if name == "far_t = near_t":
            assert want.all()
        elif name != "far_t = inf":
            assert 100 <= want.sum() <= len(want) - 100, name
    med.set_option("shadow_lean", 1)


@gpu
def test_batch_abi_c1(env):
    """guide 16:32: the shadow batch, its variants, and the far-origin bundles of test_gpu_guide.py (near_t in the hundreds and
    thousands; camera-like segments with first_scatter = 1, and the same bundles as continued segments)"""
    from test_gpu_guide import _far_bundle
    pkg, ob = env
    params, orc, rays, sh, vis = _shadow_batch(pkg, ob, "C1")
    med = pkg.Medium(params)
    med.build_guide(16, 32)
    assert med.get_option("shadow_lean") == 1
    _check_variants(med, orc, sh, vis, 1)
    rng = np.random.default_rng(11)
    far = np.concatenate([_far_bundle(rng, rays, 44.0), _far_bundle(rng, rays, 500.0), _far_bundle(rng, rays, 2000.0)])
    cont = far.copy()
    cont["first_scatter"] = 0
    for name, batch in (("far", far), ("far, continued", cont)):
        want = orc.transmittance(batch)
        for lean in (1, 0):
            med.set_option("shadow_lean", lean)
            assert np.array_equal(med.transmittance(batch), want), (name, lean)
    med.set_option("shadow_lean", 1)


@gpu
def test_batch_abi_small_field(env):
    """guide 6:32: the rays leave the tabulated volume and re-enter it; outside it every step is an exact one"""
    pkg, ob = env
    params, orc, rays, sh, vis = _shadow_batch(pkg, ob, "C1")
    med = pkg.Medium(params)
    med.build_guide(6, 32)
    for lean in (1, 0):
        med.set_option("shadow_lean", lean)
        assert np.array_equal(med.transmittance(sh), vis), lean
        fs = sh.copy()
        fs["first_scatter"] = 1
        assert np.array_equal(med.transmittance(fs), orc.transmittance(fs)), lean


@gpu
def test_batch_abi_c0(env):
    """a world-space medium (no isotropic-ray frame), guide 16:16"""
    pkg, ob = env
    params, orc, rays, sh, vis = _shadow_batch(pkg, ob, "C0")
    med = pkg.Medium(params)
    med.build_guide(16, 16)
    _check_variants(med, orc, sh, vis, 1)


@gpu
def test_accounting(env):
    """For continued segments the unguided march evaluates 1 + K_i + R_i times (the start value, K_i march steps up to and including
    the crossing step, R_i >= 1 refinement trips on occluded segments only; its transmittance kernel already skips lastVal).  The
    lean guided march evaluates or certifies 1 + K_i: equal on visible segments, at least one less per occluded segment.  With the
    option off the old relation holds: everything the unguided march evaluates is evaluated or certified, plus at most one
    re-evaluation of a certified previous step per segment."""
    pkg, ob = env
    params, orc, rays, sh, vis = _shadow_batch(pkg, ob, "C1")
    visible, occluded = sh[vis == 1], sh[vis == 0]
    assert len(visible) >= 100 and len(occluded) >= 100
    plain = pkg.Medium(params)
    med = pkg.Medium(params)
    med.build_guide(16, 32)

    def count(m, batch, want):
        m.reset_counters()
        assert np.array_equal(m.transmittance(batch), want)
        n_eval, n_seg = m.counters()
        assert n_seg == len(batch)
        return n_eval, (m.guide_steps() if m is med else 0)

    for name, batch, want in (("visible", visible, np.ones(len(visible), np.uint8)), ("occluded", occluded, np.zeros(len(occluded), np.uint8))):
        unguided = count(plain, batch, want)[0]
        med.set_option("shadow_lean", 1)
        e1, g1 = count(med, batch, want)
        med.set_option("shadow_lean", 0)
        e0, g0 = count(med, batch, want)
        med.set_option("shadow_lean", 1)
        print("%s: %d segments; unguided %d evaluations; lean %d + %d certified = %d; option off %d + %d = %d" % (
            name, len(batch), unguided, e1, g1, e1 + g1, e0, g0, e0 + g0))
        assert g1 > 0 and g0 > 0 and e1 <= e0
        if name == "visible":
            assert e1 + g1 == unguided
        else:
            assert e1 + g1 <= unguided - len(batch)
        assert 0 <= e0 + g0 - unguided <= len(batch)


# ---- resources (no GPU needed) ------------------------------------------------------------------------------------------------

def test_lean_instances_are_lighter(pkg):
    """each lean instance against its sibling in the same library: no more VGPRs, strictly less scratch, no more LDS"""
    import os
    from test_kernel_resources import LLVM, _kernels
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("LLVM tools of the ROCm image")
    k = _kernels(pkg.library_path())
    for lean, full in (("k_shadow_lean", "k_guided_transmittance"), ("k_shadow_lean_scene", "k_guided_transmittance_scene")):
        for small_arg in ("ILb0E", "ILb1E"):
            a = [v for n, v in k.items() if full + small_arg in n]
            b = [v for n, v in k.items() if lean + small_arg in n]
            assert len(a) == 1 and len(b) == 1, (lean, small_arg, sorted(k))
            a, b = a[0], b[0]
            print(lean + small_arg, b, "beside", a)
            assert b["vgpr_count"] <= a["vgpr_count"], (a, b)
            assert b["private_segment_fixed_size"] < a["private_segment_fixed_size"], (a, b)
            assert b["group_segment_fixed_size"] <= a["group_segment_fixed_size"], (a, b)
