"""gpis_render_scene_s_nee_paths_adaptive on the GPU.  Every sample of the library is a pure function of (x, y, k, scene_seed), so an
adaptive frame is, pixel by pixel, a concatenation of spp ranges gpis_render_scene_s_nee_paths already renders: the per-sample
values and segment counts come from that entry (one call per k, spp_count = 1, zeroed buffers), the schedule, the clamp, the sums
and the statistics from the restatement (tests/paths_adaptive_ref.py over tests/adaptive_ref.py), and the entry's image, counts,
records and info must equal the composite bit for bit.  Then: the smallest frame, the recorded fixture, the three stated
consequences, a shifted spp_begin, chunking, tuning options, accumulation, the NULL outputs and the refusals."""
import numpy as np
import pytest

import adaptive_ref as ar
import nee_paths_ref as npr
import paths_adaptive_gpu as pag
import paths_adaptive_ref as par

pytestmark = pytest.mark.gpu

W, H = pag.W, pag.H


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not par.available():
        pytest.skip("no C compiler for the restatements")
    return pkg, ob


def _medium(pkg, name, **surface_fields):
    params, surf, guide = npr.CASES[name](pkg)
    m = pkg.Medium(params)
    if guide:
        m.build_guide(*par.GUIDE)
    surf = np.array(surf, dtype=pkg.SURFACE_S)
    for k, v in surface_fields.items():
        surf[k] = v
    return m, surf


# name -> (case of nee_paths_ref.CASES, max_path_bounces, scene fields, surface fields)
CASES = {
    "mis_3": ("mis", 3, {}, {}),
    "uni_2": ("uni", 2, {}, {}),
    "colour_short_last_pass": ("mis-colour", 4, {"spp_count": 40}, {}),
    "dark_6": ("mis-dark", 6, {}, {}),
    "single_guided_4": ("single", 4, {}, {}),
    "clamped_cap": ("mis", 3, {}, {"cap_radiance": 1e6}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composite(env, name):
    pkg, ob = env
    case, bounces, fields, surface_fields = CASES[name]
    med, surf = _medium(pkg, case, **surface_fields)
    drv = pag.Nee(surf, bounces)
    scene = par.scene(ob, **fields)
    want = pag.composite(pkg, med, drv, scene)
    pag.describe(name, want)
    assert par.is_real_schedule(want["counts"])
    assert want["radiance_sum"].max() > 0 and want["seg_count"].max() > 0 and want["segs"].max() <= 3 * (bounces - 1)
    if name == "clamped_cap":
        par.assert_clamp_case(want)
        assert want["radiance_sum"].max() <= par.LIMIT * want["sample_count"].max()
    else:
        par.assert_no_clamp(want)
    if name == "colour_short_last_pass":
        assert int(want["info"]["samples"]) < W * H * 40 and (want["counts"].sum(axis=(1, 2))[2] < want["counts"].sum(axis=(1, 2))[1])
    pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
    med.close()


def test_smallest_frame(env):
    """5 x 3 from the default distance: two records, both clipped (4 x 3 and 1 x 3), 480 samples — not a multiple of 64"""
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    drv = pag.Nee(surf, 3)
    scene = par.scene(ob, 48, 5, 3, cam_pos=(0.0, 0.0, 4.0))
    want = pag.composite(pkg, med, drv, scene)
    pag.describe("5 x 3", want)
    assert want["records"].shape == (1, 2) and int(want["info"]["samples"]) % 64 != 0 and want["radiance_sum"].max() > 0
    pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
    med.close()


@pytest.mark.parametrize("case, bounces", [("mis", 3), ("uni", 2)])
def test_odd_spp_on_a_clipped_frame(env, case, bounces):
    pkg, ob = env
    med, surf = _medium(pkg, case)
    pag.check_odd_spp_on_a_clipped_frame(pkg, med, pag.Nee(surf, bounces), ob)
    med.close()


def test_fixture(env):
    pkg, ob = env
    g = np.load(par.GOLDEN_NEE)
    med = pkg.Medium(np.array(g["params"], dtype=pkg.PARAMS))
    scene, settings, surf = np.array(g["scene"], dtype=pkg.SCENE_S), np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S), np.array(g["surface"], dtype=pkg.SURFACE_S)
    drv = pag.Nee(surf, int(g["max_bounces"]))
    got = pag.adaptive(pkg, med, drv, scene, settings)
    pag.equal(got, {k: g[k] for k in drv.keys}, drv.keys)
    # and through the binding
    rad, cnt, segs, rec, info = med.render_scene_s_nee_paths_adaptive(g["scene"], g["surface"], drv.max_bounces, g["adaptive"], want_segs=True, want_records=True)
    pag.equal({"radiance_sum": rad, "sample_count": cnt, "seg_count": segs, "records": rec, "info": info}, got, drv.keys)
    rad2, cnt2, info2 = med.render_scene_s_nee_paths_adaptive(g["scene"], g["surface"], drv.max_bounces)
    assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
    med.close()


def test_threshold_at_or_above_the_spp_is_uniform(env):
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    pag.check_uniform_schedule(pkg, med, pag.Nee(surf, 3), ob)
    med.close()


@pytest.mark.parametrize("name", npr.PIN_CASES)
def test_two_bounces_equal_the_single_interaction_driver(env, name):
    """C2 has weight[0] == 1: at max_path_bounces = 2 and under a uniform schedule the image is gpis_render_scene_s_nee called once
    per pass with that pass's (spp_begin, spp_count), accumulated into one buffer, bit for bit"""
    import torch
    pkg, ob = env
    med, surf = _medium(pkg, name)

    def single(pkg, med, scene, into=None):
        med.call("gpis_render_scene_s_nee", np.array(scene, dtype=pkg.SCENE_S), np.array(surf, dtype=pkg.SURFACE_S), into[0].data_ptr(), pag.stream_ptr())
        torch.cuda.synchronize()
        return into[0].cpu().numpy().reshape(H, W), None
    pag.check_uniform_schedule(pkg, med, pag.Nee(surf, 2), ob, uniform=single)
    med.close()


def test_one_bounce_stops_after_the_first_pass(env):
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    pag.check_one_bounce(pkg, med, pag.Nee(surf, 1), ob)
    med.close()


def test_spp_begin_shifts_every_sample(env):
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    drv = pag.Nee(surf, 3)
    scene = par.scene(ob, spp_begin=7)
    want = pag.composite(pkg, med, drv, scene)
    unshifted = pag.adaptive(pkg, med, drv, par.scene(ob))
    got = pag.adaptive(pkg, med, drv, scene)
    pag.equal(got, want, drv.keys)
    assert got["radiance_sum"].tobytes() != unshifted["radiance_sum"].tobytes()
    med.close()


def test_chunk_independence(env):
    """128 x 128 at 32 spp, 3 bounces: the first pass is 2^18 samples, 4 chunks at GPIS_OPT_CHUNK_LOG2 = 16 against one by default"""
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    drv = pag.Nee(surf, 3)
    scene = par.scene(ob, 32, 128, 128)
    whole = pag.adaptive(pkg, med, drv, scene)
    assert int(whole["info"]["passes_rendered"]) == 2 and int(whole["info"]["samples"]) > 4 * 65536
    assert whole["sample_count"].min() < 32 < whole["sample_count"].max() and whole["radiance_sum"].max() > 0
    med.set_option("chunk_log2", 16)
    pag.equal(pag.adaptive(pkg, med, drv, scene), whole, drv.keys)
    med.close()


def test_tuning_options_change_nothing(env):
    """the lane-per-ray kernels in place of the persistent march, and on a guided handle every form of the march"""
    pkg, ob = env
    scene = par.scene(ob)
    for name, options in (("mis", (("persistent", 0),)), ("single", (("march_form", "resident"), ("march_form", "wave"), ("march_form", "auto")))):
        med, surf = _medium(pkg, name)
        drv = pag.Nee(surf, 4)
        want = pag.adaptive(pkg, med, drv, scene)
        assert want["radiance_sum"].max() > 0
        for key, value in options:
            med.set_option(key, value)
            pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
        med.close()


def test_accumulation(env):
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    pag.check_accumulation(pkg, med, pag.Nee(surf, 3), ob)
    med.close()


def test_null_outputs(env):
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    pag.check_null_outputs(pkg, med, pag.Nee(surf, 3), ob)
    med.close()


def test_refusals(env):
    pkg, ob = env
    import ws_oracle
    med, surf = _medium(pkg, "mis")
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    drv = pag.Nee(surf, 3)
    cases = pag.common_refusals(ob, med, ws, drv, lambda b: pag.Nee(surf, b))
    ok, good = par.scene(ob, 16), ar.default_adaptive()
    cases["no surface"] = (med, drv, ok, good, {"surface": False})
    for name, cap_cos in (("cap_cos 1", 1.0), ("cap_cos -1", -1.0), ("cap_cos 1.5", 1.5), ("cap_cos nan", float("nan"))):
        bad = np.array(surf, dtype=pkg.SURFACE_S)
        bad["cap_cos"] = cap_cos
        cases[name] = (med, pag.Nee(bad, 3), ok, good, {})
    pag.check_refusals(pkg, cases)
    assert drv.status(pkg, med, ok, good, pag.Buffers(W, H))[0] == 0
    ws.close()
    med.close()
