"""gpis_render_scene_s_paths_adaptive on the GPU.  Every sample of the library is a pure function of (x, y, k, scene_seed), so an
adaptive frame is, pixel by pixel, a concatenation of spp ranges gpis_render_scene_s_paths already renders: the per-sample values
come from that entry (one call per k, spp_count = 1, zeroed buffers), the schedule, the clamp, the sums and the statistics from the
restatement (tests/paths_adaptive_ref.py over tests/adaptive_ref.py), and the entry's image, counts, records and info must equal
the composite bit for bit.  Then: the smallest frame, the recorded fixture, the two stated consequences, a shifted spp_begin,
chunking, tuning options, accumulation, the NULL outputs and the refusals."""
import numpy as np
import pytest

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


def _medium(pkg, config, guide=False):
    m = pkg.Medium(pkg.params_for_config(config))
    if guide:
        m.build_guide(*par.GUIDE)
    return m


# name -> (configuration, guide, max_path_bounces, scene fields)
CASES = {
    "C0_4": ("C0", False, 4, {}),
    "C1_guided_3": ("C1", True, 3, {}),
    "clamped_light": ("C0", False, 4, {"light_radiance": 1e6}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composite(env, name):
    pkg, ob = env
    config, guide, bounces, fields = CASES[name]
    med = _medium(pkg, config, guide)
    drv = pag.Lambert(bounces)
    scene = par.scene(ob, **fields)
    want = pag.composite(pkg, med, drv, scene)
    pag.describe(name, want)
    assert par.is_real_schedule(want["counts"]) and want["radiance_sum"].max() > 0
    if name == "clamped_light":
        par.assert_clamp_case(want)
        assert want["radiance_sum"].max() <= par.LIMIT * want["sample_count"].max()
    else:
        par.assert_no_clamp(want)
    got = pag.adaptive(pkg, med, drv, scene)
    pag.equal(got, want, drv.keys)
    med.close()


def test_smallest_frame(env):
    """5 x 3 from the default distance: two records, both clipped (4 x 3 and 1 x 3), 480 samples — not a multiple of 64"""
    pkg, ob = env
    med = _medium(pkg, "C0")
    drv = pag.Lambert(3)
    scene = par.scene(ob, 48, 5, 3, cam_pos=(0.0, 0.0, 4.0))
    want = pag.composite(pkg, med, drv, scene)
    pag.describe("5 x 3", want)
    assert want["records"].shape == (1, 2) and int(want["info"]["samples"]) % 64 != 0 and want["radiance_sum"].max() > 0
    pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
    med.close()


@pytest.mark.parametrize("config, guide, bounces", [("C0", False, 4), ("C1", True, 3)])
def test_odd_spp_on_a_clipped_frame(env, config, guide, bounces):
    pkg, ob = env
    med = _medium(pkg, config, guide)
    pag.check_odd_spp_on_a_clipped_frame(pkg, med, pag.Lambert(bounces), ob)
    med.close()


def test_fixture(env):
    pkg, ob = env
    g = np.load(par.GOLDEN_LAMBERT)
    med = pkg.Medium(np.array(g["params"], dtype=pkg.PARAMS))
    scene, settings = np.array(g["scene"], dtype=pkg.SCENE_S), np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S)
    drv = pag.Lambert(int(g["max_bounces"]), float(g["albedo"]))
    got = pag.adaptive(pkg, med, drv, scene, settings)
    pag.equal(got, {k: g[k] for k in drv.keys}, drv.keys)
    # and through the binding
    rad, cnt, rec, info = med.render_scene_s_paths_adaptive(g["scene"], drv.max_bounces, drv.albedo, g["adaptive"], want_records=True)
    pag.equal({"radiance_sum": rad, "sample_count": cnt, "records": rec, "info": info}, got, drv.keys)
    rad2, cnt2, info2 = med.render_scene_s_paths_adaptive(g["scene"], drv.max_bounces, drv.albedo)
    assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
    med.close()


def test_threshold_at_or_above_the_spp_is_uniform(env):
    pkg, ob = env
    med = _medium(pkg, "C0")
    pag.check_uniform_schedule(pkg, med, pag.Lambert(4), ob)
    med.close()


def test_one_bounce_stops_after_the_first_pass(env):
    pkg, ob = env
    med = _medium(pkg, "C0")
    pag.check_one_bounce(pkg, med, pag.Lambert(1), ob)
    med.close()


def test_spp_begin_shifts_every_sample(env):
    pkg, ob = env
    med = _medium(pkg, "C0")
    drv = pag.Lambert(4)
    scene = par.scene(ob, spp_begin=7)
    want = pag.composite(pkg, med, drv, scene)
    unshifted = pag.adaptive(pkg, med, drv, par.scene(ob))
    got = pag.adaptive(pkg, med, drv, scene)
    pag.equal(got, want, drv.keys)
    assert got["radiance_sum"].tobytes() != unshifted["radiance_sum"].tobytes()
    med.close()


def test_chunk_independence(env):
    """128 x 128 at 32 spp, 2 bounces: the first pass is 2^18 samples, 4 chunks at GPIS_OPT_CHUNK_LOG2 = 16 against one by default"""
    pkg, ob = env
    med = _medium(pkg, "C1", guide=True)
    drv = pag.Lambert(2)
    scene = par.scene(ob, 32, 128, 128)
    whole = pag.adaptive(pkg, med, drv, scene)
    assert int(whole["info"]["passes_rendered"]) == 2 and int(whole["info"]["samples"]) > 4 * 65536
    assert whole["sample_count"].min() < 32 < whole["sample_count"].max() and whole["radiance_sum"].max() > 0
    med.set_option("chunk_log2", 16)
    pag.equal(pag.adaptive(pkg, med, drv, scene), whole, drv.keys)
    med.close()


def test_tuning_options_change_nothing(env):
    pkg, ob = env
    med = _medium(pkg, "C1", guide=True)
    drv = pag.Lambert(4)
    scene = par.scene(ob)
    want = pag.adaptive(pkg, med, drv, scene)
    assert want["radiance_sum"].max() > 0
    for form in ("resident", "wave", "auto"):
        med.set_option("march_form", form)
        for sort, presort in ((1, 1), (1, 0), (0, 1), (0, 0)):
            med.set_option("paths_sort", sort)
            med.set_option("paths_presort", presort)
            pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
    med.close()
    # the lane-per-ray kernels in place of the persistent march
    med = _medium(pkg, "C0")
    want = pag.adaptive(pkg, med, drv, scene)
    print("persistent", med.get_option("persistent"))
    med.set_option("persistent", 0)
    pag.equal(pag.adaptive(pkg, med, drv, scene), want, drv.keys)
    med.close()


def test_accumulation(env):
    pkg, ob = env
    med = _medium(pkg, "C0")
    pag.check_accumulation(pkg, med, pag.Lambert(4), ob)
    med.close()


def test_null_outputs(env):
    pkg, ob = env
    med = _medium(pkg, "C0")
    pag.check_null_outputs(pkg, med, pag.Lambert(4), ob)
    med.close()


def test_refusals(env):
    pkg, ob = env
    import adaptive_ref as ar
    import ws_oracle
    med = _medium(pkg, "C0")
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    drv = pag.Lambert(4)
    pag.check_refusals(pkg, pag.common_refusals(ob, med, ws, drv, lambda b: pag.Lambert(b)))
    assert drv.status(pkg, med, par.scene(ob, 16), ar.default_adaptive(), pag.Buffers(W, H))[0] == 0
    ws.close()
    med.close()
