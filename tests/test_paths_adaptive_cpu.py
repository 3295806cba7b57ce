"""gpis_render_scene_s_paths_adaptive and gpis_render_scene_s_nee_paths_adaptive, checked without a GPU: the declared, bound and
exported interface and the refusals that need no device; the recorded fixtures (tests/golden/paths_adaptive_small.npz,
tests/golden/nee_paths_adaptive_small.npz) against the CPU composite (tests/paths_adaptive_ref.py: the oracle's per-sample values
under the restated pass loop); and, on the CPU composite, what the GPU tests assert of their cases: a real schedule and no clamped
sample, or samples on both sides of the limit."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ar
import nee_paths_ref as npr
import paths_adaptive_ref as par

sys.path.insert(0, os.path.join(par.ROOT, "tests", "golden"))

ENTRIES = ("gpis_render_scene_s_paths_adaptive", "gpis_render_scene_s_nee_paths_adaptive")
needs_cc = pytest.mark.skipif(not par.available(), reason="no C compiler for the restatements")


# ---- interface
def test_header_declares_both_entries(pkg):
    header = open(os.path.join(par.ROOT, "include", "gpis.h")).read()
    assert re.search(r"^(?:extern )?int gpis_render_scene_s_paths_adaptive\(gpis_medium \*m, const gpis_scene_s \*s, const gpis_adaptive_s \*a,\s*"
                     r"int max_path_bounces, float albedo,\s*float \*radiance_sum, uint32_t \*sample_count,\s*"
                     r"gpis_adaptive_record \*records, gpis_adaptive_info \*info, void \*stream\);", header, flags=re.M)
    assert re.search(r"^(?:extern )?int gpis_render_scene_s_nee_paths_adaptive\(gpis_medium \*m, const gpis_scene_s \*s, const gpis_adaptive_s \*a,\s*"
                     r"const gpis_surface_s \*surf, int max_path_bounces,\s*float \*radiance_sum, uint32_t \*sample_count, uint32_t \*seg_count,\s*"
                     r"gpis_adaptive_record \*records, gpis_adaptive_info \*info, void \*stream\);", header, flags=re.M)


def test_library_exports_both_entries(pkg):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for name in ENTRIES:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert name in pkg.GpisLib.SYMBOLS
    for method in ("render_scene_s_paths_adaptive", "render_scene_s_nee_paths_adaptive"):
        assert callable(getattr(pkg.Medium, method, None))


def test_entries_refuse_a_missing_handle_without_a_device(pkg, ob):
    """the argument checks come before the first device call: no handle is GPIS_ERR_INVALID_ARG, and nothing is written"""
    L = pkg.load_library()
    scene = np.array(par.scene(ob, 16), dtype=pkg.SCENE_S)
    settings = np.array(ar.default_adaptive(), dtype=pkg.ADAPTIVE_S)
    surf = np.array(pkg.default_surface_s(), dtype=pkg.SURFACE_S)
    rad, cnt = np.full(ar.SMALL_W * ar.SMALL_H, 7.0, dtype=np.float32), np.full(ar.SMALL_W * ar.SMALL_H, 7, dtype=np.uint32)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.lib.gpis_render_scene_s_paths_adaptive(None, p(scene), p(settings), 4, ctypes.c_float(0.8), p(rad), p(cnt), None, p(info), None) == -1
    assert "gpis_render_scene_s_paths_adaptive: invalid argument" in L.last_error()
    assert L.lib.gpis_render_scene_s_nee_paths_adaptive(None, p(scene), p(settings), p(surf), 4, p(rad), p(cnt), None, None, p(info), None) == -1
    assert "gpis_render_scene_s_nee_paths_adaptive: invalid argument" in L.last_error()
    assert (rad == 7).all() and (cnt == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO)


# ---- the fixtures
def _same(g, want, keys):
    for k in keys:
        a, b = np.ascontiguousarray(g[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, k
        if b.dtype.names:                # a record: field by field (the padding between fields is not data)
            a = np.array(a, dtype=b.dtype)
            for f in b.dtype.names:
                assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), (k, f)
        else:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


@needs_cc
def test_lambert_fixture_is_the_cpu_composite(pkg, ob):
    import make_paths_adaptive_golden as mk
    g, want = np.load(par.GOLDEN_LAMBERT), mk.lambert_arrays(pkg, ob)
    assert sorted(g.files) == sorted(want)
    _same(g, want, sorted(want))
    counts = g["counts"]
    print([(int(c.min()), int(c.max())) for c in counts], g["info"])
    assert par.is_real_schedule(counts) and [(int(c.min()), int(c.max())) for c in counts] == [(16, 16), (1, 20), (1, 19)]
    assert np.array_equal(g["records"]["sample_index"], counts.sum(axis=0)) and int(g["info"]["samples"]) == int(g["sample_count"].sum())
    assert g["radiance_sum"].min() >= 0 and g["radiance_sum"].max() > 0 and (g["records"]["mean"] == 0).any()      # background records
    assert os.path.getsize(par.GOLDEN_LAMBERT) < 1 << 20


@needs_cc
def test_nee_fixture_is_the_cpu_composite(pkg, ob):
    import make_paths_adaptive_golden as mk
    g, want = np.load(par.GOLDEN_NEE), mk.nee_arrays(pkg, ob)
    assert sorted(g.files) == sorted(want)
    _same(g, want, sorted(want))
    counts = g["counts"]
    print([(int(c.min()), int(c.max())) for c in counts], g["info"])
    assert par.is_real_schedule(counts) and [(int(c.min()), int(c.max())) for c in counts] == [(16, 16), (1, 37), (1, 31)]
    assert (int(g["info"]["passes_rendered"]), int(g["info"]["stopped_early"]), int(g["info"]["samples"])) == (3, 0, 14328)
    assert np.array_equal(g["records"]["sample_index"], counts.sum(axis=0)) and int(g["info"]["samples"]) == int(g["sample_count"].sum())
    assert g["radiance_sum"].max() > 0 and g["seg_count"].max() > 0 and (g["records"]["mean"] == 0).any()
    assert os.path.getsize(par.GOLDEN_NEE) < 1 << 20


# ---- the cases of the GPU tests, on the CPU composite: (case, bounces, scene fields, surface fields) -> counts per pass
NEE_CASES = {
    "mis_3": (("mis", 3, {}, {}), [(16, 16), (1, 37), (1, 31)]),
    "uni_2": (("uni", 2, {}, {}), [(16, 16), (1, 28), (1, 31)]),
    "colour_short_last_pass": (("mis-colour", 4, {"spp_count": 40}, {}), [(16, 16), (1, 32), (1, 13)]),
    "dark_6": (("mis-dark", 6, {}, {}), [(16, 16), (1, 37), (1, 29)]),
    "single_guided_4": (("single", 4, {}, {}), [(16, 16), (1, 21), (1, 30)]),
    "clamped_cap": (("mis", 3, {}, {"cap_radiance": 1e6}), None),
}
LAMBERT_CASES = {
    "C0_4": (("C0", 4, {}), [(16, 16), (1, 20), (1, 19)]),
    "C1_3": (("C1", 3, {}), [(16, 16), (1, 24), (1, 21)]),
    "clamped_light": (("C0", 4, {"light_radiance": 1e6}), None),
}


def _nee(pkg, ob, case, bounces, fields, surface_fields, scene=None):
    params, surf, _ = npr.CASES[case](pkg)
    surf = np.array(surf, dtype=pkg.SURFACE_S)
    for k, v in surface_fields.items():
        surf[k] = v
    return par.cpu_nee(pkg, ob, params, surf, par.scene(ob, **fields) if scene is None else scene, bounces)


@needs_cc
@pytest.mark.parametrize("name", sorted(NEE_CASES))
def test_nee_cases_on_the_cpu(pkg, ob, name):
    args, counts = NEE_CASES[name]
    ref = _nee(pkg, ob, *args)
    got = [(int(c.min()), int(c.max())) for c in ref["counts"]]
    print(name, ref["info"], "k_used", ref["k_used"], got)
    assert par.is_real_schedule(ref["counts"]) and ref["k_used"] <= 84 and ref["segs"].max() <= 3 * (args[1] - 1)
    if counts is None:
        assert par.assert_clamp_case(ref) == (34, 3889)
    else:
        par.assert_no_clamp(ref)
        assert got == counts


@needs_cc
@pytest.mark.parametrize("name", sorted(LAMBERT_CASES))
def test_lambert_cases_on_the_cpu(pkg, ob, name):
    (config, bounces, fields), counts = LAMBERT_CASES[name]
    ref = par.cpu_lambert(pkg, ob, pkg.params_for_config(config), par.scene(ob, **fields), bounces)
    got = [(int(c.min()), int(c.max())) for c in ref["counts"]]
    print(name, ref["info"], "k_used", ref["k_used"], got)
    assert par.is_real_schedule(ref["counts"]) and ref["k_used"] <= 84 and not ref["seg_count"].any()
    if counts is None:
        assert par.assert_clamp_case(ref) == (2160, 386)
    else:
        par.assert_no_clamp(ref)
        assert got == counts


@needs_cc
def test_smallest_frame_on_the_cpu(pkg, ob):
    """5 x 3: two clipped records; the plan step budgets 16 pixels per record, so the later passes have 8 samples per pixel"""
    small = par.scene(ob, 48, 5, 3, cam_pos=(0.0, 0.0, 4.0))
    ref = _nee(pkg, ob, "mis", 3, {}, {}, scene=small)
    assert ref["records"].shape == (1, 2) and int(ref["info"]["samples"]) == 480 and ref["radiance_sum"].max() > 0
    assert [sorted(set(c.reshape(-1).tolist())) for c in ref["counts"]] == [[16], [8], [8]]
    lam = par.cpu_lambert(pkg, ob, pkg.params_for_config("C0"), small, 3)
    assert lam["records"].shape == (1, 2) and int(lam["info"]["samples"]) % 64 != 0 and lam["radiance_sum"].max() > 0


@needs_cc
def test_one_bounce_on_the_cpu(pkg, ob):
    """max_path_bounces = 1: every sample is zero, and the plan step ends the frame after the first pass"""
    for ref in (_nee(pkg, ob, "mis", 1, {}, {}), par.cpu_lambert(pkg, ob, pkg.params_for_config("C0"), par.scene(ob), 1)):
        info = ref["info"]
        assert (int(info["passes_rendered"]), int(info["stopped_early"]), int(info["samples"])) == (1, 1, 4928)
        assert not ref["radiance_sum"].any() and not ref["seg_count"].any() and (ref["sample_count"] == 16).all()
