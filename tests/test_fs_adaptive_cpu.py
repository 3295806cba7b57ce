"""The function-space adaptive drivers without a GPU: the entries are declared, bound and exported; the recorded fixture
tests/golden/fs_adaptive_small.npz is what the CPU composite (tests/fs_adaptive_ref.py) gives today, bit for bit, and its schedule
is a real one; every case of the GPU tests has such a schedule and holds every class of segment (a miss, an exit, a hit, a visible
and an occluded shadow segment); the clamp cases do clamp; and the early-stop cases are all zero on the CPU too."""
import ctypes
import os
import re

import numpy as np
import pytest

import fs_adaptive_ref as fa
import fs_scene_ref

ENTRIES = ("gpis_fs_render_scene_s_adaptive", "gpis_fs_render_scene_s_paths_adaptive")
needs_cc = pytest.mark.skipif(not fa.ws_oracle.available(), reason="no C compiler for the restatements")


@pytest.fixture(scope="module")
def cpu(pkg, ob):
    return fa.CpuRenderer(pkg, ob)


def test_entries_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(fa.ws_oracle.ROOT, "include", "gpis.h")).read()
    lib = ctypes.CDLL(pkg.library_path())
    for name in ENTRIES:
        assert re.search(r"^(?:extern )?int %s\(" % name, header, flags=re.M), name
        assert name in pkg.GpisLib.SYMBOLS, name
        assert getattr(lib, name) is not None
    for method in ("fs_render_scene_s_adaptive", "fs_render_scene_s_paths_adaptive"):
        assert callable(getattr(pkg.Medium, method))


@needs_cc
def test_fixture_is_the_cpu_composite(pkg, ob, cpu):
    g = np.load(fa.GOLDEN)
    want = fa.golden_arrays(pkg, ob, cpu)
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        a, b = np.ascontiguousarray(g[k]), np.ascontiguousarray(v)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    for tag in ("lambert", "paths"):
        fa.check_schedule({"counts": g[tag + "_counts"]})
        assert g[tag + "_radiance_sum"].max() > 0
        # the image's counts are the schedule's, tile by tile
        per_tile = g[tag + "_counts"].sum(axis=0)
        assert np.array_equal(g[tag + "_sample_count"], np.repeat(np.repeat(per_tile, 4, axis=0), 4, axis=1)[:fa.H, :fa.W])
        assert np.array_equal(g[tag + "_records"]["sample_index"], per_tile)
    # hits are at most one per sample; the path driver's count is segments, more than one per sample somewhere
    assert 0 < g["lambert_hit_count"].max() and (g["lambert_hit_count"] <= g["lambert_sample_count"]).all()
    assert (g["paths_hit_count"] > g["paths_sample_count"]).any()


@needs_cc
@pytest.mark.parametrize("name", sorted(dict(fa.CASES, **fa.CASES_64)))
def test_every_case_has_a_real_schedule_and_every_class(pkg, ob, cpu, name):
    driver, p, sc = fa.case_inputs(pkg, ob, name)
    ref = cpu.frame(driver, p, sc)
    c = ref["classes"]
    print(name, ref["info"], "k_used", ref["k_used"], [(int(x.min()), int(x.max())) for x in ref["counts"]],
          "miss / exit / hit / visible / occluded", c.n_miss, c.n_exit, c.n_hit, c.n_visible, c.n_occluded)
    fa.check_case_schedule(name, ref)
    fs_scene_ref.assert_non_vacuous(c)
    assert ref["largest_value"] <= 65536
    if int(sc["spp_count"]) == 40:
        assert int(ref["info"]["samples"]) < fa.W * fa.H * 40            # the short last pass


@needs_cc
@pytest.mark.parametrize("name", sorted(fa.CLAMP_CASES))
def test_clamp_cases_clamp(pkg, ob, cpu, name):
    driver, p, sc = fa.case_inputs(pkg, ob, name)
    ref = cpu.frame(driver, p, sc)
    print(name, ref["info"], "largest value", ref["largest_value"], "image max", float(ref["radiance_sum"].max()))
    fs_scene_ref.assert_non_vacuous(ref["classes"])
    assert ref["largest_value"] > 65536 and ref["radiance_sum"].max() > 0


@needs_cc
@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_all_zero_samples_stop_after_the_first_pass(pkg, ob, cpu, driver):
    """a light that faces away from every normal the camera sees for the frame driver (hits, no lit sample), one bounce for the path
    driver (a segment per sample that meets the bound, no next-event estimation)"""
    p = fa.medium(pkg)
    sc = fa.scene(ob, **(fa.DARK if driver == "lambert" else {}))
    ref = cpu.frame(driver, p, sc, bounces=1)
    assert (int(ref["info"]["passes_rendered"]), int(ref["info"]["stopped_early"]), int(ref["info"]["samples"])) == (1, 1, fa.W * fa.H * 16)
    assert (ref["radiance_sum"] == 0).all() and (ref["sample_count"] == 16).all() and ref["hit_count"].max() > 0
