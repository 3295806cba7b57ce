"""The weight-space adaptive drivers without a GPU: the entries are declared, bound and exported; the recorded fixture
tests/golden/ws_adaptive_small.npz is what the CPU composite (tests/ws_adaptive_ref.py) gives today, bit for bit, and its schedule
is a real one; every case of the GPU tests has such a schedule; and the two new fused kernels keep the budget of the ones they share
their bodies with (in the pattern of tests/test_ws_paths_resources_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_kernel_resources as res
import ws_adaptive_ref as wa

ENTRIES = ("gpis_ws_render_scene_s_adaptive", "gpis_ws_render_scene_s_paths_adaptive")
needs_cc = pytest.mark.skipif(not wa.ws_oracle.available(), reason="no C compiler for the restatements")


@pytest.fixture(scope="module")
def cpu(pkg, ob):
    return wa.CpuRenderer(pkg, ob)


def test_entries_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(wa.ws_oracle.ROOT, "include", "gpis.h")).read()
    lib = ctypes.CDLL(pkg.library_path())
    for name in ENTRIES:
        assert re.search(r"^(?:extern )?int %s\(" % name, header, flags=re.M), name
        assert name in pkg.GpisLib.SYMBOLS, name
        assert getattr(lib, name) is not None
    for method in ("render_scene_s_adaptive", "render_scene_s_paths_adaptive"):
        assert callable(getattr(pkg.WeightSpaceMedium, method))


@needs_cc
def test_fixture_is_the_cpu_composite(pkg, ob, cpu):
    g = np.load(wa.GOLDEN)
    want = wa.golden_arrays(pkg, ob, cpu)
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        a, b = np.ascontiguousarray(g[k]), np.ascontiguousarray(v)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    for tag in ("lambert", "paths"):
        wa.check_schedule({"counts": g[tag + "_counts"]})
        assert g[tag + "_radiance_sum"].max() > 0
        # the image's counts are the schedule's, tile by tile
        per_tile = g[tag + "_counts"].sum(axis=0)
        assert np.array_equal(g[tag + "_sample_count"], np.repeat(np.repeat(per_tile, 4, axis=0), 4, axis=1)[:wa.H, :wa.W])
        assert np.array_equal(g[tag + "_records"]["sample_index"], per_tile)
    assert g["lambert_hit_count"].max() > 0 and not g["paths_hit_count"].any()


@needs_cc
@pytest.mark.parametrize("name", sorted(wa.CASES))
def test_every_case_has_a_real_schedule(pkg, ob, cpu, name):
    driver, p, w, sc = wa.case_inputs(pkg, ob, name)
    ref = cpu.frame(driver, p, w, sc)
    print(name, ref["info"], "k_used", ref["k_used"], [(int(c.min()), int(c.max())) for c in ref["counts"]])
    wa.check_schedule(ref)
    assert ref["largest_value"] <= 65536
    if int(sc["spp_count"]) == 40:
        assert int(ref["info"]["samples"]) < wa.W * wa.H * 40            # the short last pass


@needs_cc
@pytest.mark.parametrize("name", sorted(wa.CLAMP_CASES))
def test_clamp_cases_clamp(pkg, ob, cpu, name):
    driver, p, w, sc = wa.case_inputs(pkg, ob, name)
    ref = cpu.frame(driver, p, w, sc)
    print(name, ref["info"], "largest value", ref["largest_value"], "image max", float(ref["radiance_sum"].max()))
    assert ref["largest_value"] > 65536 and ref["radiance_sum"].max() > 0


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_adaptive_ws_kernels_keep_the_budget(pkg):
    k = res._kernels(pkg.library_path())
    scene = [v for n, v in k.items() if "k_ws_sceneILi0" in n]
    paths = [v for n, v in k.items() if "k_ws_pathsILi0" in n]
    assert len(scene) == 1 and len(paths) == 1, sorted(k)                # the existing kernels are still one each
    for name in ("k_ws_scene_adaptiveILi0", "k_ws_paths_adaptiveILi0"):
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "k_ws_" in n))
        v = hits[0]
        print(name, v)
        assert v["vgpr_count"] <= 256 and v["vgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == scene[0]["group_segment_fixed_size"], (name, v, scene[0])      # one WsLds
    for name in ("k_ws_adaptive_sum", "k_ws_adaptive_stats"):            # one instance per driver, small and without scratch or LDS
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 2, (name, sorted(n for n in k if "k_ws_adaptive" in n))
        for v in hits:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= 64, (name, v)
