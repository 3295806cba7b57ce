"""The compact body of the Lambert frame driver ("Wavefront driver"; GPIS_OPT_SCENE_COMPACT): its two march instances
read and write 32-byte records (gpis_scene.hpp: SceneRay, SceneHit) where the instances they replace read gpis_ray_in and write
gpis_seg_out.  Checked here without a GPU: the new instances cost no scratch, no LDS and no occupancy.  The record sizes are a static_assert in gpis_scene.hpp: a library that
loads has 32-byte records."""
import os
import re

import pytest

from test_kernel_resources import LLVM, _kernels

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparse-conv-gpis-tungsten_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
@pytest.mark.parametrize("new, old", [("k_guided_sample_distance_scene", "k_guided_sample_distance_noexit"),
                                      ("k_guided_transmittance_scene", "k_guided_transmittance")])
def test_scene_instances_keep_the_budget(pkg, new, old):
    """no more scratch, no more LDS and no lower occupancy (VGPR allocation granule of 8, 512 per SIMD) than the instance replaced,
    for both SMALLARG values"""
    k = _kernels(pkg.library_path())
    for small_arg in ("ILb0E", "ILb1E"):
        a = [v for n, v in k.items() if old + small_arg in n]
        b = [v for n, v in k.items() if new + small_arg in n]
        assert len(a) == 1 and len(b) == 1, (small_arg, sorted(k))
        a, b = a[0], b[0]
        print(new + small_arg, b, "replaces", a)
        waves = lambda v: 512 // (8 * ((v["vgpr_count"] + 7) // 8))
        assert b["private_segment_fixed_size"] <= a["private_segment_fixed_size"], (a, b)
        assert waves(b) >= waves(a), (a, b)
        assert b["group_segment_fixed_size"] <= a["group_segment_fixed_size"], (a, b)


def test_scene_instances_stay_out_of_the_old_budget_checks(pkg):
    """test_kernel_resources.py finds the batch instances by the start of their mangled names: the new ones must not match"""
    k = _kernels(pkg.library_path())
    scene = [n for n in k if "_scene" in n and "k_guided_" in n]
    assert len(scene) == 4, scene
    for n in scene:
        assert "k_guided_sample_distanceILb" not in n and "k_guided_transmittanceILb" not in n, n


def test_option_is_on_by_default_in_header_and_bindings(pkg):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "gpis.h")).read()
    assert re.search(r"GPIS_OPT_SCENE_COMPACT = 10,", hdr)
    assert pkg.Medium.OPTIONS["scene_compact"] == 10
