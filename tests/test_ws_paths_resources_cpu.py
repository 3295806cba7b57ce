"""Register budget of the weight-space path kernel, read from the code object inside libgpis_hip.so (no GPU needed), in the
pattern of tests/test_kernel_resources.py.  k_ws_paths keeps ws_sample_distance and ws_transmittance_one inside the bounce loop
with the whole path state live across them; it must stay within 256 VGPRs without VGPR spills and one WsLds of LDS, which admits
two waves per SIMD as k_ws_scene has."""
import os

import pytest

import test_kernel_resources as res


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_ws_paths_kernel_keeps_its_budget(pkg):
    k = res._kernels(pkg.library_path())
    paths = [v for n, v in k.items() if "k_ws_pathsILi0" in n]
    scene = [v for n, v in k.items() if "k_ws_sceneILi0" in n]
    assert len(paths) == 1 and len(scene) == 1, sorted(k)
    v = paths[0]
    assert v["vgpr_count"] <= 256 and v["vgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] == scene[0]["group_segment_fixed_size"], (v, scene[0])      # one WsLds, as k_ws_scene
    assert any("k_ws_paths_sumILi0" in n for n in k)
