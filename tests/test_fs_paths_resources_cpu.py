"""Register, scratch and LDS budget of the function-space path kernel, read from the code object inside libgpis_hip.so (no GPU
needed), in the pattern of tests/test_fs_scene_resources_cpu.py.  k_fs_paths keeps fs_sample_distance_one and
fs_transmittance_one inside the bounce loop with the whole path (ray, sampler, throughput, emission, the template of the next
ray) live across them; it must do so without VGPR spills and within the 40 KB of LDS that let four one-wave workgroups share a
CU.  Being the third kernel over the shared march code must not have cost k_fs_march or k_fs_scene scratch or LDS."""
import os

import pytest

import test_kernel_resources as res

# the kernels of the parent commit (caeaf06), same compiler and flags:
#   k_fs_march<false> (transmittance):  210 VGPRs, 0 B scratch, 37 488 B LDS, no VGPR spills
#   k_fs_march<true>  (sampleDistance): 221 VGPRs, 0 B scratch, 37 488 B LDS, no VGPR spills
#   k_fs_scene:                         261 VGPRs, 0 B scratch, 37 488 B LDS, no VGPR spills
PARENT = {"k_fs_marchILb0E": {"private_segment_fixed_size": 0, "group_segment_fixed_size": 37488},
          "k_fs_marchILb1E": {"private_segment_fixed_size": 0, "group_segment_fixed_size": 37488},
          "k_fs_sceneILi0": {"private_segment_fixed_size": 0, "group_segment_fixed_size": 37488}}


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_fs_paths_kernel_keeps_its_budget(pkg):
    k = res._kernels(pkg.library_path())
    paths = [v for n, v in k.items() if "k_fs_pathsILi0" in n]
    assert len(paths) == 1, sorted(k)
    v = paths[0]
    assert v["vgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] <= 40960, v
    assert any("k_fs_paths_sumILi0" in n for n in k)
    for inst, parent in PARENT.items():
        old = [v for n, v in k.items() if inst in n]
        assert len(old) == 1, (inst, sorted(k))
        for key, bound in parent.items():
            assert old[0][key] <= bound, (inst, key, old[0])
        assert old[0]["vgpr_spill_count"] == 0, old[0]
