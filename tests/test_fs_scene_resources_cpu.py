"""Register, scratch and LDS budget of the function-space frame kernel, read from the code object inside libgpis_hip.so (no GPU
needed), in the pattern of tests/test_ws_paths_resources_cpu.py.  k_fs_scene keeps fs_sample_distance_one and
fs_transmittance_one in one kernel with the sample's ray, shade and sampler live across them; it must do so without VGPR spills
and within the 40 KB of LDS that let four one-wave workgroups share a CU (gpis_fs.hpp: the static_assert on FsLds).  Factoring
fs_sample_distance_one out of k_fs_march must not have cost that kernel scratch or LDS."""
import os

import pytest

import test_kernel_resources as res

# k_fs_march before fs_sample_distance_one was factored out of it (commit eb05482), same compiler and flags:
#   <false> (transmittance):  210 VGPRs, 0 B scratch, 37 488 B LDS
#   <true>  (sampleDistance): 227 VGPRs, 0 B scratch, 37 488 B LDS
PARENT_MARCH = {"ILb0E": {"private_segment_fixed_size": 0, "group_segment_fixed_size": 37488},
                "ILb1E": {"private_segment_fixed_size": 0, "group_segment_fixed_size": 37488}}


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_fs_scene_kernel_keeps_its_budget(pkg):
    k = res._kernels(pkg.library_path())
    scene = [v for n, v in k.items() if "k_fs_sceneILi0" in n]
    assert len(scene) == 1, sorted(k)
    v = scene[0]
    assert v["vgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] <= 40960, v
    assert any("k_fs_scene_sumILi0" in n for n in k)
    for inst, parent in PARENT_MARCH.items():
        march = [v for n, v in k.items() if "k_fs_march" + inst in n]
        assert len(march) == 1, (inst, sorted(k))
        for key, bound in parent.items():
            assert march[0][key] <= bound, (inst, key, march[0])
        assert march[0]["vgpr_spill_count"] == 0, march[0]
