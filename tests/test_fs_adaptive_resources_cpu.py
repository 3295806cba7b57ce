"""Resources of the kernels of gpis_fs_render_scene_s_adaptive and gpis_fs_render_scene_s_paths_adaptive, read from the code object
inside libgpis_hip.so (no GPU needed), in the pattern of tests/test_paths_adaptive_resources_cpu.py.  The two fused kernels share
their bodies with k_fs_scene and k_fs_paths, which sit at the edge of their register budget: the new ones must not spill a VGPR and
must keep the one FsLds that lets four one-wave workgroups share a CU, and the kernels of the commit before keep what they had —
no scratch, 37 488 B of LDS, no VGPR spill and the same VGPR count.  The weight-space adaptive kernels, whose sum and statistics
now share their bodies with this medium's (gpis_frame_sum.hpp), are still there once each."""
import os

import pytest

import test_kernel_resources as res

NEW_FUSED = ("k_fs_scene_adaptiveILi0", "k_fs_paths_adaptiveILi0")
NEW_SMALL = ("k_fs_adaptive_sum", "k_fs_adaptive_stats")              # one instance per driver
# (vgpr_count, private_segment_fixed_size, group_segment_fixed_size, vgpr_spill_count) in the library of the commit before; the
# count of k_fs_paths includes its accumulation registers (256 + 35)
BEFORE = {
    "k_fs_marchILb0E": (210, 0, 37488, 0),
    "k_fs_marchILb1E": (221, 0, 37488, 0),
    "k_fs_sceneILi0": (261, 0, 37488, 0),
    "k_fs_pathsILi0": (291, 0, 37488, 0),
}
WS_ADAPTIVE = {"k_ws_scene_adaptiveILi0": 1, "k_ws_paths_adaptiveILi0": 1, "k_ws_adaptive_sum": 2, "k_ws_adaptive_stats": 2}


def _tuple(v):
    return (v["vgpr_count"], v["private_segment_fixed_size"], v["group_segment_fixed_size"], v["vgpr_spill_count"])


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_fs_adaptive_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    for name in NEW_FUSED:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "k_fs_" in n))
        v = hits[0]
        print(name, v)
        assert v["vgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] <= 40960, (name, v)
        assert v["private_segment_fixed_size"] == 0, (name, v)          # as the uniform siblings: no scratch
    for name in NEW_SMALL:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 2, (name, sorted(n for n in k if "k_fs_adaptive" in n))
        for v in hits:
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= 64, (name, v)
    for inst, want in BEFORE.items():
        hits = [v for n, v in k.items() if inst in n]
        assert len(hits) == 1, (inst, sorted(n for n in k if "k_fs_" in n))
        assert _tuple(hits[0]) == want, (inst, _tuple(hits[0]), want)
    for name, count in WS_ADAPTIVE.items():
        assert len([n for n in k if name in n]) == count, (name, sorted(n for n in k if "k_ws_" in n))
