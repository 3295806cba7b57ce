"""Resources of the kernels of gpis_render_scene_s_nee_paths_rgb and its adaptive form, read from the code object inside
libgpis_hip.so (no GPU needed), in the pattern of tests/test_nee_paths_resources_cpu.py.  The set-up, emission add, shade and gather
kernels are small one-thread-per-sample kernels between the medium's launches: no scratch, no VGPR spill, no LDS.  The drivers add
nothing to the march kernels or to the mono and Lambert path kernels: their entries are the ones the library had before
(profiles/r21_nee_paths_rgb_resources.json holds the table of every kernel before and after)."""
import os

import pytest

import test_kernel_resources as res
from test_nee_paths_resources_cpu import MARCH_KERNELS_BEFORE
from test_paths_rgb_resources_cpu import PATHS_KERNELS_BEFORE, _tuple

NEW_KERNELS = ("k_cond_rgb_setup", "k_cond_rgb_emit", "k_cond_rgb_shade", "k_cond_rgb_gather")
# the mono conductor kernels whose sample functions now take the channel count: (vgpr_count, private_segment_fixed_size,
# group_segment_fixed_size, vgpr_spill_count) in the library of the commit before
NEE_KERNELS_BEFORE = {
    "_Z11k_nee_setup": (70, 0, 0, 0),
    "_Z11k_nee_shade": (60, 0, 0, 0),
    "_Z12k_nee_gather": (6, 0, 0, 0),
    "_Z17k_nee_paths_setup": (74, 0, 0, 0),
    "_Z17k_nee_paths_shade": (64, 0, 0, 0),
    "_Z18k_nee_paths_gather": (10, 0, 0, 0),
}


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_nee_paths_rgb_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    for name in NEW_KERNELS:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "cond_rgb" in n))
        v = hits[0]
        print(name, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 128, (name, v)          # 256 threads per workgroup at 4 waves per SIMD and more
    assert len([n for n in k if "cond_rgb" in n]) == len(NEW_KERNELS)
    for prefix, want in list(MARCH_KERNELS_BEFORE.items()) + list(PATHS_KERNELS_BEFORE.items()) + list(NEE_KERNELS_BEFORE.items()):
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        assert _tuple(hits[0]) == want, (prefix, _tuple(hits[0]), want)
