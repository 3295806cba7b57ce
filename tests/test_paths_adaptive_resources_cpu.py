"""Resources of the kernels of gpis_render_scene_s_paths_adaptive and gpis_render_scene_s_nee_paths_adaptive, read from the code
object inside libgpis_hip.so (no GPU needed), in the pattern of tests/test_adaptive_paths_rgb_resources_cpu.py.  The camera step on
the records of a pass, the per-pixel sum and the tile statistics are small one-thread-per-item kernels around the bounce loop: no
scratch, no VGPR spill, no LDS, a few dozen VGPRs.  The drivers add nothing to the march kernels nor to the kernels of the Lambert
and NEE path drivers, and k_paths_begin, which now shares its body with the adaptive camera step, keeps the resources it had."""
import os

import pytest

import test_kernel_resources as res
from test_nee_paths_resources_cpu import MARCH_KERNELS_BEFORE
from test_paths_rgb_resources_cpu import PATHS_KERNELS_BEFORE, _tuple

NEW_KERNELS = ("k_paths_adaptive_begin", "k_paths_adaptive_sum", "k_paths_adaptive_tile_stats")
# (vgpr_count, private_segment_fixed_size, group_segment_fixed_size, vgpr_spill_count) in the library of the commit before
PATHS_BEGIN_BEFORE = (32, 0, 0, 0)
NEE_PATH_KERNELS = ("k_nee_paths_setup", "k_nee_paths_shade", "k_nee_paths_gather", "k_scene_sum_u32")


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_paths_adaptive_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    for name in NEW_KERNELS:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "adaptive" in n))
        v = hits[0]
        print(name, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 64, (name, v)
    begin = [v for n, v in k.items() if n.startswith("_Z13k_paths_begin")]
    assert len(begin) == 1 and _tuple(begin[0]) == PATHS_BEGIN_BEFORE, begin
    for prefix, want in list(MARCH_KERNELS_BEFORE.items()) + list(PATHS_KERNELS_BEFORE.items()):
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        assert _tuple(hits[0]) == want, (prefix, _tuple(hits[0]), want)
    for name in NEE_PATH_KERNELS:
        assert len([n for n in k if name in n]) == 1, name
