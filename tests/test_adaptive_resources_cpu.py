"""Resources of the kernels of gpis_render_scene_s_adaptive, read from the code object inside libgpis_hip.so (no GPU needed), in the
pattern of tests/test_paths_rgb_resources_cpu.py.  The two camera steps, the per-pixel sum and the tile statistics are small
one-thread-per-item kernels between the medium's launches: no scratch, no VGPR spill, no LDS, a few dozen VGPRs.  The driver adds
nothing to the march kernels nor to the kernels of the Lambert path drivers: their entries are the ones the library had before."""
import os

import pytest

import test_kernel_resources as res
from test_nee_paths_resources_cpu import MARCH_KERNELS_BEFORE
from test_paths_rgb_resources_cpu import PATHS_KERNELS_BEFORE, _tuple

# the two camera steps are the instances of k_scene_primary / k_scene_primary_c on the variable-count layout (AdaptiveChunk)
NEW_KERNELS = ("k_scene_primaryIN4gpis13AdaptiveChunkE", "k_scene_primary_cIN4gpis13AdaptiveChunkE", "k_adaptive_accumulate", "k_adaptive_stats")


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_adaptive_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    for name in NEW_KERNELS:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "adaptive" in n))
        v = hits[0]
        print(name, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 64, (name, v)
    for prefix, want in list(MARCH_KERNELS_BEFORE.items()) + list(PATHS_KERNELS_BEFORE.items()):
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        assert _tuple(hits[0]) == want, (prefix, _tuple(hits[0]), want)
