"""Resources of the kernels of gpis_render_scene_s_material_paths_rgb and its adaptive form, read from the code object inside
libgpis_hip.so (no GPU needed), in the pattern of tests/test_adaptive_paths_rgb_resources_cpu.py.  The set-up and the shade kernel
switch per lane between the conductor and the Lambert step; the material table is a kernel argument read with constant indices, so
neither kernel has scratch, a VGPR spill or LDS.  The drivers add nothing to any kernel of the parent: the march kernels, the
Lambert and conductor path kernels and the RGB conductor kernels keep their figures
(profiles/r22_material_paths_resources.json holds the table of every kernel before and after)."""
import json
import os

import pytest

import test_kernel_resources as res
from test_nee_paths_resources_cpu import MARCH_KERNELS_BEFORE
from test_nee_paths_rgb_resources_cpu import NEE_KERNELS_BEFORE
from test_paths_rgb_resources_cpu import PATHS_KERNELS_BEFORE, _tuple

NEW_KERNELS = ("k_mat_rgb_setup", "k_mat_rgb_shade")
# (vgpr_count, private_segment_fixed_size, group_segment_fixed_size, vgpr_spill_count) in the library of the commit before
COND_RGB_KERNELS_BEFORE = {
    "_Z16k_cond_rgb_setup": (84, 0, 0, 0),
    "_Z15k_cond_rgb_emit": (11, 0, 0, 0),
    "_Z16k_cond_rgb_shade": (70, 0, 0, 0),
    "_Z17k_cond_rgb_gather": (12, 0, 0, 0),
}
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22_material_paths_resources.json")


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_material_paths_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    for name in NEW_KERNELS:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(n for n in k if "mat_rgb" in n))
        v = hits[0]
        print(name, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 128, (name, v)          # 256 threads per workgroup at 4 waves per SIMD and more
    assert len([n for n in k if "mat_rgb" in n]) == len(NEW_KERNELS)
    before = list(MARCH_KERNELS_BEFORE.items()) + list(PATHS_KERNELS_BEFORE.items()) + list(NEE_KERNELS_BEFORE.items()) + list(COND_RGB_KERNELS_BEFORE.items())
    for prefix, want in before:
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        assert _tuple(hits[0]) == want, (prefix, _tuple(hits[0]), want)


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_every_kernel_of_the_parent_keeps_its_figures(pkg):
    """the recorded table: nothing moved, nothing removed, and the library is the table's `after`"""
    rec = json.load(open(TABLE))
    k = {n: [int(v[c]) for c in rec["columns"]] for n, v in res._kernels(pkg.library_path()).items()}
    assert rec["moved"] == {} and rec["removed"] == [] and sorted(rec["new"]) == sorted(n for n in k if "mat_rgb" in n)
    assert rec["kernels_after"] == len(k) == rec["kernels_before"] + len(NEW_KERNELS)
    for name, want in list(rec["unchanged"].items()) + list(rec["new"].items()):
        assert k.get(name) == want, (name, k.get(name), want)
