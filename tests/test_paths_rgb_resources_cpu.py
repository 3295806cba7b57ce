"""Resources of the kernels of gpis_render_scene_s_paths_rgb, read from the code object inside libgpis_hip.so (no GPU needed), in the
pattern of tests/test_nee_paths_resources_cpu.py.  The begin, shade, NEE add, accumulate and count kernels are small
one-thread-per-sample (or per-pixel) kernels between the medium's launches: no VGPR spill, no LDS, at most 128 VGPRs, and no
scratch — except that the shade kernel calls the out-of-line fbm of field_vec for a sandstone / rust emission and may carry what
k_mean_color_emission carries for the same call.  The driver adds nothing to the march kernels nor to the kernels of
gpis_render_scene_s_paths: their entries are the ones the library had before the driver existed."""
import os

import pytest

import test_kernel_resources as res
from test_nee_paths_resources_cpu import MARCH_KERNELS_BEFORE

# kernel name -> (vgpr_count, private_segment_fixed_size, group_segment_fixed_size, vgpr_spill_count), read from the library of the
# commit BEFORE this driver was added (the march kernels: MARCH_KERNELS_BEFORE, which that library still matched).
PATHS_KERNELS_BEFORE = {
    "_Z12k_paths_keys": (25, 0, 0, 0),
    "_Z13k_paths_begin": (32, 0, 0, 0),
    "_Z13k_paths_shade": (62, 0, 0, 0),
    "_Z14k_paths_gather": (36, 0, 0, 0),
    "_Z15k_paths_nee_add": (6, 0, 0, 0),
    "_Z18k_paths_accumulate": (14, 0, 0, 0),
}
# k_paths_rgb_beginIm: the instance on the uniform sample layout (size_t first pixel); k_scene_sum_u32: the per-pixel segment count
NEW_KERNELS = ("k_paths_rgb_beginIm", "k_paths_rgb_shade", "k_paths_rgb_nee_add", "k_paths_rgb_accumulate", "k_scene_sum_u32")


def _tuple(v):
    return (v["vgpr_count"], v["private_segment_fixed_size"], v["group_segment_fixed_size"], v["vgpr_spill_count"])


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_paths_rgb_kernels_and_the_kernels_before(pkg):
    k = res._kernels(pkg.library_path())
    field = [v for n, v in k.items() if "k_mean_color_emission" in n]
    assert len(field) == 1
    for name in NEW_KERNELS:
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(k))
        v = hits[0]
        assert v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 128, (name, v)          # 256 threads per workgroup at 4 waves per SIMD and more
        allowed = field[0]["private_segment_fixed_size"] if name == "k_paths_rgb_shade" else 0
        assert v["private_segment_fixed_size"] <= allowed, (name, v, allowed)
    for prefix, want in list(MARCH_KERNELS_BEFORE.items()) + list(PATHS_KERNELS_BEFORE.items()):
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        assert _tuple(hits[0]) == want, (prefix, _tuple(hits[0]), want)
