"""Resources of the kernels of gpis_render_scene_s_nee_paths, read from the code object inside libgpis_hip.so (no GPU needed), in the
pattern of tests/test_ws_paths_resources_cpu.py.  The set-up, shade, gather and count kernels of the path driver are small
one-thread-per-sample kernels between the medium's launches: no VGPR spill, no scratch, no LDS.  The driver adds nothing to the
march kernels, the neePDF / neeGrad kernels included: their entries are the ones the library had before the driver existed."""
import os

import pytest

import test_kernel_resources as res

# kernel name (the prefix that tells it from every other kernel) -> (vgpr_count, private_segment_fixed_size,
# group_segment_fixed_size, vgpr_spill_count), read from the library of the commit BEFORE the path driver was added.
MARCH_KERNELS_BEFORE = {
    "_ZN4gpis11k_wave_evalILb0": (96, 0, 4096, 0),
    "_ZN4gpis11k_wave_evalILb1": (96, 0, 4096, 0),
    "_ZN4gpis11k_wave_gradILb0": (102, 0, 4096, 0),
    "_ZN4gpis11k_wave_gradILb1": (102, 0, 4096, 0),
    "_ZN4gpis11k_wave_stepILb0": (122, 0, 0, 0),
    "_ZN4gpis11k_wave_stepILb1": (120, 0, 0, 0),
    "_ZN4gpis11k_wave_tailILb0": (123, 0, 4544, 0),
    "_ZN4gpis11k_wave_tailILb1": (123, 0, 4544, 0),
    "_ZN4gpis15k_persist_marchINS_16spec_3d_multires7PersistELb0": (149, 0, 12784, 0),
    "_ZN4gpis15k_persist_marchINS_16spec_3d_multires7PersistELb1": (153, 0, 12784, 0),
    "_ZN4gpis15k_persist_marchINS_7generic7PersistELb0": (168, 416, 12784, 257),
    "_ZN4gpis15k_persist_marchINS_7generic7PersistELb1": (168, 464, 12784, 334),
    "_ZN4gpis15k_persist_marchINS_7spec_1d7PersistELb0": (168, 12, 12784, 26),
    "_ZN4gpis15k_persist_marchINS_7spec_1d7PersistELb1": (168, 12, 12784, 26),
    "_ZN4gpis15k_persist_marchINS_7spec_3d7PersistELb0": (124, 0, 12784, 0),
    "_ZN4gpis15k_persist_marchINS_7spec_3d7PersistELb1": (138, 0, 12784, 0),
    "_ZN4gpis15k_transmittanceINS_1": (128, 828, 0, 252),
    "_ZN4gpis15k_transmittanceINS_7g": (128, 1008, 0, 99),
    "_ZN4gpis15k_transmittanceINS_7spec_1": (128, 1580, 0, 474),
    "_ZN4gpis15k_transmittanceINS_7spec_3": (128, 600, 0, 171),
    "_ZN4gpis16k_wave_finish_s": (48, 0, 0, 0),
    "_ZN4gpis16k_wave_finish_t": (9, 0, 0, 0),
    "_ZN4gpis16k_wave_gra": (34, 0, 0, 0),
    "_ZN4gpis17k_guided_range_sdILb0": (128, 116, 4096, 50),
    "_ZN4gpis17k_guided_range_sdILb1": (128, 116, 4096, 50),
    "_ZN4gpis17k_guided_range_trILb0": (96, 228, 4096, 112),
    "_ZN4gpis17k_guided_range_trILb1": (96, 228, 4096, 112),
    "_ZN4gpis17k_sample_distanceINS_1": (128, 1312, 0, 827),
    "_ZN4gpis17k_sample_distanceINS_7g": (128, 1120, 0, 362),
    "_ZN4gpis17k_sample_distanceINS_7spec_1": (128, 2108, 0, 1214),
    "_ZN4gpis17k_sample_distanceINS_7spec_3": (128, 660, 0, 344),
    "_ZN4gpis19k_guided_range_gradILb0": (116, 0, 4096, 0),
    "_ZN4gpis19k_guided_range_gradILb1": (116, 0, 4096, 0),
    "_ZN4gpis20k_fast_tra": (110, 0, 4096, 0),
    "_ZN4gpis22k_fast_sam": (124, 0, 4096, 0),
    "_ZN4gpis22k_guided_transmittanceILb0": (96, 284, 4096, 98),
    "_ZN4gpis22k_guided_transmittanceILb1": (96, 280, 4096, 96),
    "_ZN4gpis24k_guided_sample_distanceILb0": (96, 364, 4096, 128),
    "_ZN4gpis24k_guided_sample_distanceILb1": (96, 364, 4096, 128),
    "_ZN4gpis31k_guided_sample_distance_nogradILb0": (96, 364, 4096, 128),
    "_ZN4gpis31k_guided_sample_distance_nogradILb1": (96, 364, 4096, 128),
    "_ZN4gpis5k_neeINS_7g": (137, 32, 0, 0),
    "_ZN4gpis5k_neeINS_7s": (102, 0, 0, 0),
}


@pytest.mark.skipif(not os.path.exists(os.path.join(res.LLVM, "clang-offload-bundler")), reason="LLVM tools of the ROCm image")
def test_nee_paths_kernels_and_the_march_kernels(pkg):
    k = res._kernels(pkg.library_path())
    for name in ("k_nee_paths_setup", "k_nee_paths_shade", "k_nee_paths_gather", "k_scene_sum_u32"):
        hits = [v for n, v in k.items() if name in n]
        assert len(hits) == 1, (name, sorted(k))
        v = hits[0]
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= 128, (name, v)          # 256 threads per workgroup at 4 waves per SIMD and more
    for prefix, want in MARCH_KERNELS_BEFORE.items():
        hits = [v for n, v in k.items() if n.startswith(prefix)]
        assert len(hits) == 1, prefix
        v = hits[0]
        got = (v["vgpr_count"], v["private_segment_fixed_size"], v["group_segment_fixed_size"], v["vgpr_spill_count"])
        assert got == want, (prefix, got, want)
