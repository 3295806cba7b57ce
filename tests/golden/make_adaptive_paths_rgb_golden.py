"""Writes tests/golden/adaptive_paths_rgb_small.npz: the inputs (medium parameters, scene, adaptive settings, albedo, bounces) and
the result of the restated adaptive RGB path frame (tests/adaptive_paths_rgb_ref.py) on the 22 x 14 frame at 48 spp, with the
per-sample values of the CPU composite of gpis_render_scene_s_paths_rgb (tests/paths_rgb_ref.py): image, sample and segment counts,
records, info and the per-pass sample counts.

    python tests/golden/make_adaptive_paths_rgb_golden.py

tests/test_adaptive_paths_rgb_cpu.py regenerates the arrays and compares; tests/test_gpu_adaptive_paths_rgb.py renders the recorded
inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def arrays(pkg, ob):
    import adaptive_paths_rgb_ref as apr
    import adaptive_ref as ar
    params, albedo, scene, adaptive = apr.small_inputs(pkg, ob)
    out = {"params": np.array(params, dtype=pkg.PARAMS), "scene": np.array(scene, dtype=pkg.SCENE_S), "adaptive": np.array(adaptive, dtype=ar.ADAPTIVE_S),
           "albedo": albedo, "max_bounces": np.int32(apr.SMALL_BOUNCES)}
    ref = apr.small_reference(pkg, ob)
    for k in apr.KEYS + ("counts",):
        out[k] = np.array(ref[k])
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import adaptive_paths_rgb_ref as apr
    np.savez_compressed(apr.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(apr.GOLDEN, os.path.getsize(apr.GOLDEN), "bytes")
