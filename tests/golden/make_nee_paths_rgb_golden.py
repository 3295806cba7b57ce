"""Writes tests/golden/nee_paths_rgb_small.npz: per case of tests/nee_paths_rgb_ref.py the inputs (medium parameters, RGB surface,
scene) and the CPU composite's image and per-pixel segment counts at max_path_bounces = 4 on the 22 x 15 x 3 frame, and for the
emissive case its first-hit frame (max_path_bounces = 1) too.

    python tests/golden/make_nee_paths_rgb_golden.py

tests/test_nee_paths_rgb_cpu.py regenerates the arrays and compares; tests/test_gpu_nee_paths_rgb.py renders the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def arrays(pkg, ob):
    import nee_paths_rgb_ref as rgb
    out = {"scene": np.array(rgb.frame(ob), dtype=pkg.SCENE_S), "max_path_bounces": np.array(rgb.GOLDEN_BOUNCES, dtype=np.int32)}
    for name in sorted(rgb.CASES):
        params, surf = rgb.CASES[name](pkg)
        c = rgb.reference(pkg, ob, name, rgb.GOLDEN_BOUNCES)
        out[name + "/params"] = np.array(params, dtype=pkg.PARAMS)
        out[name + "/surface"] = np.array(surf, dtype=pkg.SURFACE_RGB_S)
        out[name + "/image"] = np.array(c.image)
        out[name + "/seg_count"] = np.array(c.seg_count)
    first = rgb.reference(pkg, ob, rgb.EMISSIVE_CASE, 1)
    out["first_hit/image"] = np.array(first.image)
    out["first_hit/seg_count"] = np.array(first.seg_count)
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import nee_paths_rgb_ref as rgb
    ob.build()
    np.savez_compressed(rgb.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(rgb.GOLDEN, os.path.getsize(rgb.GOLDEN), "bytes")
