"""Writes tests/golden/nee_paths_small.npz: per case of tests/nee_paths_ref.py the inputs (medium parameters, surface, scene) and
the CPU composite's image and per-pixel segment counts at max_path_bounces = 4 on the 24 x 20 x 3 frame.

    python tests/golden/make_nee_paths_golden.py

tests/test_nee_paths_cpu.py regenerates the arrays and compares; tests/test_gpu_nee_paths.py renders the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def arrays(pkg, ob):
    import nee_paths_ref as npr
    out = {"scene": np.array(npr.frame(ob), dtype=pkg.SCENE_S), "max_path_bounces": np.array(npr.GOLDEN_BOUNCES, dtype=np.int32)}
    for name in sorted(npr.CASES):
        params, surf, guide = npr.CASES[name](pkg)
        c = npr.reference(pkg, ob, name, npr.GOLDEN_BOUNCES)
        out[name + "/params"] = np.array(params, dtype=pkg.PARAMS)
        out[name + "/surface"] = np.array(surf, dtype=pkg.SURFACE_S)
        out[name + "/guide"] = np.array(guide, dtype=np.uint8)
        out[name + "/image"] = np.array(c.image)
        out[name + "/seg_count"] = np.array(c.seg_count)
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import nee_paths_ref as npr
    np.savez_compressed(npr.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(npr.GOLDEN, os.path.getsize(npr.GOLDEN), "bytes")
