"""Writes tests/golden/paths_rgb_small.npz: per case of tests/paths_rgb_ref.py the inputs (medium parameters, albedo, guide flag;
the scene once) and the CPU composite's image and per-pixel segment counts at max_path_bounces = 4 on the 24 x 20 x 3 frame.

    python tests/golden/make_paths_rgb_golden.py

tests/test_paths_rgb_cpu.py regenerates the arrays and compares; tests/test_gpu_paths_rgb.py renders the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def arrays(pkg, ob):
    import paths_rgb_ref as prr
    out = {"scene": np.array(prr.frame(ob), dtype=pkg.SCENE_S), "max_path_bounces": np.array(prr.GOLDEN_BOUNCES, dtype=np.int32)}
    for name in sorted(prr.CASES):
        params, albedo, guide = prr.CASES[name](pkg)
        c = prr.reference(pkg, ob, name, prr.GOLDEN_BOUNCES)
        out[name + "/params"] = np.array(params, dtype=pkg.PARAMS)
        out[name + "/albedo"] = np.array(albedo, dtype=np.float32)
        out[name + "/guide"] = np.array(guide, dtype=np.uint8)
        out[name + "/image"] = np.array(c.image)
        out[name + "/seg_count"] = np.array(c.seg_count)
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import paths_rgb_ref as prr
    np.savez_compressed(prr.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(prr.GOLDEN, os.path.getsize(prr.GOLDEN), "bytes")
