"""Writes tests/golden/adaptive_small.npz: the inputs (medium parameters, scene, adaptive settings) and the result of the restated
adaptive pass loop (tests/adaptive_ref.py over tests/native/adaptive_ref.c) on the 22 x 14 frame at 48 spp, with the sample values
of the CPU oracle's Lambert estimator: image, sample and hit counts, records, info and the per-pass sample counts.

    python tests/golden/make_adaptive_golden.py

tests/test_adaptive_cpu.py regenerates the arrays and compares; tests/test_gpu_adaptive.py renders the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def arrays(pkg, ob):
    import adaptive_ref as ar
    out = {"params": np.array(pkg.params_for_config("C0"), dtype=pkg.PARAMS), "scene": np.array(ar.small_scene(ob), dtype=pkg.SCENE_S),
           "adaptive": np.array(ar.default_adaptive(), dtype=ar.ADAPTIVE_S)}
    ref = ar.small_reference(pkg, ob)
    for k in ("radiance_sum", "sample_count", "hit_count", "records", "info", "counts"):
        out[k] = np.array(ref[k])
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import adaptive_ref as ar
    np.savez_compressed(ar.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(ar.GOLDEN, os.path.getsize(ar.GOLDEN), "bytes")
