"""Writes tests/golden/paths_adaptive_small.npz and tests/golden/nee_paths_adaptive_small.npz: the inputs (medium parameters, scene,
adaptive settings, bounces, and the albedo or the surface) and the result of the restated adaptive frame (tests/paths_adaptive_ref.py)
on the 22 x 14 frame at 48 spp, with the per-sample values of the CPU oracle (oracle_render_scene_s_paths) and of the CPU composite
of gpis_render_scene_s_nee_paths (tests/nee_paths_ref.py): image, sample and segment counts, records, info and the per-pass sample
counts.  No GPU is involved.

    python tests/golden/make_paths_adaptive_golden.py

tests/test_paths_adaptive_cpu.py regenerates the arrays and compares; tests/test_gpu_paths_adaptive.py and
tests/test_gpu_nee_paths_adaptive.py render the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def lambert_arrays(pkg, ob):
    import adaptive_ref as ar
    import paths_adaptive_ref as par
    params, scene, adaptive, bounces, albedo = par.small_lambert_inputs(pkg, ob)
    out = {"params": np.array(params, dtype=pkg.PARAMS), "scene": np.array(scene, dtype=pkg.SCENE_S), "adaptive": np.array(adaptive, dtype=ar.ADAPTIVE_S),
           "albedo": np.float32(albedo), "max_bounces": np.int32(bounces)}
    ref = par.small_lambert_reference(pkg, ob)
    for k in par.LAMBERT_KEYS + ("counts",):
        out[k] = np.array(ref[k])
    return out


def nee_arrays(pkg, ob):
    import adaptive_ref as ar
    import paths_adaptive_ref as par
    params, surf, scene, adaptive, bounces = par.small_nee_inputs(pkg, ob)
    out = {"params": np.array(params, dtype=pkg.PARAMS), "surface": np.array(surf, dtype=pkg.SURFACE_S), "scene": np.array(scene, dtype=pkg.SCENE_S),
           "adaptive": np.array(adaptive, dtype=ar.ADAPTIVE_S), "max_bounces": np.int32(bounces)}
    ref = par.small_nee_reference(pkg, ob)
    for k in par.NEE_KEYS + ("counts",):
        out[k] = np.array(ref[k])
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import paths_adaptive_ref as par
    pkg = _gpis_pkg.load_package()
    for path, arrays in ((par.GOLDEN_LAMBERT, lambert_arrays), (par.GOLDEN_NEE, nee_arrays)):
        np.savez_compressed(path, **arrays(pkg, ob))
        print(path, os.path.getsize(path), "bytes")
