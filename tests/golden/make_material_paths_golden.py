"""Writes tests/golden/material_paths_small.npz: per case of tests/material_paths_ref.py the inputs (medium parameters, material
table, scene; the variance grid of the grid-flavoured case) and the CPU composite's image and per-pixel segment counts at
max_path_bounces = 4 on the 24 x 20 x 3 frame, and for the emissive case its first-hit frame (max_path_bounces = 1) too.

    python tests/golden/make_material_paths_golden.py

tests/test_material_paths_cpu.py regenerates the arrays and compares; tests/test_gpu_material_paths.py renders the recorded inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)


def _bytes(record):
    """the record's own memory: a copy made field by field (np.array(record)) leaves the alignment holes of the dtype unset"""
    return np.frombuffer(np.asarray(record).tobytes(), dtype=np.uint8)


def arrays(pkg, ob):
    import material_paths_ref as mp
    out = {"scene": _bytes(mp.frame(ob)), "max_path_bounces": np.array(mp.GOLDEN_BOUNCES, dtype=np.int32)}
    voxels, world_to_index, interpolate = mp.grid()
    assert interpolate == "linear"
    out["grid/voxels"] = np.array(voxels, dtype=np.float32)
    out["grid/world_to_index"] = np.array(world_to_index)
    for name in sorted(mp.CASES):
        params, mats, guide = mp.CASES[name](pkg)
        c = mp.reference(pkg, ob, name, mp.GOLDEN_BOUNCES)
        out[name + "/params"] = _bytes(params)
        out[name + "/materials"] = _bytes(mats)
        out[name + "/guide"] = np.array(1 if guide else 0, dtype=np.int32)
        out[name + "/image"] = np.array(c.image)
        out[name + "/seg_count"] = np.array(c.seg_count)
    first = mp.reference(pkg, ob, mp.EMISSIVE_CASE, 1)
    out["first_hit/image"] = np.array(first.image)
    out["first_hit/seg_count"] = np.array(first.seg_count)
    return out


if __name__ == "__main__":
    import _gpis_pkg
    import oracle_bindings as ob
    import material_paths_ref as mp
    ob.build()
    np.savez_compressed(mp.GOLDEN, **arrays(_gpis_pkg.load_package(), ob))
    print(mp.GOLDEN, os.path.getsize(mp.GOLDEN), "bytes")
