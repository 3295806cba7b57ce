"""Writes tests/golden/sdf_mean_small.npz: the frame case of tests/test_gpu_sdf_mean.py — the 24 x 20 x 3 frame of
tests/paths_rgb_ref.py on a single-realization knob medium with a mean-colour ramp and a non-trivial "transform", 4 bounces — and
the image and per-pixel segment counts the CPU composite gives for it (tests/sdf_march_ref.py: SdfComposite standing in for the
oracle in PathsRgbRef.compose), so the GPU test needs neither.

    python tests/golden/make_sdf_mean_small_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, d)

import _gpis_pkg                      # noqa: E402
import oracle_bindings as ob          # noqa: E402
import paths_rgb_ref as prr           # noqa: E402
import sdf_march_ref as smr           # noqa: E402

OUT = os.path.join(HERE, "sdf_mean_small.npz")
MAX_BOUNCES = 4


def case(pkg):
    p = smr.procedural(pkg, pkg.params_for_config("C0"), "knob")
    c = p["mean_color"]
    c["enabled"], c["type"] = 1, 3                                  # the two-ramp product of paths_rgb_ref._ramp_case
    c["min"], c["max"], c["start"], c["end"] = 0.2, 0.9, -1.0, 1.0
    c["min2"], c["max2"], c["start2"], c["end2"] = 0.5, 1.5, -0.5, 0.5
    return p, smr.transform_demo()


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    params, T = case(pkg)
    comp = smr.SdfComposite(pkg, ob, params, transforms=(T, None), threads=16)
    scene = np.array(prr.frame(ob), dtype=pkg.SCENE_S).reshape(())
    c = prr.PathsRgbRef(pkg, ob).compose(comp, scene, MAX_BOUNCES, prr.ALBEDO)
    print("marched %s, hits %s, shadow %s" % (c.marched, c.hits, c.shadow))
    assert c.image.any() and c.hits[0] > 100 and c.hits[-1] > 0
    np.savez_compressed(OUT, params=np.frombuffer(np.array(params, dtype=pkg.PARAMS).tobytes(), dtype=np.uint8), transform=T,
                        scene=np.frombuffer(scene.tobytes(), dtype=np.uint8), max_bounces=np.int32(MAX_BOUNCES),
                        albedo=np.array(prr.ALBEDO, dtype=np.float32), image=c.image, seg_count=c.seg_count,
                        marched=np.array(c.marched), hits=np.array(c.hits), shadow=np.array(c.shadow))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
