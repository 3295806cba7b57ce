"""Writes tests/golden/grid_mean_small.npz: the frame case of tests/test_gpu_grid_mean.py — the 24 x 20 x 3 frame of
tests/paths_rgb_ref.py on a single-realization medium whose mean is the 24^3 two-sphere grid of tests/grid_march_ref.py (a numpy
formula: the voxels are not stored), with a mean-colour ramp and a NON-ZERO emission field, 4 bounces — and the image and per-pixel
segment counts the CPU composite gives for it (tests/grid_march_ref.py: GridComposite standing in for the oracle in
PathsRgbRef.compose).  A tabulated primary mean emits 0 whatever the emission field says, so the composite is not emissive.

    python tests/golden/make_grid_mean_small_golden.py
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
import grid_march_ref as gmr          # noqa: E402

OUT = os.path.join(HERE, "grid_mean_small.npz")
MAX_BOUNCES = 4


def case(pkg):
    p = gmr.tabulated(pkg, pkg.params_for_config("C0"))
    c = p["mean_color"]
    c["enabled"], c["type"] = 1, 3                                  # the two-ramp product of paths_rgb_ref._ramp_case
    c["min"], c["max"], c["start"], c["end"] = 0.2, 0.9, -1.0, 1.0
    c["min2"], c["max2"], c["start2"], c["end2"] = 0.5, 1.5, -0.5, 0.5
    e = p["mean_emission"]
    e["enabled"], e["type"] = 1, 1                                  # left-right, at most 0.5: what would be emitted by another mean
    e["min"], e["max"], e["start"], e["end"] = 0.05, 0.5, -1.0, 1.0
    return p, gmr.grid(pkg, gmr.sphere_voxels(), gmr.sphere_world_to_index(), "linear")


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    params, g = case(pkg)
    comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=16)
    assert not prr.emissive(comp.params) and prr.emissive(params)
    scene = np.array(prr.frame(ob), dtype=pkg.SCENE_S).reshape(())
    c = prr.PathsRgbRef(pkg, ob).compose(comp, scene, MAX_BOUNCES, prr.ALBEDO)
    print("marched %s, hits %s, shadow %s" % (c.marched, c.hits, c.shadow))
    assert c.image.any() and c.hits[0] > 100 and c.hits[-1] > 0
    # with the same emission field an analytic mean does emit: the fixture's zero is the mean's doing, not the field's
    _, emi = comp.noise.mean_color_emission(np.random.default_rng(8).uniform(-1, 1, (64, 3)))
    assert emi.any()
    np.savez_compressed(OUT, medium=np.frombuffer(np.array(params, dtype=pkg.PARAMS).tobytes(), dtype=np.uint8),
                        scene=np.frombuffer(scene.tobytes(), dtype=np.uint8), max_bounces=np.int32(MAX_BOUNCES),
                        albedo=np.array(prr.ALBEDO, dtype=np.float32), image=c.image, seg_count=c.seg_count,
                        marched=np.array(c.marched), hits=np.array(c.hits), shadow=np.array(c.shadow))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
