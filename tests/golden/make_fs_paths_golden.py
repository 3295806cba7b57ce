"""Records tests/golden/fs_paths_small.npz: inputs, image, per-pixel segment counts and class counts of the CPU composite of the
function-space path frame (tests/fs_paths_ref.py) for the fixture configuration.  Needs a C compiler (the shade step is built on
demand).

    python tests/golden/make_fs_paths_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _gpis_pkg  # noqa: E402
import oracle_bindings as ob  # noqa: E402
import fs_paths_ref  # noqa: E402
import fs_scene_ref  # noqa: E402
import ws_scene_ref  # noqa: E402

MAX_BOUNCES, ALBEDO = 4, 0.8


def fixture_inputs(pkg):
    """Context RENEWAL_PLUS, 20 sample points, step 0.03, 4 bounces: the 24 x 16 x 4 test frame."""
    return fs_scene_ref.fs_params(pkg, "RENEWAL_PLUS", 20, 0.03), ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0)


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    p, scene = fixture_inputs(pkg)
    c = fs_paths_ref.FsPathsRef(pkg, ob).compose(p, scene, MAX_BOUNCES, ALBEDO)
    fs_paths_ref.check_non_vacuous(c, fs_paths_ref.EXCLUDED_BY_THE_MEDIUM)
    assert c.n_three_hits > 0
    out = os.path.join(HERE, "fs_paths_small.npz")
    np.savez_compressed(out, params=np.frombuffer(p.tobytes(), dtype=np.uint8),
                        scene=np.frombuffer(np.array(scene, dtype=pkg.SCENE_S).tobytes(), dtype=np.uint8), image=c.image, segs=c.segs,
                        max_bounces=np.int32(MAX_BOUNCES), albedo=np.float32(ALBEDO), class_counts=c.class_counts())
    print("%s: %d bytes, image sum %.6f, %d segments, classes %s" % (out, os.path.getsize(out), float(c.image.sum()), c.n_seg, c.class_counts().tolist()))


if __name__ == "__main__":
    main()
