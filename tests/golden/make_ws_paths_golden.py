"""Records tests/golden/ws_paths_small.npz: inputs, image and counts of the CPU composite of the weight-space path frame
(tests/ws_paths_ref.py) for the fixture configuration.  Needs a C compiler (the restatement is built on demand).

    python tests/golden/make_ws_paths_golden.py
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
import ws_oracle  # noqa: E402
import ws_paths_ref  # noqa: E402

MAX_BOUNCES, ALBEDO = 4, 0.8


def fixture_inputs(pkg):
    """Per-path realizations, context RENEWAL, N = 300, two gp ids, 4 bounces: the 24 x 16 x 4 test frame."""
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", single=0, n_basis=300, mean_additional=True)
    return p, w, ws_paths_ref.small_scene(ob)


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    p, w, scene = fixture_inputs(pkg)
    c = ws_paths_ref.PathsRef(pkg).compose(ws_paths_ref.WsMarch(p, w), scene, MAX_BOUNCES, ALBEDO)
    ws_paths_ref.check_non_vacuous(c)
    assert c.hit_gp_ids == {0, 1}
    out = os.path.join(HERE, "ws_paths_small.npz")
    np.savez_compressed(out, params=np.frombuffer(p.tobytes(), dtype=np.uint8), ws=np.frombuffer(w.tobytes(), dtype=np.uint8),
                        scene=np.frombuffer(np.array(scene, dtype=pkg.SCENE_S).tobytes(), dtype=np.uint8), image=c.image,
                        max_bounces=np.int32(MAX_BOUNCES), albedo=np.float32(ALBEDO), n_eval=np.uint64(c.n_eval), n_seg=np.uint64(c.n_seg))
    print("%s: %d bytes, image sum %.6f, %d segments, %d evaluations" % (out, os.path.getsize(out), float(c.image.sum()), c.n_seg, c.n_eval))


if __name__ == "__main__":
    main()
