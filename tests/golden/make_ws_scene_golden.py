"""Records tests/golden/ws_scene_small.npz: inputs, image and hit counts of the CPU composite of the weight-space scene-S frame
(tests/ws_scene_ref.py) for the fixture configuration.  Needs a C compiler (the restatement is built on demand).

    python tests/golden/make_ws_scene_golden.py
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
import ws_scene_ref  # noqa: E402


def fixture_inputs(pkg):
    """Per-path realizations, context RENEWAL, N = 300, two gp ids: the 24 x 16 x 4 test frame."""
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", single=0, n_basis=300, mean_additional=True)
    return p, w, ws_scene_ref.small_scene(ob)


def main():
    pkg = _gpis_pkg.load_package()
    p, w, scene = fixture_inputs(pkg)
    c = ws_scene_ref.SceneRef(pkg, ob).compose(p, w, scene)
    assert c.n_miss and c.n_exit and c.n_visible and c.n_occluded and c.hit_gp_ids == {0, 1}
    out = os.path.join(HERE, "ws_scene_small.npz")
    np.savez_compressed(out, params=np.frombuffer(p.tobytes(), dtype=np.uint8), ws=np.frombuffer(w.tobytes(), dtype=np.uint8),
                        scene=np.frombuffer(np.array(scene, dtype=pkg.SCENE_S).tobytes(), dtype=np.uint8), image=c.image, hits=c.hits)
    print("%s: %d bytes, image sum %.6f, %d hits" % (out, os.path.getsize(out), float(c.image.sum()), int(c.hits.sum())))


if __name__ == "__main__":
    main()
