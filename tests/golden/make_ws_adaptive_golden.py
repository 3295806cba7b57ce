"""Records tests/golden/ws_adaptive_small.npz: inputs and expected outputs of gpis_ws_render_scene_s_adaptive and
gpis_ws_render_scene_s_paths_adaptive on one case each (tests/ws_adaptive_ref.py: the Lambert frame on a renewal medium, the path
driver on a global one), produced by the CPU composite only: the schedule of tests/adaptive_ref.py over the per-sample values of
ws_scene_ref / ws_paths_ref.  Needs a C compiler (the restatements are built on demand).

    python tests/golden/make_ws_adaptive_golden.py
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
import ws_adaptive_ref  # noqa: E402


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    out = ws_adaptive_ref.golden_arrays(pkg, ob)
    np.savez_compressed(ws_adaptive_ref.GOLDEN, **out)
    print("%s: %d bytes; samples %d (Lambert), %d (paths)" % (ws_adaptive_ref.GOLDEN, os.path.getsize(ws_adaptive_ref.GOLDEN),
                                                             int(out["lambert_info"]["samples"]), int(out["paths_info"]["samples"])))


if __name__ == "__main__":
    main()
