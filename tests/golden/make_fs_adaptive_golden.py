"""Records tests/golden/fs_adaptive_small.npz: inputs and expected outputs of gpis_fs_render_scene_s_adaptive and
gpis_fs_render_scene_s_paths_adaptive on one case each (tests/fs_adaptive_ref.py: the Lambert frame on a Renewal medium, the path
driver on a Global one with a short last pass), produced by the CPU composite only: the schedule of tests/adaptive_ref.py over the per-sample values of
fs_scene_ref / fs_paths_ref.  Needs a C compiler (the restatements are built on demand).

    python tests/golden/make_fs_adaptive_golden.py
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
import fs_adaptive_ref  # noqa: E402


def main():
    pkg = _gpis_pkg.load_package()
    ob.build()
    out = fs_adaptive_ref.golden_arrays(pkg, ob)
    np.savez_compressed(fs_adaptive_ref.GOLDEN, **out)
    print("%s: %d bytes; samples %d (Lambert), %d (paths)" % (fs_adaptive_ref.GOLDEN, os.path.getsize(fs_adaptive_ref.GOLDEN),
                                                             int(out["lambert_info"]["samples"]), int(out["paths_info"]["samples"])))


if __name__ == "__main__":
    main()
