"""Writes tests/golden/ws_small.npz: the weight-space medium's recorded answers (basis, field values, gradients, gp ids,
gpis_seg_out records, transmittance) for a few hundred inputs, computed by the C restatement tests/native/ws_oracle.c.
tests/test_gpu_ws.py::test_fixture compares the device with it, so the GPU test has a fixed answer even where no C compiler is.

    python tests/golden/make_ws_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _gpis_pkg  # noqa: E402
import ws_oracle  # noqa: E402

CASES = [  # (context, single realization, normal method, basis functions, CSG mean)
    ("renewal", 0, 0, 300, False),
    ("global", 1, 1, 301, True),
    ("renewal_plus", 0, 1, 65, True),
]


def main():
    pkg = _gpis_pkg.load_package()
    wso = ws_oracle.WsOracle()
    out = {"n_cases": np.int32(len(CASES))}
    for k, (ctx, single, normal, n_basis, extra) in enumerate(CASES):
        p, w = ws_oracle.ws_params(pkg, ctx=ctx, single=single, normal=normal, n_basis=n_basis, mean_additional=extra)
        rays = ws_oracle.make_rays(pkg, 64, seed=500 + k)
        rays["first_scatter"][::4] = 0
        seg, _ = wso.sample_distance(p, w, rays)
        vis, _ = wso.transmittance(p, w, rays)
        q = ws_oracle.make_queries(pkg, 48, seed=600 + k)
        v, g, i = wso.eval(p, w, q)
        pss = np.random.default_rng(700 + k).integers(0, 2 ** 32, (3, 4), dtype=np.uint64).astype(np.uint32)
        out.update({"params_%d" % k: np.array(p).reshape(1).view(np.uint8), "ws_%d" % k: np.array(w).reshape(1).view(np.uint8),
                    "rays_%d" % k: rays.view(np.uint8), "out_%d" % k: seg.view(np.uint8), "vis_%d" % k: vis,
                    "queries_%d" % k: q.view(np.uint8), "value_%d" % k: v, "grad_%d" % k: g, "id_%d" % k: i,
                    "pss_%d" % k: pss, "basis_%d" % k: wso.basis(p, w, pss)})
    path = os.path.join(HERE, "ws_small.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
