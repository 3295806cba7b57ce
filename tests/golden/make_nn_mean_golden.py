"""Writes the fixtures of the neural SDF mean (tests/test_nn_mean_cpu.py, tests/test_gpu_nn_mean.py):

  tests/golden/nn/net_{A,B,C,D,E,F,Z}.json + .bin   seeded numpy networks in the reference's descriptor format (no training)
  tests/golden/nn_mean_pins.npz                   Eigen's GEMV on the networks' layer shapes, from the REFERENCE's compiled Eigen
  tests/golden/nn_bake_small.npz                  the 24 x 20 x 3 four-bounce RGB frame of a medium baked from network A

The pins go through ref_fs_cond_forms of oracle/_ref/libgpis_ref.so with pinv = I, s12 = W^T, resid = x: `solved` is exactly W (a
dynamic column-major MatrixXd) and mean_out = mean + solved * resid.  Two records per shape:
  y0  with mean = 0: the product accumulated from zero — the temporary the network's `W * x + b` forms before it adds b;
  yb  with mean = b: `b + W * x`, which Eigen accumulates into a destination that already holds b.
For fewer than 128 columns the two orders give the same bits; from 128 columns on (16-column blocks) they do not, and the network
takes the first: the restatement is checked as gemv == y0 + b and gemv_acc(start = b) == yb.
PARITY UNPINNED: the clamp, the transform, the sine's use and offset / scale (restated from the source text alone).

The frame and the march condition (>= 20 % hits and >= 20 % misses in each march batch of tests/test_gpu_nn_mean.py) are asserted
here on the reference side: tests/grid_march_ref.py's GridComposite over the restatement's voxels.

    python tests/golden/make_nn_mean_golden.py [networks|pins|frame]
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, d)

import _gpis_pkg                      # noqa: E402
import nn_mean_ref as nmr             # noqa: E402

PIN_SHAPES = ((32, 3), (32, 32), (13, 13), (1, 32), (1, 13), (5, 127), (3, 128), (150, 150), (1, 150), (1, 1))       # rows x cols
MAX_BOUNCES = 4


def _blob(layers, mats):
    """the file's order: per layer out x in column-major, then out biases"""
    return np.concatenate([np.concatenate([np.asarray(W, dtype=np.float64).T.reshape(-1), np.asarray(b, dtype=np.float64)]) for W, b in mats])


def _random(rng, layers, wscale):
    return [(rng.standard_normal((o, i)) * wscale(i), rng.standard_normal(o) * 0.3) for i, o in layers]


def networks():
    out = {}
    # A, "blob": hidden units 0..2 are sin(2 p_a + pi/2) = cos(2 p_a); the output is 0.54 (2.362 - sum cos): a closed surface of
    # radius about 0.6 with a unit-size gradient there; small seeded weights everywhere else
    rng = np.random.default_rng(1601)
    layers = [(3, 32), (32, 32), (32, 1)]
    W0, b0 = rng.standard_normal((32, 3)) * 0.3, rng.standard_normal(32) * 0.3
    W0[:3], b0[:3] = 2.0 * np.eye(3), 0.0
    W1, b1 = rng.standard_normal((32, 32)) * 0.05, rng.standard_normal(32) * 0.3
    W1[:3] = 0.0
    W1[:3, :3], b1[:3] = np.eye(3), np.pi / 2
    W2, b2 = rng.standard_normal((1, 32)) * 0.004, np.array([0.54 * 2.362])
    W2[0, :3] = -0.54
    out["A"] = (layers, [(W0, b0), (W1, b1), (W2, b2)], 1.5)
    # B: the first layer scaled by 30, so the pre-activations spread over every branch of the sine below its limit; unit 0 of the
    # first hidden layer has zero weights and bias (the |x| < 2^-26 branch)
    rng = np.random.default_rng(1602)
    layers = [(3, 13)] + [(13, 13)] * 4 + [(13, 1)]
    mats = _random(rng, layers, lambda i: 1.0 / np.sqrt(i))
    mats[0] = (mats[0][0] * 30.0, mats[0][1] * 30.0)
    mats[1][0][0, :], mats[1][1][0] = 0.0, 0.0
    out["B"] = (layers, mats, 1.0)
    rng = np.random.default_rng(1603)
    layers = [(3, 150), (150, 150), (150, 1)]                       # 150 columns: the 16-column blocks with a tail of 6; 150 % 8 = 6 rows
    out["C"] = (layers, _random(rng, layers, lambda i: 1.0 / np.sqrt(i)), 1.0)
    rng = np.random.default_rng(1604)
    layers = [(3, 1), (1, 1), (1, 1), (1, 1)]                       # every layer a dot
    out["D"] = (layers, _random(rng, layers, lambda i: 1.0), 1.0)
    rng = np.random.default_rng(1605)
    layers = [(3, 5), (5, 1)]                                       # no hidden layer: no sine
    out["E"] = (layers, _random(rng, layers, lambda i: 1.0), 1.0)
    rng = np.random.default_rng(1606)
    layers = [(3, 44), (44, 44), (44, 1)]                           # between 33 and 64 wide: the 64-wide LDS form, 44 % 8 = 4 rows over
    out["F"] = (layers, _random(rng, layers, lambda i: 1.0 / np.sqrt(i)), 1.0)
    layers = [(3, 8), (8, 8), (8, 1)]
    mats = [(np.zeros((o, i)), np.zeros(o)) for i, o in layers]
    mats[-1][1][0] = nmr.Z_CONSTANT
    out["Z"] = (layers, mats, 1.0)
    return out


def write_networks():
    os.makedirs(nmr.NN_DIR, exist_ok=True)
    for name, (layers, mats, half) in networks().items():
        blob = _blob(layers, mats)
        blob.astype("<f8").tofile(os.path.join(nmr.NN_DIR, "net_%s.bin" % name))
        doc = {"bounds": {"min": [-half] * 3, "max": [half] * 3},
               "mean": {"file": "net_%s.bin" % name, "layers": [list(l) for l in layers]},
               "cov": {"file": "net_%s_cov.bin" % name, "layers": [[6, 4], [4, 1]]}}         # named, never written: the loader ignores it
        with open(nmr.network_path(name), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("net %s: %s, %d doubles" % (name, layers, blob.size))
    # the condition on the sine's branches, on the points the tests use
    pkg = _gpis_pkg.load_package()
    ref = nmr.NnMeanRef()
    for name, need in (("A", 3), ("B", 4)):
        net = pkg.load_network(nmr.network_path(name))
        br = np.unique(nmr.sin_branch(ref.preactivations(net, nmr.demo_points(net))))
        print("net %s: sine branches %s" % (name, br))
        assert br.max() <= 3 and len(br) >= need, (name, br)


def write_pins():
    import oracle_bindings as ob
    lib = ob.ref_lib()
    assert lib is not None, "oracle/_ref must be built (it needs the reference's sources)"
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.ref_fs_cond_forms.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp]
    P = lambda a: a.ctypes.data_as(vp)
    rng = np.random.default_rng(1600)
    out = {"shapes": np.array(PIN_SHAPES, dtype=np.int32)}
    for rows, cols in PIN_SHAPES:
        W, b, x = rng.standard_normal((rows, cols)), rng.standard_normal(rows), rng.standard_normal(cols)
        pinv, s12, s22 = np.asfortranarray(np.eye(cols)), np.asfortranarray(W.T), np.zeros((rows, rows), order="F")
        rec = {}
        for key, start in (("y0", np.zeros(rows)), ("yb", b)):
            y, cov = np.zeros(rows), np.zeros((rows, rows), order="F")
            lib.ref_fs_cond_forms(cols, rows, P(pinv), P(s12), P(s22), P(x), P(np.ascontiguousarray(start)), P(y), P(cov))
            rec[key] = y
        tag = "%dx%d" % (rows, cols)
        out.update({"W_" + tag: W, "b_" + tag: b, "x_" + tag: x, "y0_" + tag: rec["y0"], "yb_" + tag: rec["yb"]})
        print("pin %s: y0 + b == yb on %d of %d rows" % (tag, int(((rec["y0"] + b) == rec["yb"]).sum()), rows))
    np.savez_compressed(os.path.join(nmr.GOLD, "nn_mean_pins.npz"), **out)


def write_frame():
    import oracle_bindings as ob
    import grid_march_ref as gmr
    import paths_rgb_ref as prr
    import sdf_march_ref as smr
    import make_grid_mean_small_golden as small
    pkg = _gpis_pkg.load_package()
    ob.build()
    ref = nmr.NnMeanRef()
    vox = nmr.bake_case_voxels(pkg, ref)
    T = gmr.sphere_world_to_index()
    # the march condition of tests/test_gpu_nn_mean.py, on the reference side
    import test_gpu_grid_mean as tgg
    for ctx in ("none", "renewal", "renewal+"):
        params, _ = tgg.march_case(pkg, ctx)
        g = gmr.grid(pkg, vox, T, "linear")
        comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=16)
        rays = smr.camera_rays(pkg, tgg.N_RAYS, tgg.RAY_SEED)
        first = comp.sample_distance(rays)
        for k, w in enumerate((first, comp.sample_distance(tgg._continued(pkg, first, 6)))):
            hits = int((w["exited"] == 0).sum())
            print("march %s batch %d: %d hits of %d" % (ctx, k, hits, tgg.N_RAYS))
            assert 5 * hits >= tgg.N_RAYS and 5 * (tgg.N_RAYS - hits) >= tgg.N_RAYS, (ctx, k, hits)
    params, _ = small.case(pkg)
    g = gmr.grid(pkg, vox, T, "linear")
    comp = gmr.GridComposite(pkg, ob, params, grids=(g, None), threads=16)
    scene = np.array(prr.frame(ob), dtype=pkg.SCENE_S).reshape(())
    c = prr.PathsRgbRef(pkg, ob).compose(comp, scene, MAX_BOUNCES, prr.ALBEDO)
    print("marched %s, hits %s, shadow %s" % (c.marched, c.hits, c.shadow))
    assert c.image.any() and c.hits[0] > 100 and c.hits[-1] > 0
    np.savez_compressed(os.path.join(nmr.GOLD, "nn_bake_small.npz"),
                        medium=np.frombuffer(np.array(params, dtype=pkg.PARAMS).tobytes(), dtype=np.uint8),
                        scene=np.frombuffer(scene.tobytes(), dtype=np.uint8), max_bounces=np.int32(MAX_BOUNCES),
                        albedo=np.array(prr.ALBEDO, dtype=np.float32), image=c.image, seg_count=c.seg_count)


if __name__ == "__main__":
    what = sys.argv[1:] or ["networks", "pins", "frame"]
    if "networks" in what:
        write_networks()
    if "pins" in what:
        write_pins()
    if "frame" in what:
        write_frame()
