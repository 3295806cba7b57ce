"""The neural SDF mean without a GPU: the C restatement of the reference's NeuralMean (tests/native/nn_mean_ref.c, the reference of
tests/test_gpu_nn_mean.py) against the pins recorded from the reference's own compiled Eigen, bit for bit; the all-zero network;
the descriptor loader; the condition on the sine's branches.

PARITY UNPINNED: the clamp to the bounds, the transform, where the sine is applied and offset / scale are restated from the
reference's source text; only the summation order of a layer is pinned (tests/golden/make_nn_mean_golden.py says how)."""
import json
import os
import shutil

import numpy as np
import pytest

import nn_mean_ref as nmr

pytestmark = pytest.mark.skipif(not nmr.available(), reason="no C compiler for the restatement")


@pytest.fixture(scope="module")
def ref():
    return nmr.NnMeanRef()


@pytest.fixture(scope="module")
def pins():
    return dict(np.load(os.path.join(nmr.GOLD, "nn_mean_pins.npz")))


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_restatement_equals_the_pinned_eigen_gemv(ref, pins):
    """every layer shape of the test networks, the sizes around the 128-column threshold and the single-row dots: W x + b is the
    product accumulated from zero (y0) plus b; b + W x (yb) accumulates into b.  Both orders, bit for bit."""
    shapes = [tuple(int(v) for v in s) for s in pins["shapes"]]
    assert set(shapes) >= {(32, 3), (32, 32), (13, 13), (1, 32), (1, 13), (5, 127), (3, 128), (150, 150), (1, 150), (1, 1)}
    differ = 0
    for rows, cols in shapes:
        tag = "%dx%d" % (rows, cols)
        W, b, x, y0, yb = (pins["%s_%s" % (k, tag)] for k in ("W", "b", "x", "y0", "yb"))
        assert _same(ref.gemv(W, b, x), y0 + b), tag
        assert _same(ref.gemv_acc(W, x, np.zeros(rows)), y0), tag
        assert _same(ref.gemv_acc(W, x, b), yb), tag
        differ += int(not _same(y0 + b, yb))
        if cols < 128 or rows == 1:
            assert _same(y0 + b, yb), tag             # one block, or the dot: the order of the bias does not show
    assert differ >= 2                                # 3 x 128 and 150 x 150: the blocked order is told apart from the plain one


def test_blocked_order_is_not_the_sequential_sum(ref, pins):
    """at 128 columns and above the pinned result differs from the plain left-to-right sum on some row, and a single row never does"""
    for tag, blocked in (("3x128", True), ("150x150", True), ("5x127", False), ("1x150", False)):
        W, b, x, y0 = (pins["%s_%s" % (k, tag)] for k in ("W", "b", "x", "y0"))
        seq = np.zeros(W.shape[0])
        first = W[:, 0] * x[0]
        for j in range(W.shape[1]):
            seq = (first if (j == 0 and W.shape[0] == 1) else seq + W[:, j] * x[j])
        assert _same(seq, y0) != blocked, tag


@pytest.fixture(scope="module")
def nets(pkg):
    return {n: pkg.load_network(nmr.network_path(n)) for n in nmr.NAMES}


def test_zero_network_is_its_constant(ref, nets):
    pts = nmr.demo_points(nets["Z"])
    v, g = ref.mean(nets["Z"], pts, transform=nmr.demo_transform())
    assert np.array_equal(v, np.full(len(pts), nmr.Z_CONSTANT)) and not g.any()
    v, g = ref.mean(nets["Z"], pts, offset=0.5, scale=2.0)
    assert np.array_equal(v, np.full(len(pts), (nmr.Z_CONSTANT + 0.5) * 2.0)) and not g.any()


def test_mean_is_the_layers_in_numpy_order_of_operations(ref, nets):
    """network E (no sine, fewer than 128 columns): the value is two GEMVs the restatement performs one at a time, at a point inside
    the bounds with the identity transform; outside, the point is clamped first"""
    net = nets["E"]
    (W0, b0), (W1, b1) = net.layer(0), net.layer(1)
    for p, q in (((0.3, -0.2, 0.7), (0.3, -0.2, 0.7)), ((1.5, -0.2, -3.0), (1.0, -0.2, -1.0)), ((1.0, 1.0, -1.0), (1.0, 1.0, -1.0))):
        want = ref.gemv(W1, b1, ref.gemv(W0, b0, np.array(q)))[0]
        assert ref.mean(net, np.array([p]), want_grad=False)[0] == want
        assert ref.mean(net, np.array([p]), offset=0.25, scale=3.0, want_grad=False)[0] == (want + 0.25) * 3.0


def test_blob_is_a_closed_surface_of_radius_0_6(ref, nets):
    net = nets["A"]
    d = np.random.default_rng(3).standard_normal((500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    assert (ref.mean(net, 0.3 * d, want_grad=False) < 0).all() and (ref.mean(net, 1.0 * d, want_grad=False) > 0).all()
    v, g = ref.mean(net, 0.6 * np.eye(3))
    assert np.abs(v).max() < 0.05 and np.abs(np.linalg.norm(g, axis=1) - 1).max() < 0.1


def test_loader_round_trip_and_column_major_order(pkg, nets, tmp_path):
    a = nets["A"]
    assert a.layers == [(3, 32), (32, 32), (32, 1)] and a.weights.size == 32 * 4 + 32 * 33 + 33
    assert np.array_equal(a.bounds_min, [-1.5] * 3) and np.array_equal(a.bounds_max, [1.5] * 3)
    W0, b0 = a.layer(0)
    assert np.array_equal(W0[:3], 2.0 * np.eye(3)) and not b0[:3].any()            # the cos(2 p) units: rows of W, columns apart in the file
    assert a.weights[0] == 2.0 and a.weights[32 + 1] == 2.0 and a.weights[64 + 2] == 2.0
    W2, b2 = a.layer(2)
    assert W2.shape == (1, 32) and b2[0] == 0.54 * 2.362
    # a descriptor written from scratch reads back
    layers = [(3, 2), (2, 1)]
    w = np.arange(11, dtype=np.float64)
    w.astype("<f8").tofile(str(tmp_path / "w.bin"))
    doc = {"bounds": {"min": [-1, -2, -3], "max": [1, 2, 3]}, "mean": {"file": "w.bin", "layers": [list(l) for l in layers]}}
    (tmp_path / "n.json").write_text(json.dumps(doc))
    n = pkg.load_network(str(tmp_path / "n.json"))
    assert np.array_equal(n.weights, w) and np.array_equal(n.bounds_max, [1, 2, 3])
    W, b = n.layer(0)
    assert np.array_equal(W, [[0, 2, 4], [1, 3, 5]]) and np.array_equal(b, [6, 7])
    d = n.desc(offset=0.5, scale=2.0)
    assert int(d["n_layers"]) == 2 and d["dims"][:2].tolist() == [[3, 2], [2, 1]] and d["transform"].reshape(4, 4).tolist() == np.eye(4).tolist()


def test_loader_ignores_cov_and_raises_on_a_short_file(pkg, tmp_path):
    doc = json.load(open(nmr.network_path("E")))
    assert "cov" in doc and not os.path.exists(os.path.join(nmr.NN_DIR, doc["cov"]["file"]))       # named, absent, ignored
    shutil.copy(os.path.join(nmr.NN_DIR, "net_E.bin"), str(tmp_path / "net_E.bin"))
    del doc["cov"]
    (tmp_path / "e.json").write_text(json.dumps(doc))
    assert np.array_equal(pkg.load_network(str(tmp_path / "e.json")).weights, pkg.load_network(nmr.network_path("E")).weights)
    blob = open(str(tmp_path / "net_E.bin"), "rb").read()
    open(str(tmp_path / "net_E.bin"), "wb").write(blob[:-8])
    with pytest.raises(ValueError, match="need 26"):
        pkg.load_network(str(tmp_path / "e.json"))


def test_test_points_reach_the_branches_of_the_sine(ref, nets):
    """the condition the generator asserts when recording: A's pre-activations take at least three branches of sin_glibc, B's all
    four finite ones, and none passes the limit beyond which the restated sine gives NaN"""
    for name, need in (("A", 3), ("B", 4)):
        for T in (None, nmr.demo_transform()):
            br = np.unique(nmr.sin_branch(ref.preactivations(nets[name], nmr.demo_points(nets[name]), transform=T)))
            assert br.max() <= 3 and len(br) >= need, (name, br)
    assert np.array_equal(nmr.sin_branch([0.0, 1e-9, 0.5, 1.0, 3.0, 1e8, 2e8]), [0, 0, 1, 2, 3, 3, 4])


def test_points_cover_inside_faces_corners_and_outside(nets):
    for name in ("A", "B"):
        net = nets[name]
        p = nmr.demo_points(net)
        assert len(p) == nmr.N_POINTS == 2051 and len(p) % 64 != 0
        lo, hi = net.bounds_min, net.bounds_max
        out = (p < lo) | (p > hi)
        assert (~out.any(axis=1)).sum() > 300 and all((out.sum(axis=1) == k).sum() > 20 for k in (1, 2, 3))
        assert ((p == lo) | (p == hi)).all(axis=1).sum() == 8 and (((p == lo) | (p == hi)).any(axis=1) & ~out.any(axis=1)).sum() >= 100


def test_network_descriptor_size_matches_c(pkg):
    lib = pkg.load_library()
    got = dict(kv.split("=") for kv in lib.lib.gpis_abi_sizes().decode().split(","))
    assert int(got["gpis_mean_network"]) == pkg.MEAN_NETWORK.itemsize == 256
