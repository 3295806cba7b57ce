"""TEST INFRASTRUCTURE: loads tests/native/nn_mean_ref.c, the plain-C restatement of the reference's NeuralMean over the mean network
of GPNeuralNetwork (the tests' reference for csrc/gpis_nn_mean.hpp; an independent second writing of it, with the host's sin).

Compiled on demand into build/nn_mean_ref/ (git-ignored) with the compiler and the flags of tests/sdf_mean_ref.py, plus OpenMP where
the compiler has it (the points are independent: threads change no bit).  The inverse of the transform comes from
tests/sdf_mean_ref.py's restatement of Mat4f::invert."""
import ctypes
import os
import subprocess

import numpy as np

import sdf_mean_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "nn_mean_ref.c")
OUT_DIR = os.path.join(ROOT, "build", "nn_mean_ref")
LIB = os.path.join(OUT_DIR, "libnn_mean_ref.so")
FLAGS = sdf_mean_ref.FLAGS + ["-Wno-unknown-pragmas"]
GOLD = os.path.join(ROOT, "tests", "golden")
NN_DIR = os.path.join(GOLD, "nn")
NAMES = ("A", "B", "C", "D", "E", "F", "Z")
Z_CONSTANT = 0.25

NET = np.dtype([
    ("n_layers", "<i4"), ("_pad", "<i4"), ("dims", "<i4", (16, 2)),
    ("bounds_min", "<f8", 3), ("bounds_max", "<f8", 3), ("offset", "<f4"), ("scale", "<f4"), ("inv_transform", "<f4", 16),
], align=True)


def available():
    return os.path.exists(LIB) or sdf_mean_ref._compiler() is not None


def build():
    if os.path.exists(LIB) and os.path.getmtime(SRC) <= os.path.getmtime(LIB):
        return LIB
    cc = sdf_mean_ref._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the neural mean restatement")
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    cmd = [cc] + FLAGS + ["-shared", "-o", tmp, SRC, "-lm"]
    if subprocess.call(cmd[:1] + ["-fopenmp"] + cmd[1:], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def network_path(name):
    return os.path.join(NN_DIR, "net_%s.json" % name)


class NnMeanRef:
    def __init__(self, threads=16):
        L = self.lib = ctypes.CDLL(build())
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.nn_ref_net_size.restype = sz
        L.nn_ref_gemv.argtypes = [i32, i32, vp, vp, vp, vp]
        L.nn_ref_gemv_acc.argtypes = [i32, i32, vp, vp, vp]
        L.nn_ref_mean.argtypes = [vp, vp, sz, vp, vp, vp]
        L.nn_ref_preactivations.argtypes = [vp, vp, sz, vp, vp]
        L.nn_ref_preactivations.restype = sz
        L.nn_ref_bake.argtypes = [vp, vp, vp, vp, vp, vp]
        assert L.nn_ref_net_size() == NET.itemsize
        os.environ.setdefault("OMP_NUM_THREADS", str(threads))
        self.inv = sdf_mean_ref.SdfMeanRef().invert

    def gemv(self, W, b, x):
        """W x + b in Eigen's order for a column-major MatrixXd W[rows, cols]"""
        W = np.asarray(W, dtype=np.float64)
        rows, cols = W.shape
        wc = np.ascontiguousarray(W.T).reshape(-1)                 # column-major
        b, x = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(rows, dtype=np.float64)
        self.lib.nn_ref_gemv(rows, cols, _p(wc), _p(b), _p(x), _p(y))
        return y

    def gemv_acc(self, W, x, start):
        """start + W x as Eigen's `dst += W * x` accumulates it into a destination that holds `start`"""
        W = np.asarray(W, dtype=np.float64)
        rows, cols = W.shape
        wc = np.ascontiguousarray(W.T).reshape(-1)
        x, y = np.ascontiguousarray(x, dtype=np.float64), np.array(start, dtype=np.float64).reshape(rows).copy()
        self.lib.nn_ref_gemv_acc(rows, cols, _p(wc), _p(x), _p(y))
        return y

    def net(self, net, offset=0.0, scale=1.0, transform=None):
        """the restatement's record of a bindings.Network (any object with layers, bounds_min, bounds_max, weights)"""
        d = np.zeros((), dtype=NET)
        d["n_layers"] = len(net.layers)
        for k, (i, o) in enumerate(net.layers):
            d["dims"][k] = (i, o)
        d["bounds_min"], d["bounds_max"] = net.bounds_min, net.bounds_max
        d["offset"], d["scale"] = offset, scale
        d["inv_transform"] = self.inv(np.eye(4, dtype=np.float32) if transform is None else transform).reshape(16)
        return d

    def mean(self, net, points, offset=0.0, scale=1.0, transform=None, want_grad=True):
        """(value, grad) of NeuralMean::mean / dmean_da at double-precision points (n, 3)"""
        d = self.net(net, offset, scale, transform)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        val = np.zeros(p.shape[0], dtype=np.float64)
        grad = np.zeros((p.shape[0], 3), dtype=np.float64) if want_grad else None
        self.lib.nn_ref_mean(_p(d), _p(net.weights), p.shape[0], _p(p), _p(val), _p(grad))
        return (val, grad) if want_grad else val

    def preactivations(self, net, points, transform=None):
        """every argument a sine receives while the network is evaluated at the points"""
        d = self.net(net, 0.0, 1.0, transform)
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        hidden = sum(o for _, o in net.layers[1:-1])
        out = np.zeros(p.shape[0] * hidden, dtype=np.float64)
        k = self.lib.nn_ref_preactivations(_p(d), _p(net.weights), p.shape[0], _p(p), _p(out))
        assert k == out.size
        return out

    def bake(self, net, dims, index_to_world, origin=(0, 0, 0), offset=0.0, scale=1.0, transform=None):
        """voxels[k, j, i] = float(mean(index_to_world . (origin + (i, j, k), 1))), index_to_world: 12 floats (rows 0..2)"""
        d = self.net(net, offset, scale, transform)
        dm, og = np.array(dims, dtype=np.int32), np.array(origin, dtype=np.int32)
        A = np.ascontiguousarray(index_to_world, dtype=np.float32).reshape(12)
        out = np.zeros((int(dm[2]), int(dm[1]), int(dm[0])), dtype=np.float32)
        self.lib.nn_ref_bake(_p(d), _p(net.weights), _p(dm), _p(og), _p(A), _p(out))
        return out


def sin_branch(x):
    """the branch of sin_glibc (csrc/gpis_libm.hpp) an argument takes: 0 |x| < 2^-26, 1 < 0.855469, 2 < 2.426265, 3 < 105414357.85,
    4 beyond (NaN in the restated sine)"""
    k = (np.abs(np.asarray(x, dtype=np.float64)).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return np.searchsorted(np.array([0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb], dtype=np.uint32), k, side="right")


# ---- the test points and transforms (numpy formulas) ---------------------------------------------------------------------------
N_POINTS = 2051


def demo_transform():
    """rotation x non-uniform scale x translation, row-major Mat4f"""
    c, s = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    tr = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2], [0, 0, 0, 1.0]])
    return (tr @ rot @ np.diag([1.1, 0.8, 1.3, 1.0])).astype(np.float32)


def demo_points(net, seed=21):
    """2 051 points (not a multiple of 64): uniform ones reaching past every face of the bounds, points on the faces, the eight
    corners, and points outside on one, two and three axes"""
    rng = np.random.default_rng(seed)
    lo, hi = net.bounds_min, net.bounds_max
    ext = hi - lo
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    faces = rng.uniform(lo, hi, (120, 3))
    for r in range(120):
        a = r % 3
        faces[r, a] = (lo, hi)[(r // 3) % 2][a]
    far = rng.uniform(lo - 2 * ext, hi + 2 * ext, (200, 3))
    uni = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (N_POINTS - 8 - 120 - 200, 3))
    return np.concatenate([corners, faces, far, uni])


def bake_case_voxels(pkg, ref, name="A"):
    """the march and frame case: network `name` on the 24^3 lattice of tests/grid_march_ref.py's two-sphere grid (voxel 0.125, not
    axis-aligned), as the restatement bakes it — voxels[k, j, i]"""
    import grid_march_ref as gmr
    T = gmr.sphere_world_to_index()
    return ref.bake(pkg.load_network(network_path(name)), (24, 24, 24), pkg.index_to_world(T))
