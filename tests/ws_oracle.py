"""TEST INFRASTRUCTURE: loads tests/native/ws_oracle.c, the plain-C restatement of the reference's weight-space GP medium.

The library is compiled on demand into build/ws_oracle/ (git-ignored) with `cc` (or ROCm's clang where `cc` is missing) and the
restatement flags of oracle/Makefile's CFLAGS_ORACLE (SSE4.2, no FMA, no contraction), linked against the host libm."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ws_oracle.c")
OUT_DIR = os.path.join(ROOT, "build", "ws_oracle")
LIB = os.path.join(OUT_DIR, "libws_oracle.so")
THREADS = 16


def _compiler():
    cc = shutil.which("cc")
    if cc:
        return cc
    clang = "/opt/rocm/llvm/bin/clang"
    if os.path.exists(clang):
        return clang
    return None


def _flags():
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^CFLAGS_ORACLE\s*:?=\s*(.+)$", text, flags=re.M)
    return m.group(1).split()


def available():
    return os.path.exists(LIB) or _compiler() is not None


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = _compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the weight-space restatement")
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + _flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm", "-lpthread"])
    os.replace(tmp, LIB)
    return LIB


class WsOracle:
    def __init__(self):
        self.lib = ctypes.CDLL(build())
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L = self.lib
        L.ws_oracle_sample_distance.argtypes = [vp, vp, sz, vp, vp, i32, vp]
        L.ws_oracle_transmittance.argtypes = [vp, vp, sz, vp, vp, i32, vp]
        L.ws_oracle_eval.argtypes = [vp, vp, sz, vp, vp, vp, vp, i32]
        L.ws_oracle_basis.argtypes = [vp, vp, sz, vp, vp, i32]
        L.ws_oracle_sizes.argtypes = [i32]
        L.ws_oracle_sizes.restype = sz
        L.ws_xxhash32_4.argtypes = [vp]
        L.ws_xxhash32_4.restype = ctypes.c_uint32
        L.ws_pcg32_stream.argtypes = [sz, vp, ctypes.c_uint32, vp]
        L.ws_box_muller.argtypes = [ctypes.c_uint64, ctypes.c_uint32, vp]

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s: configuration outside the restatement (%d)" % (what, rc))

    def sample_distance(self, params, ws, rays, threads=THREADS):
        from _gpis_pkg import load_package
        pkg = load_package()
        rays = np.ascontiguousarray(rays, dtype=pkg.RAY_IN)
        out = np.zeros(len(rays), dtype=pkg.SEG_OUT)
        n_eval = ctypes.c_uint64()
        self._check(self.lib.ws_oracle_sample_distance(self._p(params), self._p(ws), len(rays), self._p(rays), self._p(out), threads,
                                                       ctypes.byref(n_eval)), "sample_distance")
        return out, n_eval.value

    def transmittance(self, params, ws, rays, threads=THREADS):
        from _gpis_pkg import load_package
        rays = np.ascontiguousarray(rays, dtype=load_package().RAY_IN)
        vis = np.zeros(len(rays), dtype=np.uint8)
        n_eval = ctypes.c_uint64()
        self._check(self.lib.ws_oracle_transmittance(self._p(params), self._p(ws), len(rays), self._p(rays), self._p(vis), threads,
                                                     ctypes.byref(n_eval)), "transmittance")
        return vis, n_eval.value

    def eval(self, params, ws, queries, threads=THREADS):
        n = len(queries)
        v, g, i = np.zeros(n), np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        self._check(self.lib.ws_oracle_eval(self._p(params), self._p(ws), n, self._p(np.ascontiguousarray(queries)), self._p(v), self._p(g),
                                            self._p(i), threads), "eval")
        return v, g, i

    def basis(self, params, ws, pss4, threads=THREADS):
        pss4 = np.ascontiguousarray(pss4, dtype=np.uint32).reshape(-1, 4)
        N = int(ws["basis_functions"])
        out = np.zeros((len(pss4), N, 6))
        self._check(self.lib.ws_oracle_basis(self._p(params), self._p(ws), len(pss4), self._p(pss4), self._p(out), threads), "basis")
        return out

    def xxhash32_4(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
        return np.array([self.lib.ws_xxhash32_4(self._p(np.ascontiguousarray(w))) for w in words], dtype=np.uint32)

    def pcg32_stream(self, states, count):
        states = np.ascontiguousarray(states, dtype=np.uint64)
        out = np.zeros((len(states), count), dtype=np.uint32)
        self.lib.ws_pcg32_stream(len(states), self._p(states), count, self._p(out))
        return out

    def box_muller(self, state, pairs):
        out = np.zeros(2 * pairs)
        self.lib.ws_box_muller(ctypes.c_uint64(int(state)), pairs, self._p(out))
        return out


# ---- the test medium and rays (shared by the tests, tests/golden/make_ws_golden.py and tools/ws_bench.py) ----------------------
CTX_NAMES = {"global": 0, "renewal_plus": 1, "renewal": 2, "none": 3}


def ws_params(pkg, ctx="renewal", single=0, normal=0, n_basis=300, mean_additional=False, sigma=0.1, length_scale=0.05,
              aniso=(1.0, 1.0, 1.0), seed=7, absorption_only=False):
    """A C0-like medium (spherical mean of radius 1 at the origin, squared exponential sigma 0.1, l 0.05) as a weight-space medium."""
    p = pkg.params_for_config("C0")
    p["correlation_context"] = CTX_NAMES[ctx] if isinstance(ctx, str) else ctx
    p["single_realization"] = single
    p["sigma"], p["length_scale"], p["aniso"], p["seed"] = sigma, length_scale, aniso, seed
    if mean_additional:           # CSG min with a second sphere (gp id 1)
        p["has_mean_additional"] = 1
        p["mean_additional"]["type"] = 1
        p["mean_additional"]["radius"] = 0.5
        p["mean_additional"]["center"] = (0.6, 0.3, 0.2)
    if absorption_only:
        p["sigma_a"], p["sigma_s"] = 1.0, 0.0
    w = pkg.default_ws_params(n_basis, normal)
    return p, w


def make_rays(pkg, n, seed=1, far=6.0, first_scatter=1, spread=0.35):
    """Camera-like rays from around (0, 0, 4) towards the unit sphere; near 0, finite far."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=pkg.RAY_IN)
    org = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.full(n, 4.0)], 1)
    tgt = np.stack([rng.uniform(-spread, spread, n) * 3, rng.uniform(-spread, spread, n) * 3, rng.uniform(-0.5, 0.5, n)], 1)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r["pos"] = org.astype(np.float32)
    r["dir"] = d.astype(np.float32)
    r["near_t"] = 0.0
    r["far_t"] = far
    r["pixel"][:, 0] = rng.integers(0, 1920, n)
    r["pixel"][:, 1] = rng.integers(0, 1080, n)
    r["spp"] = rng.integers(0, 64, n)
    r["segment"] = rng.integers(0, 4, n)
    r["scene_seed"] = 0xBA5EBA11
    r["u_jitter"] = rng.random(n, dtype=np.float32)
    r["first_scatter"] = first_scatter
    r["last_gp_id"] = 0
    r["last_aniso"] = (0.0, 0.0, 1.0)
    return r


def make_queries(pkg, n, seed=2, radius=1.3):
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=pkg.WS_QUERY)
    q["p"] = rng.uniform(-radius, radius, (n, 3))
    q["pixel"][:, 0] = rng.integers(0, 1920, n)
    q["pixel"][:, 1] = rng.integers(0, 1080, n)
    q["spp"] = rng.integers(0, 64, n)
    q["segment"] = rng.integers(0, 4, n)
    return q
