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


# ---- randomised media and rays (tests/test_ws_fuzz_cpu.py, tests/test_gpu_ws_fuzz.py, tests/test_gpu_ws_large.py) -----------------
# Argument range.  The device restates cos / sin for |x| < 105414350 only and refuses a call that leaves that range, so the
# generators keep every argument omega_i d_i.p + phi_i far inside it: a ray starts within 3.5 units of the origin and an
# "infinite" segment is clamped to near + 2000, so |p| < 2004; omega = |g sqrt(aniso) / l| with |g| < 9.8 (three Box-Muller
# normals of 23-bit uniforms are below 5.65 each), aniso <= 2 and l >= 0.04 is below 350; |phi| <= 2 pi.  The argument stays
# below 350 * 2004 + 7 < 10^6.
FUZZ_RNG_BASE = 7000                       # the fuzz case of seed s draws from default_rng(FUZZ_RNG_BASE + s)
FUZZ_DEFAULT_SEEDS = 24
FUZZ_N_BASIS = (0, 1, 8, 63, 64, 65, 128, 300, 301)
FUZZ_N_BASIS_P = (0.08, 0.08, 0.22, 0.14, 0.14, 0.14, 0.10, 0.05, 0.05)      # most cases <= 128 (cost)
f32 = np.float32


def random_ws_params(pkg, rng):
    """A seeded random (gpis_params, gpis_ws_params) pair drawn only from what gpis_ws_create accepts."""
    p = pkg.params_for_config("C0")
    p["correlation_context"] = int(rng.integers(0, 4))
    p["single_realization"] = int(rng.integers(0, 2))
    normal = int(rng.integers(0, 2))                     # conditioned Gaussian / finite differences
    n_basis = int(rng.choice(FUZZ_N_BASIS, p=FUZZ_N_BASIS_P))
    p["seed"] = int(rng.integers(0, 2 ** 31))
    p["sigma"] = float(rng.uniform(0.05, 0.3))
    p["length_scale"] = float(rng.uniform(0.04, 0.12))
    p["aniso"] = rng.uniform(0.5, 2.0, 3).astype(f32) if rng.random() < 0.5 else (1.0, 1.0, 1.0)
    p["step_size"] = float(rng.choice([0.005, 0.01, 0.02]))
    p["min_step"] = int(rng.choice([0, 4, 16]))
    p["max_bounces"] = int(rng.choice([2, 1024]))
    kind = rng.integers(0, 4)
    if kind == 1:
        p["mean"]["type"] = pkg.MEAN_TYPE.LINEAR
        p["mean"]["center"] = rng.uniform(-0.3, 0.3, 3)
        p["mean"]["dir"] = rng.standard_normal(3)
        p["mean"]["scale"] = float(rng.uniform(0.5, 2.0))
        p["mean"]["min"] = float(rng.choice([-3.4e38, -0.2]))
    elif kind == 2:
        p["mean"]["type"] = pkg.MEAN_TYPE.HOMOGENEOUS
        p["mean"]["offset"] = float(rng.uniform(-0.05, 0.1))
    else:
        p["mean"]["center"] = rng.uniform(-0.2, 0.2, 3)
        p["mean"]["radius"] = float(rng.uniform(0.6, 1.1))
    if rng.random() < 0.35:
        p["has_mean_additional"] = 1
        p["mean_additional"]["type"] = pkg.MEAN_TYPE.SPHERICAL
        p["mean_additional"]["center"] = rng.uniform(-0.8, 0.8, 3)
        p["mean_additional"]["radius"] = float(rng.uniform(0.3, 0.7))
    p["density"] = float(rng.choice([0.5, 1.0, 2.0]))
    p["sigma_a"] = rng.choice([0.0, 0.25, 1.0], 3).astype(f32)
    p["sigma_s"] = (np.zeros(3) if rng.random() < 0.2 else rng.choice([0.5, 1.0, 3.0], 3)).astype(f32)     # zeros: absorption only
    if rng.random() < 0.3:
        c = p["mean_color"]
        c["enabled"], c["type"] = 1, int(rng.integers(0, 4))
        c["min"], c["max"], c["start"], c["end"] = rng.uniform(0.1, 0.3), rng.uniform(0.6, 0.95), -1.0, 1.0
        c["min2"], c["max2"], c["start2"], c["end2"] = rng.uniform(0.05, 0.2), rng.uniform(0.5, 0.8), -0.8, 0.5
    return p, pkg.default_ws_params(n_basis, normal)


def random_rays(pkg, rng, n):
    """Segments of every kind (test_gpu_fuzz.py's _random_rays): 40 % start inside the surface as continued paths (first_scatter 0,
    bounce >= 1, random last_aniso / last_gp_id / last_val), the rest outside with near_t > 0; the first three are the early-out
    (far_t 0), the "infinite segment" and the empty segment (far_t == near_t)."""
    r = np.zeros(n, dtype=pkg.RAY_IN)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = rng.random(n) < 0.4
    o = np.where(inside[:, None], rng.uniform(-0.9, 0.9, (n, 3)), -2.5 * d + rng.uniform(-0.7, 0.7, (n, 3)))
    r["pos"], r["dir"] = o.astype(f32), d.astype(f32)
    r["near_t"] = np.where(inside, 0.0, rng.uniform(0.8, 1.4, n)).astype(f32)
    r["far_t"] = r["near_t"] + rng.uniform(0.3, 2.2, n).astype(f32)
    r["far_t"][:3] = (0.0, np.inf, r["near_t"][2])
    # far_t < near_t with min_step 0 is outside the medium's domain: the reference's step (far - near) / 0.0f is -inf and its march
    # loop `while (t < farT)` never ends (transmittance has no early-out for far_t == 0), so the far_t = 0 ray starts at 0
    r["near_t"][0] = 0.0
    r["pixel"] = rng.integers(0, 2000, (n, 2))
    r["spp"] = rng.integers(0, 64, n)
    r["segment"] = rng.integers(0, 4, n)
    r["scene_seed"] = 0xBA5EBA11
    r["info_t"] = rng.uniform(0, 3, n).astype(f32)
    r["u_jitter"] = rng.random(n).astype(f32)
    r["first_scatter"] = (~inside).astype(np.uint32)
    r["bounce"] = np.where(inside, rng.integers(1, 3, n), 0)
    r["last_gp_id"] = np.where(inside, rng.integers(0, 2, n), 0)
    r["last_val"] = np.where(inside, rng.uniform(-0.02, 0.02, n), 0).astype(f32)
    r["last_aniso"] = np.where(inside[:, None], rng.standard_normal((n, 3)) * 4.0, 0.0)
    return r


def random_queries(pkg, rng, n, radius=1.3):
    q = np.zeros(n, dtype=pkg.WS_QUERY)
    q["p"] = rng.uniform(-radius, radius, (n, 3))
    q["pixel"] = rng.integers(0, 1920, (n, 2))
    q["spp"] = rng.integers(0, 64, n)
    q["segment"] = rng.integers(0, 4, n)
    return q


def fuzz_case(pkg, seed):
    """The inputs of fuzz case `seed`: params, ws params, 8 pss words, 256 queries, 448 rays."""
    rng = np.random.default_rng(FUZZ_RNG_BASE + seed)
    p, w = random_ws_params(pkg, rng)
    pss = rng.integers(0, 2 ** 32, (8, 4), dtype=np.uint64).astype(np.uint32)
    return p, w, pss, random_queries(pkg, rng, 256), random_rays(pkg, rng, 448)


def absorption_only(p):
    return not np.asarray(p["sigma_s"]).any()


def fuzz_classes(pkg, p, w):
    """The configuration classes a fuzz case belongs to (test_ws_fuzz_cpu.py asserts that the seed list covers every one)."""
    n = int(w["basis_functions"])
    out = {"ctx%d" % int(p["correlation_context"]), "normal%d" % int(w["normal_method"]),
           "single" if int(p["single_realization"]) else "per_path", "mean%d" % int(p["mean"]["type"]),
           "n0" if n == 0 else ("n<=63" if n <= 63 else ("n64" if n == 64 else "n>=65"))}
    if int(p["has_mean_additional"]):
        out.add("csg")
    if not np.all(np.asarray(p["aniso"]) == 1.0):
        out.add("aniso")
    if absorption_only(p):
        out.add("absorption_only")
    return out


FUZZ_CLASSES = ({"ctx%d" % c for c in range(4)} | {"normal0", "normal1", "single", "per_path", "mean0", "mean1", "mean2", "csg", "aniso",
                                                   "absorption_only", "n0", "n<=63", "n64", "n>=65"})


def describe(p, w):
    return ("ctx %d single %d normal %d N %d sigma %.3f l %.3f aniso %s step %g min_step %d max_bounces %d mean %d csg %d abs_only %d colour %d"
            % (int(p["correlation_context"]), int(p["single_realization"]), int(w["normal_method"]), int(w["basis_functions"]),
               float(p["sigma"]), float(p["length_scale"]), np.asarray(p["aniso"]).round(2).tolist(), float(p["step_size"]), int(p["min_step"]),
               int(p["max_bounces"]), int(p["mean"]["type"]), int(p["has_mean_additional"]), int(absorption_only(p)),
               int(p["mean_color"]["enabled"]) * (1 + int(p["mean_color"]["type"]))))


def mixed_rays(pkg, rng, n):
    """Rays for batches of more segments than resident waves: the kind of each ray is drawn independently, so whatever stride a
    wave walks the batch with, its consecutive segments differ in kind and cost.  Kinds: 0 a miss of the unit sphere (marches the
    whole segment), 1 an early hit (starts just outside the surface), 2 a far hit (camera-like, from z = 4), 3 a start inside the
    surface as a continued path, 4 far_t = 0 (the early-out)."""
    r = make_rays(pkg, n, seed=int(rng.integers(0, 2 ** 31)), far=6.0)
    kind = rng.integers(0, 5, n)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos, dr = r["pos"].astype(np.float64), r["dir"].astype(np.float64)
    k = kind == 0                                            # passes the sphere at distance 1.6 from the origin
    side = np.cross(d, rng.standard_normal((n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    pos[k], dr[k] = (1.6 * side - 2.0 * d)[k], d[k]
    r["far_t"][k] = 4.0
    k = kind == 1
    pos[k], dr[k] = (-1.15 * d)[k], d[k]
    r["far_t"][k] = 2.0
    k = kind == 3
    pos[k], dr[k] = rng.uniform(-0.5, 0.5, (n, 3))[k], d[k]
    r["far_t"][k] = 2.5
    r["first_scatter"][k] = 0
    r["bounce"][k] = 1
    r["last_gp_id"][k] = rng.integers(0, 2, n)[k]
    r["last_val"][k] = rng.uniform(-0.02, 0.02, n).astype(f32)[k]
    r["last_aniso"][k] = (rng.standard_normal((n, 3)) * 4.0)[k]
    r["far_t"][kind == 4] = 0.0
    r["pos"], r["dir"] = pos.astype(f32), dr.astype(f32)
    return r, kind


# ---- the field's formula in high precision, independent of the restatement --------------------------------------------------------
# f(p) = sqrt(sigma^2) sqrt(2 / N) sum_i w_i cos(omega_i d_i.p + phi_i) + mean(p), from an exported basis (d, omega, phi, w as
# IEEE doubles, taken as exact inputs), with mpmath at 60 digits (numpy's long double where mpmath is missing).
U = 2.0 ** -53
FD_EPS = float(f32(0.0001))                  # sampleGradient's `float eps = 0.0001f`, widened


def _mp():
    try:
        import mpmath
        mpmath.mp.dps = 60
        return mpmath
    except ImportError:
        return None


class ExactField:
    """f, its analytic gradient and the bound of a double evaluation's rounding error, for the realization `basis` ((N, 6):
    d.x, d.y, d.z, omega, phi, w) of the medium `p`.  sigma^2 is the float product the reference's covariance stores."""

    def __init__(self, pkg, p, basis):
        self.mp = _mp()
        self.pkg, self.p = pkg, p
        self.n = len(basis)
        self.basis = np.asarray(basis, dtype=np.float64).reshape(self.n, 6)
        self.s2 = float(f32(p["sigma"]) * f32(p["sigma"]))
        R = self.R
        self.amp = self._sqrt(R(self.s2)) * self._sqrt(R(2) / R(self.n)) if self.n else R(0)
        self.amp_f = float(self.amp)
        self.means = [p["mean"]] + ([p["mean_additional"]] if int(p["has_mean_additional"]) else [])

    def R(self, x):
        return self.mp.mpf(float(x)) if self.mp else np.longdouble(x)

    def _sqrt(self, x):
        return self.mp.sqrt(x) if self.mp else np.sqrt(x)

    def _cos(self, x):
        return self.mp.cos(x) if self.mp else np.cos(x)

    def _sin(self, x):
        return self.mp.sin(x) if self.mp else np.sin(x)

    def _mean_one(self, mu, P):
        """(value, gradient) of one mean function at P (a list of three reals)"""
        R, T = self.R, self.pkg.MEAN_TYPE
        zero = [R(0)] * 3
        if int(mu["type"]) == T.HOMOGENEOUS:
            return R(mu["offset"]), zero
        d = [P[c] - R(mu["center"][c]) for c in range(3)]
        if int(mu["type"]) == T.SPHERICAL:
            ln = self._sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            return ln - R(mu["radius"]), [x / ln for x in d]
        dr = [R(mu["dir"][c]) for c in range(3)]
        ln = self._sqrt(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2])
        dr = [x / ln for x in dr]
        v = (d[0] * dr[0] + d[1] * dr[1] + d[2] * dr[2]) * R(mu["scale"])
        if v > R(mu["min"]):
            return v, [x * R(mu["scale"]) for x in dr]
        return R(mu["min"]), zero

    def mean(self, P):
        """(value, gradient, gp id): the minimum of the mean and the additional mean (the CSG union)"""
        best = None
        for k, mu in enumerate(self.means):
            v, g = self._mean_one(mu, P)
            if best is None or v < best[0]:
                best = (v, g, k)
        return best

    def value(self, p):
        """f(p) at the double point p: (f, gp id)"""
        P = [self.R(x) for x in p]
        acc = self.R(0)
        for d0, d1, d2, om, ph, w in self.basis:
            acc += self.R(w) * self._cos(self.R(om) * (self.R(d0) * P[0] + self.R(d1) * P[1] + self.R(d2) * P[2]) + self.R(ph))
        m, _, gid = self.mean(P)
        return self.amp * acc + m, gid

    def gradient(self, p):
        """the analytic gradient of f at p"""
        P = [self.R(x) for x in p]
        g = [self.R(0)] * 3
        for d0, d1, d2, om, ph, w in self.basis:
            s = -self._sin(self.R(om) * (self.R(d0) * P[0] + self.R(d1) * P[1] + self.R(d2) * P[2]) + self.R(ph)) * self.R(w) * self.R(om)
            g = [g[0] + s * self.R(d0), g[1] + s * self.R(d1), g[2] + s * self.R(d2)]
        _, mg, _ = self.mean(P)
        return [self.amp * g[c] for c in range(3)], mg

    def bound(self, p, grad=False):
        """The rounding-error bound of a double evaluation of f (or, with grad, of a component of its gradient) at p:
            amp sum_i |c_i| ((N + 4) u + 4 u (|omega_i| |d_i| |p| + |phi_i|)) + 4 u |mean(p)|,   c_i = w_i (or w_i omega_i),
        with amp = sqrt(sigma^2) sqrt(2 / N) and u = 2^-53.  The term (N + 4) u covers the N - 1 additions of the sum in any order,
        the product with w_i, the cos / sin (below one ulp) and the two final products; 4 u (|omega| |d| |p| + |phi|) is the
        perturbation of the argument (three products, two sums, the product with omega, the sum with phi) through |cos'| <= 1;
        4 u |mean| stands for the mean's own few operations."""
        b = self.basis
        pn = float(np.linalg.norm(np.asarray(p, dtype=np.float64)))
        c = np.abs(b[:, 5] * (b[:, 3] if grad else 1.0))
        dn = np.linalg.norm(b[:, :3], axis=1)
        basis = self.amp_f * float(np.sum(c * ((self.n + 4) * U + 4 * U * (np.abs(b[:, 3]) * dn * pn + np.abs(b[:, 4]))))) if self.n else 0.0
        return basis + 4 * U * abs(float(self.mean([self.R(x) for x in p])[0]))

    def check(self, p, value, grad, normal_method):
        """Compares a double evaluation (value, grad[3]) of the medium at p with the exact formula and asserts |error| <= bound.
        Returns the figures (value error, value bound, largest gradient error / bound ratio).

        Conditioned-Gaussian normals: the reference pushes the analytic gradient of the basis sum through the Jacobian of its
        shell embedding, J = diag(((p_c + eps) - p_c) / eps) with eps = 1e-4 in doubles.  In exact arithmetic J is the identity; in
        doubles p_c + eps is rounded, so J_cc differs from 1 by up to ulp(p_c) / (2 eps), about 1e-12: a property of the formula the
        medium defines, not of how it is evaluated.  The exact gradient is therefore g_c / J_cc + dmean / dp_c with J_cc taken from
        the IEEE sum p_c + eps and everything else exact.
        Finite differences: the six points p +- eps e_c (eps = 0.0001f) are the IEEE sums; the exact central difference is taken at
        those very points, so no truncation term is needed, and its bound is the gradient's bound plus
        (bound_f(p + e) + bound_f(p - e)) / (2 eps)."""
        R = self.R
        p = np.asarray(p, dtype=np.float64)
        fv, _ = self.value(p)
        bv = self.bound(p)
        ev = abs(float(R(value) - fv))
        assert ev <= bv, ("value", p.tolist(), value, float(fv), ev, bv)
        assert bv <= 1e-9 * max(1.0, abs(float(fv))), ("value bound", bv, float(fv))
        bg = self.bound(p, grad=True)
        worst = 0.0
        if normal_method == self.pkg.NORMAL.FINITE_DIFFERENCES:
            for c in range(3):
                e = np.zeros(3)
                e[c] = FD_EPS
                hi, lo = p + e, p - e
                cd = (self.value(hi)[0] - self.value(lo)[0]) / (R(2) * R(FD_EPS))
                b_cd = bg + (self.bound(hi) + self.bound(lo)) / (2 * FD_EPS)
                err = abs(float(R(grad[c]) - cd))
                assert err <= b_cd, ("central difference", c, p.tolist(), grad[c], float(cd), err, b_cd)
                worst = max(worst, err / b_cd)
        else:
            g, mg = self.gradient(p)
            for c in range(3):
                j = (R(float(p[c] + 1e-4)) - R(p[c])) / R(1e-4)
                want = g[c] / j + mg[c]
                err = abs(float(R(grad[c]) - want))
                assert err <= bg, ("gradient", c, p.tolist(), grad[c], float(want), err, bg, "without J", float(g[c] + mg[c]))
                worst = max(worst, err / bg)
        return ev, bv, worst


# The configuration classes of the high-precision check: normal method x mean type, with anisotropy, a CSG pair, a single
# realization.  N >= 64: the bound's mean term 4 u |mean(p)| vanishes on the surface, where the subtraction |p - c| - r still
# leaves an error of about u |p - c|; from N = 64 on the sum's own (N + 4) u term is an order of magnitude above that.
EXACT_CASES = {
    "cg-spherical-n65": dict(ctx="renewal", normal=0, n_basis=65, aniso=(1.0, 0.5, 2.0), sigma=0.1, length_scale=0.05, seed=11),
    "cg-linear-csg-n300": dict(ctx="global", normal=0, n_basis=300, mean_additional=True, sigma=0.2, length_scale=0.08, seed=12),
    "cg-homogeneous-single-n64": dict(ctx="none", single=1, normal=0, n_basis=64, aniso=(2.0, 1.5, 0.5), sigma=0.3, length_scale=0.04, seed=13),
    "fd-spherical-csg-n64": dict(ctx="renewal_plus", normal=1, n_basis=64, mean_additional=True, sigma=0.1, length_scale=0.05, seed=14),
    "fd-linear-n65": dict(ctx="renewal", normal=1, n_basis=65, aniso=(0.5, 2.0, 1.0), sigma=0.25, length_scale=0.12, seed=15),
    "fd-homogeneous-n300": dict(ctx="none", single=1, normal=1, n_basis=300, sigma=0.05, length_scale=0.06, seed=16),
}


def exact_case(pkg, name, n_queries=16):
    p, w = ws_params(pkg, **EXACT_CASES[name])
    if "linear" in name:
        p["mean"]["type"] = pkg.MEAN_TYPE.LINEAR
        p["mean"]["center"] = (0.1, -0.2, 0.05)
        p["mean"]["dir"] = (0.3, -1.0, 0.6)
        p["mean"]["scale"] = 1.5
        p["mean"]["min"] = -0.2                  # the clamp is active on about half of the cube
    elif "homogeneous" in name:
        p["mean"]["type"] = pkg.MEAN_TYPE.HOMOGENEOUS
        p["mean"]["offset"] = 0.03
    return p, w, random_queries(pkg, np.random.default_rng(int(p["seed"])), n_queries)
