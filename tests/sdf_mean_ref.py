"""TEST INFRASTRUCTURE: loads tests/native/sdf_mean_ref.c, the plain-C restatement of the reference's ProceduralMean over its SDF
shapes (the tests' reference for the mean; an independent second writing of csrc/gpis_sdf.hpp).

Compiled on demand into build/sdf_mean_ref/ (git-ignored) with `cc` (or ROCm's clang where `cc` is missing) and
-msse4.2 -mno-fma -ffp-contract=off, linked against the host libm."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sdf_mean_ref.c")
OUT_DIR = os.path.join(ROOT, "build", "sdf_mean_ref")
LIB = os.path.join(OUT_DIR, "libsdf_mean_ref.so")
FLAGS = ["-std=c11", "-O2", "-msse4.2", "-mno-fma", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra"]
FUNCS = ("knob", "knob_inner", "knob_outer", "two_spheres", "plane")       # SdfFunctions::Function order

SLOT = np.dtype([("type", "<i4"), ("func", "<i4"), ("radius", "<f4"), ("offset", "<f4"), ("scale", "<f4"), ("min", "<f4"),
                 ("center", "<f8", 3), ("dir", "<f8", 3), ("inv_transform", "<f4", 16)], align=True)

# outcome bits of sdf_ref_trace (tests/native/sdf_mean_ref.c: T_*): name -> (first bit, number of outcomes)
TRACE = {
    "opSmoothUnion clamp": (0, 3), "ssub(cutout, sphere) clamp": (3, 3), "ssub(sphere, base) clamp": (6, 3),
    "sdBase max(base, cylinder)": (9, 2), "sdBase max(-cylinder, base)": (11, 2), "sdBase max(-prism, base)": (13, 2),
    "knob eye min / max": (15, 2), "knob max(-etch, d)": (17, 2), "knob min(ssub(sphere, base), d)": (19, 2),
    "sdCappedCylinder min(., 0)": (21, 2), "sdCappedCylinder max(dx, dy)": (23, 2),
    "sdTriPrism outer max": (25, 2), "sdTriPrism inner max": (27, 2),
}


def _compiler():
    cc = shutil.which("cc")
    if cc:
        return cc
    clang = "/opt/rocm/llvm/bin/clang"
    return clang if os.path.exists(clang) else None


def available():
    return os.path.exists(LIB) or _compiler() is not None


def build():
    if os.path.exists(LIB) and os.path.getmtime(SRC) <= os.path.getmtime(LIB):
        return LIB
    cc = _compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the SDF mean restatement")
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + FLAGS + ["-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class SdfMeanRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(build())
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.sdf_ref_eval.argtypes = [i32, sz, vp, vp]
        L.sdf_ref_trace.argtypes = [i32, sz, vp]
        L.sdf_ref_trace.restype = ctypes.c_uint64
        L.sdf_ref_mat4_invert.argtypes = [vp, vp]
        L.sdf_ref_transform_point.argtypes = [vp, sz, vp, vp]
        L.sdf_ref_mean.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.sdf_ref_slot_size.restype = sz
        L.sdf_ref_rot_axis_x.argtypes = [ctypes.c_float, vp]
        assert L.sdf_ref_slot_size() == SLOT.itemsize

    def eval(self, func, points):
        """the SDF `func` (name or number) at float triples (n, 3) -> float32 (n,)"""
        f = FUNCS.index(func) if isinstance(func, str) else int(func)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(p.shape[0], dtype=np.float32)
        self.lib.sdf_ref_eval(f, p.shape[0], _p(p), _p(out))
        return out

    def trace(self, func, points):
        """the union of the min / max / clamp outcomes the points take: dict name -> tuple of booleans (TRACE)"""
        f = FUNCS.index(func) if isinstance(func, str) else int(func)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        bits = int(self.lib.sdf_ref_trace(f, p.shape[0], _p(p)))
        return {name: tuple(bool(bits >> (b + k) & 1) for k in range(n)) for name, (b, n) in TRACE.items()}

    def rot_axis_x(self, degrees):
        """Mat4f::rotAxis(Vec3f(1, 0, 0), degrees), upper-left 3x3"""
        out = np.zeros(9, dtype=np.float32)
        self.lib.sdf_ref_rot_axis_x(float(degrees), _p(out))
        return out.reshape(3, 3)

    def invert(self, m):
        a = np.ascontiguousarray(m, dtype=np.float32).reshape(16)
        out = np.zeros(16, dtype=np.float32)
        self.lib.sdf_ref_mat4_invert(_p(a), _p(out))
        return out.reshape(4, 4)

    def transform_point(self, m, points):
        a = np.ascontiguousarray(m, dtype=np.float32).reshape(16)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros_like(p)
        self.lib.sdf_ref_transform_point(_p(a), p.shape[0], _p(p), _p(out))
        return out

    def slot(self, mean, transform=None):
        """one mean slot from a gpis_mean record (a numpy record of bindings.MEAN) and, for a procedural mean, its "transform" """
        s = np.zeros((), dtype=SLOT)
        for k in ("type", "func", "radius", "offset", "scale", "min", "center"):
            s[k] = mean[k]
        d = np.array(mean["dir"], dtype=np.float64)
        l2 = 0.0
        for k in range(3):
            l2 += d[k] * d[k]
        ln = np.sqrt(l2)
        s["dir"] = d * (1.0 / ln if ln > 0 else 0.0)
        s["inv_transform"] = self.invert(np.eye(4, dtype=np.float32) if transform is None else transform).reshape(16)
        return s

    def mean(self, params, points, transforms=(None, None)):
        """(value, id, grad) of GaussianProcess::mean_weight_space for the means of a gpis_params record"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        s0 = self.slot(params["mean"], transforms[0])
        s1 = self.slot(params["mean_additional"], transforms[1]) if int(params["has_mean_additional"]) else None
        val = np.zeros(p.shape[0], dtype=np.float64)
        gid = np.zeros(p.shape[0], dtype=np.int32)
        grad = np.zeros((p.shape[0], 3), dtype=np.float64)
        self.lib.sdf_ref_mean(_p(s0), _p(s1) if s1 is not None else None, p.shape[0], _p(p), _p(val), _p(gid), _p(grad))
        return val, gid, grad
