"""Writes tests/golden/sdf_mean_pins.npz: values of the reference's own SdfFunctions::{knob, knob_inner, knob_outer, two_spheres}
and Mat4f::rotAxis, recorded through ctypes from oracle/_ref/libgpis_ref.so (the reference's SdfFunctions.cpp / Mat4f.cpp compiled in
place by oracle/Makefile), bit patterns as uint32.  `plane` is p.y and needs no pin.

The points (float triples): 2 048 uniform in [-1.2, 1.2]^3; 1 024 within 0.02 of a zero set, found by bisection of the reference
function along random rays (256 per function); 1 024 uniform in the box of the knob's base, where sdBase's choices are decided; the
axes, the origin, points with p.xz = 0, +-0 components, the cut-out centre, the base offset, points at |p| = 50.

A condition, asserted here when recording: over the pin set every min, max and clamp of sdKnob, sdKnobOuter and sdBase takes each
of its outcomes at least once (each clamp at both ends and in the interior), as the C restatement's trace reports it
(tests/sdf_mean_ref.py: SdfMeanRef.trace).

    python tests/golden/make_sdf_mean_golden.py        (needs oracle/_ref/libgpis_ref.so)
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libgpis_ref.so")
OUT = os.path.join(HERE, "sdf_mean_pins.npz")
SYMBOLS = {
    "knob": "_ZN8Tungsten12SdfFunctions4knobENS_3VecIfLj3EEERi",
    "knob_inner": "_ZN8Tungsten12SdfFunctions10knob_innerENS_3VecIfLj3EEERi",
    "knob_outer": "_ZN8Tungsten12SdfFunctions10knob_outerENS_3VecIfLj3EEERi",
    "two_spheres": "_ZN8Tungsten12SdfFunctions11two_spheresENS_3VecIfLj3EEERi",
}
ROT_AXIS = "_ZN8Tungsten5Mat4f7rotAxisERKNS_3VecIfLj3EEEf"
ROT_ANGLES = (-90.0, 90.0, -45.0)


class Vec3f(ctypes.Structure):
    _fields_ = [("v", ctypes.c_float * 3)]


class Mat4f(ctypes.Structure):
    _fields_ = [("a", ctypes.c_float * 16)]


class RefSdf:
    """the reference's exported functions; None from load() when oracle/_ref has not been built"""

    def __init__(self, lib):
        self.fn = {}
        for name, sym in SYMBOLS.items():
            f = getattr(lib, sym)
            f.argtypes = [Vec3f, ctypes.POINTER(ctypes.c_int)]
            f.restype = ctypes.c_float
            self.fn[name] = f
        self.rot = getattr(lib, ROT_AXIS)
        self.rot.argtypes = [ctypes.POINTER(Vec3f), ctypes.c_float]
        self.rot.restype = Mat4f

    @staticmethod
    def load():
        if not os.path.exists(REF_SO):
            return None
        return RefSdf(ctypes.CDLL(REF_SO))

    def eval(self, name, points):
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(p.shape[0], dtype=np.float32)
        mat = ctypes.c_int(0)
        f = self.fn[name]
        for i in range(p.shape[0]):
            out[i] = f(Vec3f((ctypes.c_float * 3)(*p[i])), ctypes.byref(mat))
        return out

    def rot_axis_x(self, degrees):
        axis = Vec3f((ctypes.c_float * 3)(1.0, 0.0, 0.0))
        return np.array(list(self.rot(ctypes.byref(axis), ctypes.c_float(degrees)).a), dtype=np.float32).reshape(4, 4)


def near_zero_set(ref, name, rng, count):
    """points within 0.02 of the zero set of `name`: bisection along random segments whose ends differ in sign"""
    lo, hi = (-1.2, 1.2)
    out = []
    while len(out) < count:
        a = rng.uniform(lo, hi, 3).astype(np.float32)
        b = rng.uniform(lo, hi, 3).astype(np.float32)
        fa, fb = ref.eval(name, a)[0], ref.eval(name, b)[0]
        if not (fa < 0) ^ (fb < 0):
            continue
        for _ in range(30):
            m = ((a.astype(np.float64) + b) * 0.5).astype(np.float32)
            fm = ref.eval(name, m)[0]
            if (fm < 0) == (fa < 0):
                a, fa = m, fm
            else:
                b, fb = m, fm
        d = (b.astype(np.float64) - a)
        d = rng.normal(size=3) if not d.any() else d
        d /= np.linalg.norm(d)
        out.append((a + d * rng.uniform(-0.02, 0.02)).astype(np.float32))
    return np.array(out, dtype=np.float32)


def special_points():
    s = np.float32(0.8)
    pts = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5),
           (0, 0.3, 0), (0, -0.3, 0), (0, 0.77, 0), (0, -0.62, 0), (0, -0.9, 0), (0, 1.2, 0),                 # p.xz = 0
           (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0), (0.0, 0.0, -0.0), (-0.0, -0.0, -0.0), (-0.0, 0.4, 0.3), (0.2, -0.0, 0.9),
           (0.0, 0.5 * s, 0.5 * s), (0.0, 0.2 * s, 0.2 * s),                                               # cut-out centre, etch centre
           (0.0, -0.775 * s, 0.0), (0.3, -0.775 * s, 0.0), (0.0, -0.775 * s, 0.8),                           # the base offset
           (50, 0, 0), (0, 50, 0), (0, 0, -50), (50 / np.sqrt(3), 50 / np.sqrt(3), 50 / np.sqrt(3)), (-30, 40, 0), (0, 10, 0), (0, -10, 0)]
    return np.array(pts, dtype=np.float32)


def pin_points(ref):
    rng = np.random.default_rng(20240614)
    parts = [rng.uniform(-1.2, 1.2, (2048, 3)).astype(np.float32)]
    for name in SYMBOLS:
        parts.append(near_zero_set(ref, name, rng, 256))
    box = rng.uniform((-0.95, -0.9, -0.95), (0.95, -0.35, 0.95), (1024, 3)).astype(np.float32)
    parts.append(box)
    parts.append(special_points())
    return np.concatenate(parts)


def assert_coverage(points):
    from sdf_mean_ref import SdfMeanRef
    r = SdfMeanRef()
    for func in ("knob", "knob_outer"):
        for name, hit in r.trace(func, points).items():
            assert all(hit), "pin points of %s miss an outcome of %s: %s" % (func, name, hit)


def main():
    ref = RefSdf.load()
    assert ref is not None, "oracle/_ref/libgpis_ref.so is not built"
    assert ref.eval("knob", [(0.9, 0.1, -0.2)]).view(np.uint32)[0] == 0x3E026B27
    assert ref.eval("knob", [(0, 0, 0)]).view(np.uint32)[0] == 0xBF19999A
    pts = pin_points(ref)
    assert_coverage(pts)
    out = {"points": pts, "rot_angles": np.array(ROT_ANGLES, dtype=np.float32),
           "rot_axis_x": np.stack([ref.rot_axis_x(a) for a in ROT_ANGLES]).view(np.uint32)}
    for name in SYMBOLS:
        out[name] = ref.eval(name, pts).view(np.uint32)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d points" % (OUT, pts.shape[0]))


if __name__ == "__main__":
    main()
