"""TEST INFRASTRUCTURE: loads tests/native/grid_mean_ref.c, the plain-C restatement of the reference's TabulatedMean over a dense
voxel array (the tests' reference for that mean; an independent second writing of csrc/gpis_grid_mean.hpp).

Compiled on demand into build/grid_mean_ref/ (git-ignored) with the compiler and the flags of tests/sdf_mean_ref.py."""
import ctypes
import os
import subprocess

import numpy as np

import sdf_mean_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "grid_mean_ref.c")
OUT_DIR = os.path.join(ROOT, "build", "grid_mean_ref")
LIB = os.path.join(OUT_DIR, "libgrid_mean_ref.so")
FLAGS = sdf_mean_ref.FLAGS

DESC = np.dtype([
    ("dims", "<i4", 3), ("interpolate", "<i4"), ("origin", "<i4", 3), ("_pad", "<i4"),
    ("bounds_min", "<f4", 3), ("bounds_max", "<f4", 3), ("inv_natural_transform", "<f4", 16),
], align=True)


class _Slot(ctypes.Structure):
    _fields_ = [("desc", ctypes.c_void_p), ("voxels", ctypes.c_void_p), ("offset", ctypes.c_float), ("scale", ctypes.c_float),
                ("volume", ctypes.c_int32)]


def available():
    return os.path.exists(LIB) or sdf_mean_ref._compiler() is not None


def build():
    if os.path.exists(LIB) and os.path.getmtime(SRC) <= os.path.getmtime(LIB):
        return LIB
    cc = sdf_mean_ref._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the tabulated mean restatement")
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + FLAGS + ["-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Grid:
    """a voxel grid as gpis_set_mean_grid takes it: a descriptor record (the layout of gpis_variance_grid) and voxels[k, j, i]"""

    def __init__(self, desc, voxels):
        self.desc = np.array(desc, dtype=DESC)
        self.voxels = np.ascontiguousarray(voxels, dtype=np.float32)
        d = self.desc["dims"]
        assert self.voxels.size == int(d[0]) * int(d[1]) * int(d[2])


class GridMeanRef:
    def __init__(self):
        L = self.lib = ctypes.CDLL(build())
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.grid_ref_density.argtypes = [vp, vp, sz, vp, vp]
        L.grid_ref_mean.argtypes = [vp, sz, vp, vp, vp]
        L.grid_ref_desc_size.restype = sz
        L.grid_ref_slot_size.restype = sz
        assert L.grid_ref_desc_size() == DESC.itemsize and L.grid_ref_slot_size() == ctypes.sizeof(_Slot)

    def density(self, grid, points):
        """VdbGrid::density(invNaturalTransform * Vec3f(p)) at double-precision world points (n, 3) -> float32 (n,)"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(p.shape[0], dtype=np.float32)
        self.lib.grid_ref_density(_p(grid.desc), _p(grid.voxels), p.shape[0], _p(p), _p(out))
        return out

    def mean(self, grid, points, offset=0.0, scale=1.0, volume=False):
        """(value, grad) of TabulatedMean::mean / dmean_da; grid = None: no grid set, the density is the background 0"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        s = _Slot(_p(grid.desc) if grid is not None else None, _p(grid.voxels) if grid is not None else None,
                  float(np.float32(offset)), float(np.float32(scale)), 1 if volume else 0)
        val = np.zeros(p.shape[0], dtype=np.float64)
        grad = np.zeros((p.shape[0], 3), dtype=np.float64)
        self.lib.grid_ref_mean(ctypes.byref(s), p.shape[0], _p(p), _p(val), _p(grad))
        return val, grad
