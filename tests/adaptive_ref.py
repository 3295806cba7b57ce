"""TEST INFRASTRUCTURE: ctypes wrapper of tests/native/adaptive_ref.c, the plain-C restatement of the adaptive sample schedule
(SampleRecord's Welford statistics, the plan step of PathTraceIntegrator::generateWork, the integrator's sampler and the pass
loop), compiled with the flags of oracle/Makefile.  The sample values come from the caller: frame() takes a function that
returns the unclamped contribution and the hit flag of the samples k < K of every pixel, and asks it for more while a pass needs
them."""
import ctypes
import os
import subprocess

import numpy as np

import ws_oracle

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "adaptive_ref.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libadaptive_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "adaptive_small.npz")
PINS = os.path.join(ROOT, "tests", "golden", "adaptive_ref_pins.npz")

ADAPTIVE_S = np.dtype([("spp_step", "<u4"), ("threshold", "<u4"), ("seed", "<u4"), ("_pad", "<u4")], align=True)
RECORD = np.dtype([("sample_count", "<u4"), ("next_sample_count", "<u4"), ("sample_index", "<u4"),
                   ("adaptive_weight", "<f4"), ("mean", "<f4"), ("running_variance", "<f4")], align=True)
INFO = np.dtype([("passes_rendered", "<u4"), ("stopped_early", "<u4"), ("samples", "<u8")], align=True)


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the adaptive-schedule restatement")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        L.adaptive_ref_rng_init.argtypes = [vp, u32, u32]
        L.adaptive_ref_rng_init.restype = ctypes.c_uint64
        L.adaptive_ref_add.argtypes = [vp, sz, vp, vp]
        L.adaptive_ref_add.restype = None
        L.adaptive_ref_plan.argtypes = [vp, u32, u32, u32, u32, vp, sz, vp]
        L.adaptive_ref_frame.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def default_adaptive(spp_step=16, threshold=16, seed=0xBA5EBA11):
    a = np.zeros((), dtype=ADAPTIVE_S)
    a["spp_step"], a["threshold"], a["seed"] = spp_step, threshold, seed
    return a


def rng_init(adaptive, width, height):
    return int(lib().adaptive_ref_rng_init(_p(np.array(adaptive, dtype=ADAPTIVE_S)), width, height))


def add_samples(values, record=None):
    """(record, variance, errorEstimate) after SampleRecord::addSample over `values`, starting from `record` (default: empty)"""
    rec = np.zeros((), dtype=RECORD) if record is None else np.array(record, dtype=RECORD).copy()
    v = np.ascontiguousarray(values, dtype=np.float32)
    out2 = np.zeros(2, dtype=np.float32)
    lib().adaptive_ref_add(_p(rec), v.size, _p(v), _p(out2))
    return rec, out2[0], out2[1]


def plan(adaptive, width, height, current_spp, pass_spp, rng_state, records):
    """one plan step: (return value, rng_state, records) — `records` is not modified"""
    rec = np.ascontiguousarray(records, dtype=RECORD).copy().reshape(-1)
    state = ctypes.c_uint64(rng_state)
    rc = lib().adaptive_ref_plan(_p(np.array(adaptive, dtype=ADAPTIVE_S)), width, height, current_spp, pass_spp, ctypes.byref(state), rec.size, _p(rec))
    return rc, state.value, rec


def frame(adaptive, width, height, spp_total, sample_values, max_passes=8):
    """The whole pass loop.  sample_values(k0, k1) -> (values, hits), arrays (height, width, k1 - k0) float32 / uint8 of the samples
    k0 <= k < k1 (relative to the scene's spp_begin).  Returns a dict: radiance_sum, sample_count, hit_count (height, width), records
    (vh, vw), info, counts (passes, vh, vw: next_sample_count per rendered pass) and k_used."""
    adaptive = np.array(adaptive, dtype=ADAPTIVE_S)
    vh, vw = (height + 3) // 4, (width + 3) // 4
    vals = np.zeros((height, width, 0), dtype=np.float32)
    hits = np.zeros((height, width, 0), dtype=np.uint8)
    need = spp_total
    while True:
        if need > vals.shape[2]:
            v, h = sample_values(vals.shape[2], need)
            vals = np.ascontiguousarray(np.concatenate([vals, np.asarray(v, dtype=np.float32)], axis=2))
            hits = np.ascontiguousarray(np.concatenate([hits, np.asarray(h, dtype=np.uint8)], axis=2))
        rad = np.zeros((height, width), dtype=np.float32)
        cnt = np.zeros((height, width), dtype=np.uint32)
        hit = np.zeros((height, width), dtype=np.uint32)
        rec = np.zeros((vh, vw), dtype=RECORD)
        info = np.zeros((), dtype=INFO)
        counts = np.zeros((max_passes, vh, vw), dtype=np.uint32)
        k_needed = ctypes.c_uint32(0)
        rc = lib().adaptive_ref_frame(_p(adaptive), width, height, spp_total, vals.shape[2], _p(vals), _p(hits), _p(rad), _p(cnt), _p(hit), _p(rec),
                                      _p(info), _p(counts), max_passes, ctypes.byref(k_needed))
        if rc == 0:
            n = min(int(info["passes_rendered"]), max_passes)
            return {"radiance_sum": rad, "sample_count": cnt, "hit_count": hit, "records": rec, "info": info, "counts": counts[:n], "k_used": vals.shape[2]}
        if rc != 1:
            raise RuntimeError("adaptive_ref_frame failed (%d)" % rc)
        need = int(k_needed.value)


# ---- the small whole-frame case of tests/golden/adaptive_small.npz: a C0 medium seen from twice the default distance, so that the
# 22 x 14 frame (tiles clipped on two edges, a 16-pixel tile boundary inside) has records of pure background
SMALL_W, SMALL_H, SMALL_SPP = 22, 14, 48


def small_scene(ob):
    scene = ob.default_scene_s(SMALL_W, SMALL_H, SMALL_SPP)
    scene["cam_pos"] = (0.0, 0.0, 8.0)
    return scene


def per_sample_values(render_one, scene):
    """sample_values for frame() from a renderer of the Lambert estimator: render_one(scene with spp_count = 1) -> (image, hits)"""
    def values(k0, k1):
        v = np.zeros((int(scene["height"]), int(scene["width"]), k1 - k0), dtype=np.float32)
        h = np.zeros(v.shape, dtype=np.uint8)
        for k in range(k0, k1):
            one = np.array(scene).copy()
            one["spp_begin"], one["spp_count"] = int(scene["spp_begin"]) + k, 1
            img, hits = render_one(one)
            v[:, :, k - k0], h[:, :, k - k0] = img, hits
        return v, h
    return values


def small_reference(pkg, ob):
    orc = ob.Oracle(pkg.params_for_config("C0"), threads=THREADS)
    scene = small_scene(ob)
    return frame(default_adaptive(), SMALL_W, SMALL_H, SMALL_SPP, per_sample_values(lambda s: orc.render_scene_s(s, want_hits=True), scene))


THREADS = 16
