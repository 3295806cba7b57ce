"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_paths_rgb_adaptive.  The schedule is the restated pass loop of
tests/adaptive_ref.py, fed with the clamped luminance of every sample; the clamp and the luminance are the plain-C restatement
tests/native/adaptive_rgb_value.c (compiled with the flags of oracle/Makefile); image, sample and segment counts are re-summed here
in numpy float32 from the per-pass counts the loop returns: per pixel, pass and channel from zero in sample order, then added to
the image once.  The per-sample RGB values and segment counts come from the caller, one sample index k at a time."""
import ctypes
import os
import subprocess

import numpy as np

import adaptive_ref as ar
import ws_oracle

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "adaptive_rgb_value.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libadaptive_rgb_value.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "adaptive_paths_rgb_small.npz")
PINS = os.path.join(ROOT, "tests", "golden", "adaptive_rgb_pins.npz")

# the small whole-frame case of the fixture: adaptive_ref.small_scene, the `ramp` case of paths_rgb_ref.CASES
SMALL_CASE, SMALL_BOUNCES = "ramp", 4
KEYS = ("radiance_sum", "sample_count", "seg_count", "records", "info")


def available():
    return ar.available()


def build():
    deps = [SRC, os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the clamp and luminance restatement")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


_lib = None


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def value(rgb):
    """(clamped rgb, luminance, clamp flag) of the samples rgb[..., 3]"""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.adaptive_rgb_value_ref.argtypes = [ctypes.c_size_t] + [ctypes.c_void_p] * 4
        _lib.adaptive_rgb_value_ref.restype = None
    v = np.ascontiguousarray(rgb, dtype=np.float32)
    assert v.shape[-1] == 3
    out, lum, flag = np.zeros_like(v), np.zeros(v.shape[:-1], dtype=np.float32), np.zeros(v.shape[:-1], dtype=np.uint8)
    _lib.adaptive_rgb_value_ref(lum.size, _p(v), _p(out), _p(lum), _p(flag))
    return out, lum, flag


def frame(adaptive, width, height, spp_total, sample_rgb, max_passes=8, drive=None):
    """The whole frame.  sample_rgb(k0, k1) -> (rgb, segs): arrays (height, width, k1 - k0, 3) float32 and (height, width, k1 - k0)
    uint32 of the samples k0 <= k < k1 (relative to the scene's spp_begin), unclamped.  `drive`: what the statistics see of a clamped
    sample (default: its luminance).  Returns a dict: radiance_sum (height, width, 3), sample_count, seg_count (height, width),
    records (vh, vw), info, counts (passes, vh, vw), k_used, and of the samples k < k_used: rgb (unclamped), clamped (flag), segs."""
    store = {"rgb": np.zeros((height, width, 0, 3), dtype=np.float32), "segs": np.zeros((height, width, 0), dtype=np.uint32)}

    def values(k0, k1):
        assert k0 == store["rgb"].shape[2]
        rgb, segs = sample_rgb(k0, k1)
        store["rgb"] = np.concatenate([store["rgb"], np.asarray(rgb, dtype=np.float32)], axis=2)
        store["segs"] = np.concatenate([store["segs"], np.asarray(segs, dtype=np.uint32)], axis=2)
        clamped_rgb, lum, _ = value(rgb)
        return (lum if drive is None else drive(clamped_rgb)), np.zeros(lum.shape, dtype=np.uint8)
    ref = ar.frame(adaptive, width, height, spp_total, values, max_passes=max_passes)
    counts = ref["counts"]
    assert len(counts) == int(ref["info"]["passes_rendered"]), "max_passes is below the number of passes"
    rgb, segs = store["rgb"], store["segs"]
    clamped_rgb, _, flag = value(rgb)
    img = np.zeros((height, width, 3), dtype=np.float32)
    cnt = np.zeros((height, width), dtype=np.uint32)
    seg = np.zeros((height, width), dtype=np.uint32)
    begin = np.zeros(counts.shape[1:], dtype=np.uint32)
    for c in counts:
        for y in range(height):
            for x in range(width):
                b, n = int(begin[y // 4, x // 4]), int(c[y // 4, x // 4])
                acc = np.zeros(3, dtype=np.float32)
                for i in range(b, b + n):
                    acc = acc + clamped_rgb[y, x, i]              # float32 + float32, per channel
                img[y, x] = img[y, x] + acc
                cnt[y, x] += n
                seg[y, x] += segs[y, x, b:b + n].sum(dtype=np.uint32)
        begin += c
    assert np.array_equal(cnt, ref["sample_count"])
    return {"radiance_sum": img, "sample_count": cnt, "seg_count": seg, "records": ref["records"], "info": ref["info"], "counts": counts,
            "k_used": rgb.shape[2], "rgb": rgb, "clamped": flag, "segs": segs}


def per_sample_rgb(render_one, scene):
    """sample_rgb for frame() from a renderer of the RGB path estimator: render_one(scene with spp_count = 1) -> (image (H, W, 3),
    seg_count (H, W))"""
    def values(k0, k1):
        h, w = int(scene["height"]), int(scene["width"])
        rgb = np.zeros((h, w, k1 - k0, 3), dtype=np.float32)
        segs = np.zeros((h, w, k1 - k0), dtype=np.uint32)
        for k in range(k0, k1):
            one = np.array(scene).copy()
            one["spp_begin"], one["spp_count"] = int(scene["spp_begin"]) + k, 1
            img, sg = render_one(one)
            rgb[:, :, k - k0], segs[:, :, k - k0] = img, sg
        return rgb, segs
    return values


def is_real_schedule(counts):
    """3 passes, the first uniform at 16, and a later pass with some count 1 and some count above 16"""
    return len(counts) == 3 and bool((counts[0] == 16).all()) and any((c == 1).any() and (c > 16).any() for c in counts[1:])


def small_inputs(pkg, ob):
    """(params, albedo, scene, adaptive) of the fixture"""
    import paths_rgb_ref as pr
    params, albedo, guide = pr.CASES[SMALL_CASE](pkg)
    assert not guide
    return params, np.asarray(albedo, dtype=np.float32), ar.small_scene(ob), ar.default_adaptive()


_memo = {}


def small_reference(pkg, ob, drive=None):
    """the restated frame of the fixture on the CPU oracle (computed once per process and `drive`); the per-sample values are
    computed once and shared"""
    import paths_rgb_ref as pr
    key = "luminance" if drive is None else drive.__name__
    if key not in _memo:
        params, albedo, scene, adaptive = small_inputs(pkg, ob)
        if "samples" not in _memo:
            orc = ob.Oracle(params, threads=ar.THREADS)
            ref = pr.PathsRgbRef(pkg, ob)
            cache = {}

            def render_one(one):
                k = int(one["spp_begin"])
                if k not in cache:
                    c = ref.compose(orc, one, SMALL_BOUNCES, albedo)
                    cache[k] = (c.image, c.seg_count)
                return cache[k]
            _memo["samples"] = per_sample_rgb(render_one, scene)
        _memo[key] = frame(adaptive, ar.SMALL_W, ar.SMALL_H, ar.SMALL_SPP, _memo["samples"], drive=drive)
    return _memo[key]
