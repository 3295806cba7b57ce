"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_paths_adaptive and gpis_render_scene_s_nee_paths_adaptive.  Every sample
of the two uniform entries is a pure function of (x, y, k, scene_seed), so an adaptive frame is, pixel by pixel, a concatenation
of spp ranges those entries already render.  The schedule, the clamp, the sums and the statistics are the restated pass loop of
tests/adaptive_ref.py (tests/native/adaptive_ref.c); the per-sample values E and, for the NEE driver, the per-sample segment counts
come from the caller, one sample index k at a time.  The segment counts travel in the `hits` slot of adaptive_ref.frame: a sample
marches at most 3 * (max_path_bounces - 1) <= 15 segments, which fits its uint8; its hit_count is then the expected seg_count.

On the CPU the per-sample values are the oracle's: oracle_render_scene_s_paths for the Lambert driver and the composite of
tests/nee_paths_ref.py for the NEE driver, each called with spp_count = 1."""
import os

import numpy as np

import adaptive_ref as ar
import nee_paths_ref as npr
import ws_oracle

ROOT = ws_oracle.ROOT
GOLDEN_LAMBERT = os.path.join(ROOT, "tests", "golden", "paths_adaptive_small.npz")
GOLDEN_NEE = os.path.join(ROOT, "tests", "golden", "nee_paths_adaptive_small.npz")

LAMBERT_KEYS = ("radiance_sum", "sample_count", "records", "info")
NEE_KEYS = ("radiance_sum", "sample_count", "seg_count", "records", "info")
LIMIT = 65536.0
ALBEDO = 0.8
GUIDE = (16, 8)                      # build_guide arguments of tests/test_gpu_nee_paths.py

# the fixtures: the 22 x 14 frame of adaptive_ref.small_scene; C0 at 4 bounces, and the `mis` case of nee_paths_ref.CASES at 3
SMALL_LAMBERT = ("C0", 4)
SMALL_NEE = ("mis", 3)


def available():
    return ar.available() and npr.available()


def scene(ob, spp=ar.SMALL_SPP, w=ar.SMALL_W, h=ar.SMALL_H, **fields):
    """the common frame: cam_pos = (0, 0, 8) unless `fields` says otherwise"""
    s = ob.default_scene_s(w, h, spp)
    s["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        s[k] = v
    return s


def frame(adaptive, width, height, spp_total, sample_values, max_passes=8):
    """The whole frame.  sample_values(k0, k1) -> (values, segs): arrays (height, width, k1 - k0) float32 and unsigned of the samples
    k0 <= k < k1 (relative to the scene's spp_begin), unclamped.  Returns the dict of adaptive_ref.frame with seg_count (its
    hit_count) and, of the samples k < k_used, values (unclamped) and segs."""
    store = {"values": np.zeros((height, width, 0), dtype=np.float32), "segs": np.zeros((height, width, 0), dtype=np.uint32)}

    def values(k0, k1):
        assert k0 == store["values"].shape[2]
        v, s = sample_values(k0, k1)
        v, s = np.asarray(v, dtype=np.float32), np.asarray(s, dtype=np.uint32)
        assert s.max(initial=0) <= 255
        store["values"] = np.concatenate([store["values"], v], axis=2)
        store["segs"] = np.concatenate([store["segs"], s], axis=2)
        return v, s.astype(np.uint8)
    ref = ar.frame(adaptive, width, height, spp_total, values, max_passes=max_passes)
    assert len(ref["counts"]) == int(ref["info"]["passes_rendered"]), "max_passes is below the number of passes"
    out = dict(ref)
    out["seg_count"] = out.pop("hit_count")
    out["values"], out["segs"] = store["values"], store["segs"]
    return out


def per_sample(render_one, scene):
    """sample_values for frame() from a renderer of a mono path estimator: render_one(scene with spp_count = 1) -> (image (H, W),
    seg_count (H, W) or None)"""
    def values(k0, k1):
        h, w = int(scene["height"]), int(scene["width"])
        v = np.zeros((h, w, k1 - k0), dtype=np.float32)
        segs = np.zeros((h, w, k1 - k0), dtype=np.uint32)
        for k in range(k0, k1):
            one = np.array(scene).copy()
            one["spp_begin"], one["spp_count"] = int(scene["spp_begin"]) + k, 1
            img, sg = render_one(one)
            v[:, :, k - k0] = img
            if sg is not None:
                segs[:, :, k - k0] = sg
        return v, segs
    return values


def generated(ref):
    """the unclamped values of every sample the composite asked its renderer for: k < k_used of every pixel"""
    return ref["values"].reshape(-1)


def spent(ref):
    """of those, the samples the schedule spent: sample k of a pixel for k below the pixel's sample count"""
    k = np.arange(ref["values"].shape[2])[None, None, :]
    return ref["values"][k < ref["sample_count"][:, :, None]]


def is_real_schedule(counts):
    """3 passes, the first uniform at 16, and a later pass with some count 1 and some count above 16 (the rule of
    adaptive_paths_rgb_ref.is_real_schedule)"""
    return len(counts) == 3 and bool((counts[0] == 16).all()) and any((c == 1).any() and (c > 16).any() for c in counts[1:])


def assert_clamp_case(ref):
    """some samples are over the limit and some non-zero ones are under it, among those the schedule spent too; none is non-finite.
    Returns the two counts among the generated samples."""
    g, u = generated(ref), spent(ref)
    assert np.isfinite(g).all()
    over, under = int((g > LIMIT).sum()), int(((g != 0) & (g <= LIMIT)).sum())
    assert (u > LIMIT).any() and ((u != 0) & (u <= LIMIT)).any() and over > 0 and under > 0, (over, under)
    return over, under


def assert_no_clamp(ref):
    g = generated(ref)
    assert np.isfinite(g).all() and not (g > LIMIT).any()


# ---- the CPU composites -------------------------------------------------------------------------------------------------------------
def cpu_lambert(pkg, ob, params, scene, max_bounces, albedo=ALBEDO, adaptive=None):
    orc = ob.Oracle(params, threads=ar.THREADS)
    return frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                 per_sample(lambda one: (orc.render_scene_s_paths(one, int(max_bounces), float(albedo)), None), scene))


def cpu_nee(pkg, ob, params, surface, scene, max_bounces, adaptive=None):
    orc = ob.Oracle(params, threads=ar.THREADS)
    ref = npr.NeePathsRef(pkg, ob)

    def render_one(one):
        c = ref.compose(orc, one, surface, int(max_bounces))
        return c.image, c.seg_count
    return frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                 per_sample(render_one, scene))


def small_lambert_inputs(pkg, ob):
    """(params, scene, adaptive, max_bounces, albedo) of tests/golden/paths_adaptive_small.npz"""
    return pkg.params_for_config(SMALL_LAMBERT[0]), scene(ob), ar.default_adaptive(), SMALL_LAMBERT[1], np.float32(ALBEDO)


def small_nee_inputs(pkg, ob):
    """(params, surface, scene, adaptive, max_bounces) of tests/golden/nee_paths_adaptive_small.npz"""
    params, surf, guide = npr.CASES[SMALL_NEE[0]](pkg)
    assert not guide
    return params, surf, scene(ob), ar.default_adaptive(), SMALL_NEE[1]


_memo = {}


def small_lambert_reference(pkg, ob):
    """the restated frame of the Lambert fixture on the CPU oracle (computed once per process)"""
    if "lambert" not in _memo:
        params, sc, adaptive, bounces, albedo = small_lambert_inputs(pkg, ob)
        _memo["lambert"] = cpu_lambert(pkg, ob, params, sc, bounces, albedo, adaptive)
    return _memo["lambert"]


def small_nee_reference(pkg, ob):
    """the restated frame of the NEE fixture on the CPU composite (computed once per process)"""
    if "nee" not in _memo:
        params, surf, sc, adaptive, bounces = small_nee_inputs(pkg, ob)
        _memo["nee"] = cpu_nee(pkg, ob, params, surf, sc, bounces, adaptive)
    return _memo["nee"]
