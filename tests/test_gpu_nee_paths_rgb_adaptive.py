"""gpis_render_scene_s_nee_paths_rgb_adaptive on the GPU.  Every sample of the library is a pure function of (x, y, k, scene_seed), so
an adaptive frame is, pixel by pixel, a concatenation of spp ranges gpis_render_scene_s_nee_paths_rgb already renders (and
tests/test_gpu_nee_paths_rgb.py pins to the CPU composite): the per-sample RGB values and segment counts come from that entry (one
call per k, spp_count = 1, zeroed buffers), the schedule from tests/adaptive_ref.py's plain-C plan, the clamp and the luminance from
tests/adaptive_paths_rgb_ref.py, and the entry's image, counts, records and info must equal the composite bit for bit — as
tests/test_gpu_adaptive_paths_rgb.py does for the Lambert driver.  Frames are 22 x 14 at 32 spp in steps of 16: one uniform and one
planned pass."""
import ctypes

import numpy as np
import pytest

import adaptive_paths_rgb_ref as apr
import adaptive_ref as ar
import nee_paths_rgb_ref as rgb
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

W, H, SPP = ar.SMALL_W, ar.SMALL_H, 32
BOUNCES = 4
ENTRY = "gpis_render_scene_s_nee_paths_rgb_adaptive"


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not apr.available():
        pytest.skip("no C compiler for the restatement")
    return pkg, ob


def _scene(ob, spp=SPP, w=W, h=H, **fields):
    scene = ob.default_scene_s(w, h, spp)
    scene["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        scene[k] = v
    return scene


def _medium(pkg, name, emission=True):
    params, surf = rgb.CASES[name](pkg)
    return pkg.Medium(params if emission else rgb.without_emission(params)), surf


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Buffers:
    """device buffers of one frame; fill != 0 makes a write visible"""
    def __init__(self, w, h, fill=0):
        import torch
        self.w, self.h, self.vw, self.vh = w, h, (w + 3) // 4, (h + 3) // 4
        self.rad = torch.full((3 * h * w,), float(fill), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.seg = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.rec = torch.full((self.vh * self.vw * ar.RECORD.itemsize,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {"radiance_sum": self.rad.cpu().numpy().reshape(self.h, self.w, 3), "sample_count": self.cnt.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "seg_count": self.seg.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "records": self.rec.cpu().numpy().view(ar.RECORD).reshape(self.vh, self.vw)}


def _status(pkg, med, scene, adaptive, surf, bounces, b, rad=True, cnt=True, seg=True, rec=True, info=True):
    """the entry's return value, on raw pointers"""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    sf = None if surf is None else np.array(surf, dtype=pkg.SURFACE_RGB_S)
    inf = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    st = getattr(med.L.lib, ENTRY)(med.h, _vp(sc), _vp(ad), _vp(sf), int(bounces), vp(b.rad.data_ptr()) if rad else None,
                                   vp(b.cnt.data_ptr()) if cnt else None, vp(b.seg.data_ptr()) if seg else None,
                                   vp(b.rec.data_ptr()) if rec else None, _vp(inf) if info else None, vp(stream_ptr()))
    return st, inf


def _adaptive(pkg, med, scene, surf, bounces=BOUNCES, adaptive=None, into=None, **outputs):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, scene, ar.default_adaptive() if adaptive is None else adaptive, surf, bounces, b, **outputs)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, scene, surf, bounces=BOUNCES, into=None):
    """gpis_render_scene_s_nee_paths_rgb: (image, segs)"""
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, seg = into or (torch.zeros(3 * h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    med.call("gpis_render_scene_s_nee_paths_rgb", np.array(scene, dtype=pkg.SCENE_S), np.array(surf, dtype=pkg.SURFACE_RGB_S), int(bounces), rad.data_ptr(),
             seg.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w, 3), seg.cpu().numpy().view(np.uint32).reshape(h, w)


def _composite(pkg, med, scene, surf, bounces=BOUNCES, adaptive=None):
    return apr.frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                     apr.per_sample_rgb(lambda one: _uniform(pkg, med, one, surf, bounces), scene))


def _equal(got, want):
    for k in apr.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


# name -> (case of nee_paths_rgb_ref.CASES, bounces, surface fields, scene fields).  clamped_light: per unit of cap_radiance the non-zero
# samples of this frame's CPU composite have a median of 0.013 and a largest value of 0.85, so a light of 3e6 in channel 0 puts
# a good part of them over 65536 there and leaves the rest, and every value of the other two channels, under it
CASES = {
    "mis": ("mis", BOUNCES, {}, {}),
    "uni": ("uni", BOUNCES, {}, {}),
    "emission": (rgb.EMISSIVE_CASE, BOUNCES, {}, {}),
    "first_hit_emission": (rgb.EMISSIVE_CASE, 1, {}, {}),
    "short_last_pass": ("nee", BOUNCES, {}, {"spp_count": 24}),
    "clamped_light": ("mis", BOUNCES, {"cap_radiance": (3e6, 10.0, 10.0)}, {}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composite(env, name):
    pkg, ob = env
    case, bounces, surface_fields, fields = CASES[name]
    med, surf = _medium(pkg, case)
    surf = rgb.copper(pkg, cap_cos=float(surf["cap_cos"]), **surface_fields)
    scene = _scene(ob, **fields)
    want = _composite(pkg, med, scene, surf, bounces)
    counts, values, flag = want["counts"], want["rgb"], want["clamped"].astype(bool)
    finite = values[np.isfinite(values)]
    print(name, want["info"], "k_used", want["k_used"], "largest component", float(finite.max()), "clamped samples", int(flag.sum()),
          "counts per pass", [(int(c.min()), int(c.max())) for c in counts])
    # a real schedule: a uniform pass of 16, then a planned pass with tiles at one sample and tiles above the step
    assert len(counts) == 2 and (counts[0] == 16).all() and (counts[1] == 1).any() and (counts[1] > int(scene["spp_count"]) - 16).any()
    assert want["radiance_sum"].max() > 0 and want["seg_count"].max() > 0
    if name == "clamped_light":
        only0 = (values[..., 0] > 65536) & (values[..., 1] <= 65536) & (values[..., 2] <= 65536)
        print("over the limit in channel 0 only", int(only0.sum()), "unclamped non-zero", int((~flag & (values != 0).any(axis=-1)).sum()))
        assert only0.any() and flag[only0].all() and (~flag & (values != 0).any(axis=-1)).any()
        assert (want["segs"][flag] > 0).all()                                            # a clamped sample's segments count
    else:
        assert not flag.any()
    if name == "first_hit_emission":
        assert (want["segs"] <= 1).all()                                                 # one segment, no shadow ray
    got = _adaptive(pkg, med, scene, surf, bounces)
    _equal(got, want)
    if name == "mis":                                                                    # and through the binding
        rad, cnt, segs, rec, info = med.render_scene_s_nee_paths_rgb_adaptive(scene, surf, bounces, want_segs=True, want_records=True)
        _equal({"radiance_sum": rad, "sample_count": cnt, "seg_count": segs, "records": rec, "info": info}, got)
        rad2, cnt2, info2 = med.render_scene_s_nee_paths_rgb_adaptive(scene, surf, bounces, ar.default_adaptive())
        assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
    med.close()


def test_threshold_at_or_above_the_spp_is_uniform(env):
    """With threshold >= S every pass is uniform: the image is the sequence of the passes' gpis_render_scene_s_nee_paths_rgb calls
    accumulated into one buffer, bit for bit (nothing is clamped), and every pixel has S samples."""
    import torch
    pkg, ob = env
    med, surf = _medium(pkg, rgb.EMISSIVE_CASE)
    for S, step in ((16, 16), (32, 16), (24, 16)):
        scene = _scene(ob, S)
        got = _adaptive(pkg, med, scene, surf, adaptive=ar.default_adaptive(spp_step=step, threshold=64))
        into = (torch.zeros(3 * H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        passes = 0
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, part, surf, into=into)
            passes += 1
        assert want[0].max() > 0 and want[0].max() <= 65536
        assert np.array_equal(got["radiance_sum"].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got["seg_count"], want[1])
        assert (got["sample_count"] == S).all() and (got["records"]["sample_index"] == S).all()
        assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (passes, 0, W * H * S)
    med.close()


def test_zero_radiance_stops_after_the_first_pass(env):
    """without emission and with max_path_bounces = 1 nothing is marched and every sample is zero"""
    pkg, ob = env
    med, surf = _medium(pkg, rgb.EMISSIVE_CASE, emission=False)
    got = _adaptive(pkg, med, _scene(ob), surf, bounces=1)
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 1, W * H * 16)
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all() and (got["seg_count"] == 0).all()
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["running_variance"] == 0).all()
    med.close()


def test_chunk_independence_and_tuning_options(env):
    """chunks of 2^8 samples — one record of the uniform pass (16 pixels x 16 samples) each, and a record of the planned pass that
    holds more is a chunk of its own — against one chunk per pass; then the lane-per-ray kernels in place of the persistent march"""
    pkg, ob = env
    med, surf = _medium(pkg, rgb.EMISSIVE_CASE)
    scene = _scene(ob)
    whole = _adaptive(pkg, med, scene, surf)
    assert int(whole["info"]["passes_rendered"]) == 2 and whole["sample_count"].min() < SPP < whole["sample_count"].max()
    med.set_option("chunk_log2", 8)
    _equal(_adaptive(pkg, med, scene, surf), whole)
    med.set_option("chunk_log2", 0)
    med.set_option("persistent", 0)
    _equal(_adaptive(pkg, med, scene, surf), whole)
    med.close()


def test_accumulation_and_null_outputs(env):
    """one pass into buffers that hold 7: exactly 7 + the pass sum; seg_count, records and info may be NULL and are then left alone"""
    pkg, ob = env
    med, surf = _medium(pkg, "mis")
    one = _scene(ob, 16)
    alone = _adaptive(pkg, med, one, surf)
    into = Buffers(W, H, fill=7)
    st, info = _status(pkg, med, one, ar.default_adaptive(), surf, BOUNCES, into, seg=False, rec=False, info=False)
    assert st == 0, med.L.last_error()
    out = into.host()
    assert alone["radiance_sum"].any() and np.array_equal(out["radiance_sum"], np.float32(7) + alone["radiance_sum"])
    assert np.array_equal(out["sample_count"], alone["sample_count"] + 7)
    assert (out["seg_count"] == 7).all() and (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    med.close()


def test_refusals(env):
    pkg, ob = env
    import ws_oracle
    med, surf = _medium(pkg, "mis")
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    ok, good = _scene(ob, 16), ar.default_adaptive()
    cases = {
        "bounces 0": (med, ok, good, surf, 0, {}),
        "no surface": (med, ok, good, None, BOUNCES, {}),
        "cap_cos 1": (med, ok, good, rgb.copper(pkg, cap_cos=1.0), BOUNCES, {}),
        "cap_cos -1": (med, ok, good, rgb.copper(pkg, cap_cos=-1.0), BOUNCES, {}),
        "no image": (med, ok, good, surf, BOUNCES, {"rad": False}),
        "weight-space handle": (ws, ok, good, surf, BOUNCES, {}),
        "rows": (med, _scene(ob, 16, y_begin=1, y_count=H - 1), good, surf, BOUNCES, {}),
        "shards": (med, _scene(ob, 16, shard_count=2), good, surf, BOUNCES, {}),
        "spp_step 0": (med, ok, ar.default_adaptive(spp_step=0), surf, BOUNCES, {}),
        "threshold 1": (med, ok, ar.default_adaptive(threshold=1), surf, BOUNCES, {}),
        "no settings": (med, ok, None, surf, BOUNCES, {}),
        "no sample counts": (med, ok, good, surf, BOUNCES, {"cnt": False}),
        "no samples": (med, _scene(ob, 0), good, surf, BOUNCES, {}),
    }
    for name, (handle, scene, adaptive, sf, bounces, missing) in cases.items():
        b = Buffers(W, H, fill=7)
        st, info = _status(pkg, handle, scene, adaptive, sf, bounces, b, **missing)
        assert st == -1, (name, st)
        out = b.host()
        assert (out["radiance_sum"] == 7).all() and (out["sample_count"] == 7).all() and (out["seg_count"] == 7).all(), name
        assert (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), name
    assert _status(pkg, med, ok, good, surf, BOUNCES, Buffers(W, H))[0] == 0
    ws.close()
    med.close()
