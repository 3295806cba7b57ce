"""TEST INFRASTRUCTURE of tests/test_gpu_paths_adaptive.py and tests/test_gpu_nee_paths_adaptive.py: device buffers, the raw calls of
the two adaptive entries and of their uniform entries, the composite (per-sample values from the uniform GPU entry, one call per k
with spp_count = 1 into zeroed buffers; schedule, clamp, sums and statistics from tests/paths_adaptive_ref.py) and the checks both
files share.  A driver is described by `Lambert(max_bounces, albedo)` or `Nee(surface, max_bounces)`."""
import ctypes

import numpy as np

import adaptive_ref as ar
import paths_adaptive_ref as par
from gpu_util import stream_ptr

W, H = ar.SMALL_W, ar.SMALL_H
MARK = 7


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


class Buffers:
    """device buffers of one frame; fill != 0 makes a write visible"""
    def __init__(self, w, h, fill=0):
        import torch
        self.w, self.h, self.vw, self.vh = w, h, (w + 3) // 4, (h + 3) // 4
        self.rad = torch.full((h * w,), float(fill), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.seg = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.rec = torch.full((self.vh * self.vw * ar.RECORD.itemsize,), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {"radiance_sum": self.rad.cpu().numpy().reshape(self.h, self.w), "sample_count": self.cnt.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "seg_count": self.seg.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "records": self.rec.cpu().numpy().view(ar.RECORD).reshape(self.vh, self.vw)}

    def untouched(self):
        out = self.host()
        return bool((out["radiance_sum"] == MARK).all() and (out["sample_count"] == MARK).all() and (out["seg_count"] == MARK).all()
                    and (out["records"].view(np.uint8) == MARK).all())


class Lambert:
    """gpis_render_scene_s_paths_adaptive over gpis_render_scene_s_paths; it has no seg_count"""
    keys = par.LAMBERT_KEYS
    entry, uniform_entry = "gpis_render_scene_s_paths_adaptive", "gpis_render_scene_s_paths"

    def __init__(self, max_bounces, albedo=par.ALBEDO):
        self.max_bounces, self.albedo = int(max_bounces), float(albedo)

    def status(self, pkg, med, scene, adaptive, b, rad=True, cnt=True, seg=True, rec=True, info=True):
        """the adaptive entry's return value, on raw pointers (seg is ignored: the entry takes none)"""
        sc = np.array(scene, dtype=pkg.SCENE_S)
        ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
        inf = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
        st = med.L.lib.gpis_render_scene_s_paths_adaptive(med.h, _vp(sc), _vp(ad), self.max_bounces, ctypes.c_float(self.albedo), _dp(b.rad) if rad else None,
                                                          _dp(b.cnt) if cnt else None, _dp(b.rec) if rec else None, _vp(inf) if info else None,
                                                          ctypes.c_void_p(stream_ptr()))
        return st, inf

    def uniform(self, pkg, med, scene, into=None):
        """gpis_render_scene_s_paths: (image, None)"""
        import torch
        h, w = int(scene["height"]), int(scene["width"])
        rad = into[0] if into else torch.zeros(h * w, dtype=torch.float32, device="cuda")
        med.call("gpis_render_scene_s_paths", np.array(scene, dtype=pkg.SCENE_S), self.max_bounces, ctypes.c_float(self.albedo), rad.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        return rad.cpu().numpy().reshape(h, w), None


class Nee:
    """gpis_render_scene_s_nee_paths_adaptive over gpis_render_scene_s_nee_paths"""
    keys = par.NEE_KEYS
    entry, uniform_entry = "gpis_render_scene_s_nee_paths_adaptive", "gpis_render_scene_s_nee_paths"

    def __init__(self, surface, max_bounces):
        self.surface, self.max_bounces = surface, int(max_bounces)

    def status(self, pkg, med, scene, adaptive, b, rad=True, cnt=True, seg=True, rec=True, info=True, surface=True):
        sc = np.array(scene, dtype=pkg.SCENE_S)
        ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
        sf = np.array(self.surface, dtype=pkg.SURFACE_S) if surface else None
        inf = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
        st = med.L.lib.gpis_render_scene_s_nee_paths_adaptive(med.h, _vp(sc), _vp(ad), _vp(sf), self.max_bounces, _dp(b.rad) if rad else None,
                                                              _dp(b.cnt) if cnt else None, _dp(b.seg) if seg else None, _dp(b.rec) if rec else None,
                                                              _vp(inf) if info else None, ctypes.c_void_p(stream_ptr()))
        return st, inf

    def uniform(self, pkg, med, scene, into=None):
        """gpis_render_scene_s_nee_paths: (image, segs)"""
        import torch
        h, w = int(scene["height"]), int(scene["width"])
        rad, seg = into or (torch.zeros(h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
        med.call("gpis_render_scene_s_nee_paths", np.array(scene, dtype=pkg.SCENE_S), np.array(self.surface, dtype=pkg.SURFACE_S), self.max_bounces,
                 rad.data_ptr(), seg.data_ptr(), stream_ptr())
        torch.cuda.synchronize()
        return rad.cpu().numpy().reshape(h, w), seg.cpu().numpy().view(np.uint32).reshape(h, w)


def adaptive(pkg, med, drv, scene, adaptive=None, into=None, **outputs):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = drv.status(pkg, med, scene, ar.default_adaptive() if adaptive is None else adaptive, b, **outputs)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def composite(pkg, med, drv, scene, adaptive=None):
    return par.frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                     par.per_sample(lambda one: drv.uniform(pkg, med, one), scene))


def equal(got, want, keys):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


def info_tuple(info):
    return int(info["passes_rendered"]), int(info["stopped_early"]), int(info["samples"])


def describe(name, want):
    g = par.generated(want)
    print(name, want["info"], "k_used", want["k_used"], "largest value", float(g.max()), "over the limit", int((g > par.LIMIT).sum()),
          "non-zero under it", int(((g != 0) & (g <= par.LIMIT)).sum()), "counts per pass", [(int(c.min()), int(c.max())) for c in want["counts"]])


def check_uniform_schedule(pkg, med, drv, ob, uniform=None):
    """With threshold >= S every pass is uniform: the image is the sequence of the passes' uniform calls accumulated into one
    buffer, bit for bit (nothing is clamped), and every pixel has S samples.  threshold = 64 at S = 48, and a short last pass."""
    import torch
    uniform = uniform or drv.uniform
    for S, step in ((48, 16), (40, 16)):
        scene = par.scene(ob, S)
        got = adaptive(pkg, med, drv, scene, adaptive=ar.default_adaptive(spp_step=step, threshold=64))
        into = (torch.zeros(H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        passes = 0
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            img, segs = uniform(pkg, med, part, into=into)
            passes += 1
        assert img.max() > 0 and img.max() <= par.LIMIT
        assert np.array_equal(got["radiance_sum"].view(np.uint32), img.view(np.uint32))
        if segs is not None:
            assert segs.max() > 0 and np.array_equal(got["seg_count"], segs)
        assert (got["sample_count"] == S).all() and (got["records"]["sample_index"] == S).all()
        assert info_tuple(got["info"]) == (passes, 0, W * H * S)


def check_odd_spp_on_a_clipped_frame(pkg, med, drv, ob):
    """9 x 6 from the default distance: 3 x 2 records, the last column and the last row of tiles clipped.  5 spp in steps of 2 under a
    threshold no pass reaches are passes of 2, 2 and 1 samples: every record plans a single sample at last, and the uniform entry
    runs odd counts beside it — per k for the composite, then the three passes' calls accumulated into one buffer."""
    import torch
    scene, settings = par.scene(ob, 5, 9, 6, cam_pos=(0.0, 0.0, 4.0)), ar.default_adaptive(spp_step=2, threshold=64)
    want = composite(pkg, med, drv, scene, settings)
    describe("9 x 6", want)
    assert want["records"].shape == (2, 3) and [np.unique(c).tolist() for c in want["counts"]] == [[2], [2], [1]]
    assert want["radiance_sum"].max() > 0
    par.assert_no_clamp(want)
    got = adaptive(pkg, med, drv, scene, settings)
    equal(got, want, drv.keys)
    assert info_tuple(got["info"]) == (3, 0, 9 * 6 * 5)
    into = (torch.zeros(6 * 9, dtype=torch.float32, device="cuda"), torch.zeros(6 * 9, dtype=torch.int32, device="cuda"))
    for k0, n in ((0, 2), (2, 2), (4, 1)):
        part = scene.copy()
        part["spp_begin"], part["spp_count"] = k0, n
        img, segs = drv.uniform(pkg, med, part, into=into)
    assert np.array_equal(got["radiance_sum"].view(np.uint32), img.view(np.uint32))
    if segs is not None:
        assert segs.max() > 0 and np.array_equal(got["seg_count"], segs)


def check_one_bounce(pkg, med, drv, ob):
    """max_path_bounces = 1: nothing is marched and every sample is zero; the plan step ends the frame after the first pass"""
    assert drv.max_bounces == 1
    got = adaptive(pkg, med, drv, par.scene(ob, 48))
    assert info_tuple(got["info"]) == (1, 1, 4928) and W * H * 16 == 4928
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all() and (got["seg_count"] == 0).all()
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["sample_count"] > 0).all() and (got["records"]["running_variance"] == 0).all()


def check_accumulation(pkg, med, drv, ob):
    """Buffers that hold values receive +=; records and info are those of the call.  Image: the frame's three pass sums are added to
    the buffer one after the other, the single frame's to zero: ((7 + a) + b) + c rounds three times, (a + b) + c twice, and with
    non-negative terms each rounding is off by at most 2^-24 of the final sum: five such errors separate the two."""
    scene = par.scene(ob)
    alone = adaptive(pkg, med, drv, scene)
    into = Buffers(W, H, fill=MARK)
    st, info = drv.status(pkg, med, scene, ar.default_adaptive(), into)
    assert st == 0, med.L.last_error()
    both = into.host()
    assert np.array_equal(both["sample_count"], alone["sample_count"] + MARK)
    if "seg_count" in drv.keys:
        assert np.array_equal(both["seg_count"], alone["seg_count"] + MARK)
    assert both["records"].tobytes() == alone["records"].tobytes() and info == alone["info"] and info_tuple(info)[0] == 3
    total = alone["radiance_sum"].astype(np.float64) + MARK
    err = np.abs(both["radiance_sum"].astype(np.float64) - total)
    print("largest difference / bound", float((err / (5 * 2.0 ** -24 * total)).max()))
    assert alone["radiance_sum"].min() >= 0 and (both["radiance_sum"] > MARK).any() and (err <= 5 * 2.0 ** -24 * total).all()
    # one pass: exactly 7 + the pass sum
    one = par.scene(ob, 16)
    alone = adaptive(pkg, med, drv, one)
    into = Buffers(W, H, fill=MARK)
    assert drv.status(pkg, med, one, ar.default_adaptive(), into)[0] == 0
    assert np.array_equal(into.host()["radiance_sum"], np.float32(MARK) + alone["radiance_sum"])


def check_null_outputs(pkg, med, drv, ob):
    scene = par.scene(ob)
    want = adaptive(pkg, med, drv, scene)
    optional = ("seg", "rec", "info") if "seg_count" in drv.keys else ("rec", "info")
    for missing in [{k: False} for k in optional] + [{k: False for k in optional}]:
        b = Buffers(W, H, fill=0)
        marker = Buffers(W, H, fill=MARK)
        for key in ("seg", "rec"):
            if key in missing:
                setattr(b, key, getattr(marker, key))          # not passed: must stay as it is
        st, info = drv.status(pkg, med, scene, ar.default_adaptive(), b, **missing)
        assert st == 0, med.L.last_error()
        out = b.host()
        assert out["radiance_sum"].tobytes() == want["radiance_sum"].tobytes() and np.array_equal(out["sample_count"], want["sample_count"])
        if "seg" in missing:
            assert (out["seg_count"] == MARK).all()
        elif "seg_count" in drv.keys:
            assert np.array_equal(out["seg_count"], want["seg_count"])
        if "rec" in missing:
            assert (out["records"].view(np.uint8) == MARK).all()
        else:
            assert out["records"].tobytes() == want["records"].tobytes()
        assert info == (np.zeros((), dtype=pkg.ADAPTIVE_INFO) if "info" in missing else want["info"])


def common_refusals(ob, med, ws, drv, make):
    """name -> (handle, driver, scene, adaptive, outputs not passed): what both entries refuse.  make(max_bounces) is the driver with
    another bounce count."""
    ok, good = par.scene(ob, 16), ar.default_adaptive()
    return {
        "bounces 0": (med, make(0), ok, good, {}),
        "bounces -3": (med, make(-3), ok, good, {}),
        "no image": (med, drv, ok, good, {"rad": False}),
        "weight-space handle": (ws, drv, ok, good, {}),
        "rows": (med, drv, par.scene(ob, 16, y_begin=1, y_count=H - 1), good, {}),
        "fewer rows": (med, drv, par.scene(ob, 16, y_count=H - 2), good, {}),
        "rows past the image": (med, drv, par.scene(ob, 16, y_begin=10, y_count=H), good, {}),
        "shards": (med, drv, par.scene(ob, 16, shard_count=2), good, {}),
        "bad shard": (med, drv, par.scene(ob, 16, shard_count=2, shard_index=2), good, {}),
        "spp_step 0": (med, drv, ok, ar.default_adaptive(spp_step=0), {}),
        "threshold 1": (med, drv, ok, ar.default_adaptive(threshold=1), {}),
        "no settings": (med, drv, ok, None, {}),
        "no sample counts": (med, drv, ok, good, {"cnt": False}),
        "no samples": (med, drv, par.scene(ob, 0), good, {}),
    }


def check_refusals(pkg, cases):
    for name, (handle, drv, scene, settings, missing) in cases.items():
        b = Buffers(W, H, fill=MARK)
        st, info = drv.status(pkg, handle, scene, settings, b, **missing)
        assert st == -1, (name, st)
        assert b.untouched() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), name
