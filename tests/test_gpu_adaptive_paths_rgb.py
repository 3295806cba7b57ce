"""gpis_render_scene_s_paths_rgb_adaptive on the GPU.  Every sample of the library is a pure function of (x, y, k, scene_seed), so an
adaptive frame is, pixel by pixel, a concatenation of spp ranges gpis_render_scene_s_paths_rgb already renders: the per-sample RGB
values and segment counts come from that entry (one call per k, spp_count = 1, zeroed buffers), the schedule, the clamp and the
luminance from the restatement (tests/adaptive_paths_rgb_ref.py), and the entry's image, counts, records and info must equal the
composite bit for bit.  Then: the recorded fixture, the two stated consequences, chunking, tuning options, accumulation, the NULL
outputs and the refusals."""
import ctypes

import numpy as np
import pytest

import adaptive_paths_rgb_ref as apr
import adaptive_ref as ar
import paths_rgb_ref as prr
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

W, H = ar.SMALL_W, ar.SMALL_H
BOUNCES = 4


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    if not apr.available():
        pytest.skip("no C compiler for the restatement")
    return pkg, ob


def _scene(ob, spp=48, w=W, h=H, **fields):
    scene = ob.default_scene_s(w, h, spp)
    scene["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        scene[k] = v
    return scene


def _medium(pkg, name, emission=True, guide=None):
    params, albedo, guided = prr.CASES[name](pkg)
    m = pkg.Medium(params if emission else prr.without_emission(params))
    if guided if guide is None else guide:
        m.build_guide(*prr.GUIDE)
    return m, np.asarray(albedo, dtype=np.float32)


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


def _status(pkg, med, scene, adaptive, bounces, albedo, b, rad=True, cnt=True, seg=True, rec=True, info=True):
    """the entry's return value, on raw pointers"""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
    inf = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    st = med.L.lib.gpis_render_scene_s_paths_rgb_adaptive(med.h, _vp(sc), _vp(ad), int(bounces), _vp(alb), vp(b.rad.data_ptr()) if rad else None,
                                                          vp(b.cnt.data_ptr()) if cnt else None, vp(b.seg.data_ptr()) if seg else None,
                                                          vp(b.rec.data_ptr()) if rec else None, _vp(inf) if info else None, vp(stream_ptr()))
    return st, inf


def _adaptive(pkg, med, scene, albedo, bounces=BOUNCES, adaptive=None, into=None, **outputs):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, scene, ar.default_adaptive() if adaptive is None else adaptive, bounces, albedo, b, **outputs)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, scene, albedo, bounces=BOUNCES, into=None):
    """gpis_render_scene_s_paths_rgb: (image, segs)"""
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, seg = into or (torch.zeros(3 * h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    sc = np.array(scene, dtype=pkg.SCENE_S)
    med.call("gpis_render_scene_s_paths_rgb", sc, int(bounces), np.ascontiguousarray(albedo, dtype=np.float32), rad.data_ptr(), seg.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w, 3), seg.cpu().numpy().view(np.uint32).reshape(h, w)


def _composite(pkg, med, scene, albedo, bounces=BOUNCES, adaptive=None):
    return apr.frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                     apr.per_sample_rgb(lambda one: _uniform(pkg, med, one, albedo, bounces), scene))


def _equal(got, want):
    for k in apr.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


# name -> (medium case, guide, bounces, albedo or None for the case's own, scene fields)
CASES = {
    "grey_guided": ("grey", True, BOUNCES, None, {}),
    "ramp_emission": ("ramp", False, BOUNCES, None, {}),
    "rust_per_path": ("rust", False, 1, None, {}),                 # first-hit emission: this medium's march is the slow one, and every k is a call
    "short_last_pass": ("ramp", False, BOUNCES, None, {"spp_count": 40}),
    "first_hit_emission": ("ramp", False, 1, None, {}),
    "clamped_light": ("grey", True, BOUNCES, (0.9, 0.5, 0.1), {"light_radiance": 1e6}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composite(env, name):
    pkg, ob = env
    case, guide, bounces, albedo, fields = CASES[name]
    med, own = _medium(pkg, case, guide=guide)
    albedo = own if albedo is None else np.asarray(albedo, dtype=np.float32)
    scene = _scene(ob, **fields)
    if name == "rust_per_path":
        assert med.get_option("persistent") == 1
    want = _composite(pkg, med, scene, albedo, bounces)
    counts, rgb, flag = want["counts"], want["rgb"], want["clamped"].astype(bool)
    finite = rgb[np.isfinite(rgb)]
    print(name, want["info"], "k_used", want["k_used"], "largest component", float(finite.max()), "clamped samples", int(flag.sum()),
          "counts per pass", [(int(c.min()), int(c.max())) for c in counts])
    assert apr.is_real_schedule(counts)                                                  # a real schedule
    assert want["radiance_sum"].max() > 0 and want["seg_count"].max() > 0
    if name == "clamped_light":
        only0 = (rgb[..., 0] > 65536) & (rgb[..., 1] <= 65536) & (rgb[..., 2] <= 65536)
        print("over the limit in channel 0 only", int(only0.sum()), "unclamped non-zero", int((~flag & (rgb != 0).any(axis=-1)).sum()))
        assert only0.any() and flag[only0].all() and (~flag & (rgb != 0).any(axis=-1)).any()
        assert want["radiance_sum"].max() <= 65536.0 * want["sample_count"].max()
    else:
        assert not flag.any()
    if name == "short_last_pass":
        assert int(want["info"]["samples"]) < W * H * 40 and (counts.sum(axis=(1, 2))[2] < counts.sum(axis=(1, 2))[1])
    if name == "first_hit_emission":
        assert (want["segs"] <= 1).all()                                                 # one segment, no shadow ray
    got = _adaptive(pkg, med, scene, albedo, bounces)
    _equal(got, want)
    med.close()


def test_fixture(env):
    pkg, ob = env
    g = np.load(apr.GOLDEN)
    med = pkg.Medium(np.array(g["params"], dtype=pkg.PARAMS))
    scene, adaptive, albedo, bounces = np.array(g["scene"], dtype=pkg.SCENE_S), np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S), g["albedo"], int(g["max_bounces"])
    got = _adaptive(pkg, med, scene, albedo, bounces, adaptive)
    _equal(got, {k: g[k] for k in apr.KEYS})
    # and through the binding
    rad, cnt, segs, rec, info = med.render_scene_s_paths_rgb_adaptive(g["scene"], bounces, albedo, g["adaptive"], want_segs=True, want_records=True)
    _equal({"radiance_sum": rad, "sample_count": cnt, "seg_count": segs, "records": rec, "info": info}, got)
    rad2, cnt2, info2 = med.render_scene_s_paths_rgb_adaptive(g["scene"], bounces, albedo)
    assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
    # a scalar albedo is broadcast
    a = med.render_scene_s_paths_rgb_adaptive(g["scene"], 2, 0.5)
    b = med.render_scene_s_paths_rgb_adaptive(g["scene"], 2, (0.5, 0.5, 0.5))
    assert a[0].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    med.close()


def test_threshold_at_or_above_the_spp_is_uniform(env):
    """With threshold >= S every pass is uniform: the image is the sequence of the passes' gpis_render_scene_s_paths_rgb calls
    accumulated into one buffer, bit for bit (nothing is clamped), and every pixel has S samples."""
    import torch
    pkg, ob = env
    med, albedo = _medium(pkg, "ramp")
    for S, step in ((16, 16), (48, 48), (48, 16), (40, 16)):
        scene = _scene(ob, S)
        got = _adaptive(pkg, med, scene, albedo, adaptive=ar.default_adaptive(spp_step=step, threshold=max(S, 64) if S > 16 else 16))
        into = (torch.zeros(3 * H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        passes = 0
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, part, albedo, into=into)
            passes += 1
        assert want[0].max() > 0 and want[0].max() <= 65536
        assert np.array_equal(got["radiance_sum"].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got["seg_count"], want[1])
        assert (got["sample_count"] == S).all() and (got["records"]["sample_index"] == S).all()
        assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (passes, 0, W * H * S)
    med.close()


@pytest.mark.parametrize("name", ["grey_guided", "ramp_emission"])
def test_odd_spp_on_a_clipped_frame(env, name):
    """9 x 6 from the default distance: 3 x 2 records, the last column and the last row of tiles clipped.  5 spp in steps of 2 under a
    threshold no pass reaches are passes of 2, 2 and 1 samples: every record plans a single sample at last, and
    gpis_render_scene_s_paths_rgb runs odd counts beside it — per k for the composite, then the three passes' calls accumulated
    into one buffer."""
    import torch
    pkg, ob = env
    case, guide, bounces, _, _ = CASES[name]
    med, albedo = _medium(pkg, case, guide=guide)
    scene, settings = ob.default_scene_s(9, 6, 5), ar.default_adaptive(spp_step=2, threshold=64)
    want = _composite(pkg, med, scene, albedo, bounces, settings)
    print(name, want["info"], "clamped samples", int(want["clamped"].sum()), "image max", float(want["radiance_sum"].max()))
    assert want["records"].shape == (2, 3) and [np.unique(c).tolist() for c in want["counts"]] == [[2], [2], [1]]
    assert want["radiance_sum"].max() > 0 and want["seg_count"].max() > 0 and not want["clamped"].any()
    got = _adaptive(pkg, med, scene, albedo, bounces, settings)
    _equal(got, want)
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (3, 0, 9 * 6 * 5)
    into = (torch.zeros(3 * 6 * 9, dtype=torch.float32, device="cuda"), torch.zeros(6 * 9, dtype=torch.int32, device="cuda"))
    for k0, n in ((0, 2), (2, 2), (4, 1)):
        part = scene.copy()
        part["spp_begin"], part["spp_count"] = k0, n
        passes = _uniform(pkg, med, part, albedo, bounces, into=into)
    med.close()
    assert np.array_equal(got["radiance_sum"].view(np.uint32), passes[0].view(np.uint32)) and np.array_equal(got["seg_count"], passes[1])


def test_zero_radiance_stops_after_the_first_pass(env):
    """without emission and with max_path_bounces = 1 nothing is marched and every sample is zero"""
    pkg, ob = env
    med, albedo = _medium(pkg, "ramp", emission=False)
    got = _adaptive(pkg, med, _scene(ob, 48), albedo, bounces=1)
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 1, W * H * 16)
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all() and (got["seg_count"] == 0).all()
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["sample_count"] > 0).all() and (got["records"]["running_variance"] == 0).all()
    med.close()


def test_chunk_independence(env):
    """128 x 128 at 32 spp, 2 bounces: the first pass is 2^18 samples, 4 chunks at GPIS_OPT_CHUNK_LOG2 = 16 against one by default"""
    pkg, ob = env
    med, albedo = _medium(pkg, "grey", guide=True)
    scene = _scene(ob, 32, 128, 128)
    whole = _adaptive(pkg, med, scene, albedo, bounces=2)
    assert int(whole["info"]["passes_rendered"]) == 2 and int(whole["info"]["samples"]) > 4 * 65536
    assert whole["sample_count"].min() < 32 < whole["sample_count"].max() and whole["radiance_sum"].max() > 0
    med.set_option("chunk_log2", 16)
    _equal(_adaptive(pkg, med, scene, albedo, bounces=2), whole)
    med.close()


def test_tuning_options_change_nothing(env):
    pkg, ob = env
    med, albedo = _medium(pkg, "grey", guide=True)
    scene = _scene(ob)
    want = _adaptive(pkg, med, scene, albedo)
    for form in ("resident", "wave", "auto"):
        med.set_option("march_form", form)
        for sort, presort in ((1, 1), (1, 0), (0, 1), (0, 0)):
            med.set_option("paths_sort", sort)
            med.set_option("paths_presort", presort)
            _equal(_adaptive(pkg, med, scene, albedo), want)
    med.close()
    # the lane-per-ray kernels in place of the persistent march on the per-path medium
    med, albedo = _medium(pkg, "rust")
    want = _adaptive(pkg, med, scene, albedo)
    med.set_option("persistent", 0)
    _equal(_adaptive(pkg, med, scene, albedo), want)
    med.close()


def test_accumulation(env):
    """Buffers that hold values receive +=; records and info are those of the call.  Image: the frame's three pass sums are added to
    the buffer one after the other, the single frame's to zero: ((7 + a) + b) + c rounds three times, (a + b) + c twice, and with
    non-negative terms each rounding is off by at most 2^-24 of the final sum: five such errors separate the two."""
    pkg, ob = env
    med, albedo = _medium(pkg, "ramp")
    scene = _scene(ob)
    alone = _adaptive(pkg, med, scene, albedo)
    into = Buffers(W, H, fill=7)
    st, info = _status(pkg, med, scene, ar.default_adaptive(), BOUNCES, albedo, into)
    assert st == 0, med.L.last_error()
    both = into.host()
    assert np.array_equal(both["sample_count"], alone["sample_count"] + 7) and np.array_equal(both["seg_count"], alone["seg_count"] + 7)
    assert both["records"].tobytes() == alone["records"].tobytes() and info == alone["info"]
    total = alone["radiance_sum"].astype(np.float64) + 7.0
    err = np.abs(both["radiance_sum"].astype(np.float64) - total)
    print("largest difference / bound", float((err / (5 * 2.0 ** -24 * total)).max()))
    assert (both["radiance_sum"] > 7).any() and (err <= 5 * 2.0 ** -24 * total).all()
    # one pass: exactly 7 + the pass sum
    one = _scene(ob, 16)
    alone = _adaptive(pkg, med, one, albedo)
    into = Buffers(W, H, fill=7)
    assert _status(pkg, med, one, ar.default_adaptive(), BOUNCES, albedo, into)[0] == 0
    assert np.array_equal(into.host()["radiance_sum"], np.float32(7) + alone["radiance_sum"])
    med.close()


def test_null_outputs(env):
    pkg, ob = env
    med, albedo = _medium(pkg, "ramp")
    scene = _scene(ob)
    want = _adaptive(pkg, med, scene, albedo)
    for missing in ({"seg": False}, {"rec": False}, {"info": False}, {"seg": False, "rec": False, "info": False}):
        b = Buffers(W, H, fill=0)
        marker = Buffers(W, H, fill=7)
        for key, attr in (("seg", "seg"), ("rec", "rec")):
            if key in missing:
                setattr(b, attr, getattr(marker, attr))          # not passed: must stay as it is
        st, info = _status(pkg, med, scene, ar.default_adaptive(), BOUNCES, albedo, b, **missing)
        assert st == 0, med.L.last_error()
        out = b.host()
        assert out["radiance_sum"].tobytes() == want["radiance_sum"].tobytes() and np.array_equal(out["sample_count"], want["sample_count"])
        if "seg" in missing:
            assert (out["seg_count"] == 7).all()
        else:
            assert np.array_equal(out["seg_count"], want["seg_count"])
        if "rec" in missing:
            assert (out["records"].view(np.uint8) == 7).all()
        else:
            assert out["records"].tobytes() == want["records"].tobytes()
        assert info == (np.zeros((), dtype=pkg.ADAPTIVE_INFO) if "info" in missing else want["info"])
    med.close()


def test_refusals(env):
    pkg, ob = env
    import ws_oracle
    med, albedo = _medium(pkg, "ramp")
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    ok, good = _scene(ob, 16), ar.default_adaptive()
    cases = {
        "bounces 0": (med, ok, good, 0, albedo, {}),
        "bounces -3": (med, ok, good, -3, albedo, {}),
        "no albedo": (med, ok, good, BOUNCES, None, {}),
        "no image": (med, ok, good, BOUNCES, albedo, {"rad": False}),
        "weight-space handle": (ws, ok, good, BOUNCES, albedo, {}),
        "rows": (med, _scene(ob, 16, y_begin=1, y_count=H - 1), good, BOUNCES, albedo, {}),
        "fewer rows": (med, _scene(ob, 16, y_count=H - 2), good, BOUNCES, albedo, {}),
        "shards": (med, _scene(ob, 16, shard_count=2), good, BOUNCES, albedo, {}),
        "spp_step 0": (med, ok, ar.default_adaptive(spp_step=0), BOUNCES, albedo, {}),
        "threshold 1": (med, ok, ar.default_adaptive(threshold=1), BOUNCES, albedo, {}),
        "no settings": (med, ok, None, BOUNCES, albedo, {}),
        "no sample counts": (med, ok, good, BOUNCES, albedo, {"cnt": False}),
        "no samples": (med, _scene(ob, 0), good, BOUNCES, albedo, {}),
    }
    for name, (handle, scene, adaptive, bounces, alb, missing) in cases.items():
        b = Buffers(W, H, fill=7)
        st, info = _status(pkg, handle, scene, adaptive, bounces, alb, b, **missing)
        assert st == -1, (name, st)
        out = b.host()
        assert (out["radiance_sum"] == 7).all() and (out["sample_count"] == 7).all() and (out["seg_count"] == 7).all(), name
        assert (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), name
    assert _status(pkg, med, ok, good, BOUNCES, albedo, Buffers(W, H))[0] == 0
    ws.close()
    med.close()
