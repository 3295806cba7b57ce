"""gpis_render_scene_s_adaptive on the GPU.  Every sample of the library is a pure function of (x, y, k, scene_seed), so an adaptive
frame is, pixel by pixel, a concatenation of spp ranges gpis_render_scene_s already renders: the per-sample values come from that
entry (one call per k, spp_count = 1), the schedule from the plain-C restatement (tests/adaptive_ref.py), and the entry's image,
counts, records and info must equal the composite bit for bit — on the full-record and the 32-byte-record body, a per-path medium, a
light bright enough for the clamp and a short last pass.  Then: the recorded fixture, the uniform limits, the early stop, chunking,
accumulation and the refusals."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

W, H = ar.SMALL_W, ar.SMALL_H


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return pkg, ob


def _scene(ob, spp=48, w=W, h=H, **fields):
    scene = ob.default_scene_s(w, h, spp)
    scene["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        scene[k] = v
    return scene


class Buffers:
    """device buffers of one frame; fill != 0 makes a write visible"""
    def __init__(self, w, h, fill=0):
        import torch
        self.w, self.h, self.vw, self.vh = w, h, (w + 3) // 4, (h + 3) // 4
        self.rad = torch.full((h * w,), float(fill), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.hit = torch.full((h * w,), fill, dtype=torch.int32, device="cuda")
        self.rec = torch.full((self.vh * self.vw * ar.RECORD.itemsize,), fill, dtype=torch.uint8, device="cuda")

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {"radiance_sum": self.rad.cpu().numpy().reshape(self.h, self.w), "sample_count": self.cnt.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "hit_count": self.hit.cpu().numpy().view(np.uint32).reshape(self.h, self.w),
                "records": self.rec.cpu().numpy().view(ar.RECORD).reshape(self.vh, self.vw)}


def _status(pkg, med, scene, adaptive, b, rad=True, cnt=True):
    """the entry's return value, on raw pointers"""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    st = med.L.lib.gpis_render_scene_s_adaptive(med.h, vp(sc.ctypes.data), None if ad is None else vp(ad.ctypes.data), vp(b.rad.data_ptr()) if rad else None,
                                                vp(b.cnt.data_ptr()) if cnt else None, vp(b.hit.data_ptr()), vp(b.rec.data_ptr()),
                                                vp(info.ctypes.data), vp(stream_ptr()))
    return st, info


def _adaptive(pkg, med, scene, adaptive=None, into=None):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, scene, ar.default_adaptive() if adaptive is None else adaptive, b)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, scene, into=None):
    """gpis_render_scene_s: (image, hits)"""
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, hits = into or (torch.zeros(h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    sc = np.array(scene, dtype=pkg.SCENE_S)
    med.call("gpis_render_scene_s", sc.ctypes.data_as(ctypes.c_void_p), rad.data_ptr(), hits.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w), hits.cpu().numpy().view(np.uint32).reshape(h, w)


def _composite(pkg, med, scene, adaptive=None):
    seen = []

    def render_one(one):
        img, hits = _uniform(pkg, med, one)
        seen.append(float(img.max()))
        return img, hits
    ref = ar.frame(ar.default_adaptive() if adaptive is None else adaptive, int(scene["width"]), int(scene["height"]), int(scene["spp_count"]),
                   ar.per_sample_values(render_one, scene))
    ref["largest_value"] = max(seen)
    return ref


def _equal(got, want):
    for k in ("radiance_sum", "sample_count", "hit_count", "records", "info"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


def _c0(pkg):
    return pkg.Medium(pkg.params_for_config("C0"))


def _c1_guided(pkg):
    med = pkg.Medium(pkg.params_for_config("C1"))
    med.build_guide(16, 8)
    assert med.get_option("scene_compact") == 1 and med.get_option("scene_exit_state") == 0      # the 32-byte-record body
    return med


def _per_path(pkg):
    p = pkg.params_for_config("C0")
    p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL       # a realization per (pixel, k): k reaches the seed
    return pkg.Medium(p)


CASES = {
    "c0_full_records": (_c0, {}),
    "c1_guided_compact": (_c1_guided, {}),
    "per_path_renewal": (_per_path, {}),
    "clamped_light": (_c0, {"light_radiance": 1e5}),
    "short_last_pass": (_c0, {"spp_count": 40}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_composite(env, name):
    pkg, ob = env
    make, fields = CASES[name]
    med, scene = make(pkg), _scene(ob, **fields)
    want = _composite(pkg, med, scene)
    counts, S = want["counts"], int(scene["spp_count"])
    print(name, want["info"], "k_used", want["k_used"], "largest value", want["largest_value"], "counts per pass", [(int(c.min()), int(c.max())) for c in counts])
    assert len(counts) == 3 and (counts[0] == 16).all() and (counts[1:] == 1).any() and counts[1].max() > 16          # a real schedule
    if name == "clamped_light":
        assert want["largest_value"] > 65536 and 0 < want["radiance_sum"].max() <= 65536.0 * want["sample_count"].max()
    else:
        assert want["largest_value"] <= 65536
    if name == "short_last_pass":
        assert int(want["info"]["samples"]) < W * H * 40
    got = _adaptive(pkg, med, scene)
    _equal(got, want)


def test_fixture(env):
    pkg, ob = env
    g = np.load(ar.GOLDEN)
    med = pkg.Medium(np.array(g["params"], dtype=pkg.PARAMS))
    got = _adaptive(pkg, med, np.array(g["scene"], dtype=pkg.SCENE_S), np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S))
    _equal(got, {k: g[k] for k in ("radiance_sum", "sample_count", "hit_count", "records", "info")})
    # and through the binding
    rad, cnt, hits, rec, info = med.render_scene_s_adaptive(g["scene"], g["adaptive"], want_hits=True, want_records=True)
    _equal({"radiance_sum": rad, "sample_count": cnt, "hit_count": hits, "records": rec, "info": info}, got)
    rad2, cnt2, info2 = med.render_scene_s_adaptive(g["scene"])
    assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info


def test_threshold_at_or_above_the_spp_is_uniform(env):
    """A frame of one pass below the threshold is one gpis_render_scene_s call, bit for bit.  With several passes below the threshold
    the image is the sequence of the passes' calls accumulated — each pass adds its own sum, as the contract states — and every
    pixel has S samples."""
    pkg, ob = env
    med = _c0(pkg)
    one = _scene(ob, 16)
    got = _adaptive(pkg, med, one)                                     # threshold 16 >= S = 16
    want = _uniform(pkg, med, one)
    assert want[0].max() > 0
    assert np.array_equal(got["radiance_sum"], want[0]) and np.array_equal(got["hit_count"], want[1]) and (got["sample_count"] == 16).all()
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 0, W * H * 16)
    for S, step in ((48, 48), (48, 16), (40, 16)):
        scene = _scene(ob, S)
        got = _adaptive(pkg, med, scene, ar.default_adaptive(spp_step=step, threshold=max(S, 64)))
        import torch
        into = (torch.zeros(H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, part, into)
        assert np.array_equal(got["radiance_sum"], want[0]) and np.array_equal(got["hit_count"], want[1]) and (got["sample_count"] == S).all()
        assert (got["records"]["sample_index"] == S).all() and int(got["info"]["samples"]) == W * H * S


@pytest.mark.parametrize("name", ["c0_full_records", "c1_guided_compact"])
def test_odd_spp_on_a_clipped_frame(env, name):
    """9 x 6 from the default distance: 3 x 2 records, the last column and the last row of tiles clipped.  5 spp in steps of 2 under a
    threshold no pass reaches are passes of 2, 2 and 1 samples: every record plans a single sample at last, and gpis_render_scene_s
    runs odd counts beside it — per k for the composite, then the three passes' calls accumulated into one buffer."""
    import torch
    pkg, ob = env
    med = CASES[name][0](pkg)
    scene, settings = ob.default_scene_s(9, 6, 5), ar.default_adaptive(spp_step=2, threshold=64)
    want = _composite(pkg, med, scene, settings)
    print(name, want["info"], "largest value", want["largest_value"], "image max", float(want["radiance_sum"].max()))
    assert want["records"].shape == (2, 3) and [np.unique(c).tolist() for c in want["counts"]] == [[2], [2], [1]]
    assert 0 < want["largest_value"] <= 65536 and want["hit_count"].max() > 0
    got = _adaptive(pkg, med, scene, settings)
    _equal(got, want)
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (3, 0, 9 * 6 * 5)
    into = (torch.zeros(6 * 9, dtype=torch.float32, device="cuda"), torch.zeros(6 * 9, dtype=torch.int32, device="cuda"))
    for k0, n in ((0, 2), (2, 2), (4, 1)):
        part = scene.copy()
        part["spp_begin"], part["spp_count"] = k0, n
        passes = _uniform(pkg, med, part, into)
    assert np.array_equal(got["radiance_sum"].view(np.uint32), passes[0].view(np.uint32)) and np.array_equal(got["hit_count"], passes[1])


def test_zero_radiance_stops_after_the_first_pass(env):
    pkg, ob = env
    got = _adaptive(pkg, _c0(pkg), _scene(ob, 48, light_radiance=0.0))
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 1, W * H * 16)
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all() and got["hit_count"].max() > 0
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["running_variance"] == 0).all()


def test_chunk_independence(env):
    """256 x 256 at 32 spp: at GPIS_OPT_CHUNK_LOG2 = 16 (the smallest) the first pass alone is 16 chunks"""
    pkg, ob = env
    med = _c1_guided(pkg)
    scene = _scene(ob, 32, 256, 256, cam_pos=(0.0, 0.0, 4.0))
    whole = _adaptive(pkg, med, scene)
    assert int(whole["info"]["passes_rendered"]) == 2 and int(whole["info"]["samples"]) > 2 * 4 * 65536
    assert whole["sample_count"].min() < 32 < whole["sample_count"].max()
    med.set_option("chunk_log2", 16)
    try:
        _equal(_adaptive(pkg, med, scene), whole)
        med.set_option("scene_compact", 0)                  # and the full-record body gives the same frame
        _equal(_adaptive(pkg, med, scene), whole)
    finally:
        med.set_option("scene_compact", 1)
        med.set_option("chunk_log2", 0)


def test_accumulation(env):
    """Two calls (spp_begin 0 and 64) into the same buffers.  Counts add exactly.  With one pass per call the image is the sum of the
    two single-call images bit for bit; with three passes per call the six pass sums are added one after the other, not pairwise:
    twelve float32 additions of non-negative terms separate the two orders, each off by at most 2^-24 of the final sum."""
    pkg, ob = env
    med = _c0(pkg)
    for S in (16, 48):
        a, b = _scene(ob, S), _scene(ob, S, spp_begin=64)
        ra, rb = _adaptive(pkg, med, a), _adaptive(pkg, med, b)
        assert not np.array_equal(ra["radiance_sum"], rb["radiance_sum"])
        into = Buffers(W, H)
        _adaptive(pkg, med, a, into=into)
        both = _adaptive(pkg, med, b, into=into)
        assert np.array_equal(both["sample_count"], ra["sample_count"] + rb["sample_count"])
        assert np.array_equal(both["hit_count"], ra["hit_count"] + rb["hit_count"])
        assert both["records"].tobytes() == rb["records"].tobytes()              # the records are those of the call
        total = ra["radiance_sum"] + rb["radiance_sum"]
        if S == 16:
            assert np.array_equal(both["radiance_sum"], total)
        else:
            err = np.abs(both["radiance_sum"].astype(np.float64) - total.astype(np.float64))
            print("largest difference / bound", float((err[total > 0] / (12 * 2.0 ** -24 * total[total > 0])).max()))
            assert (err <= 12 * 2.0 ** -24 * total.astype(np.float64)).all()


def test_refusals(env):
    pkg, ob = env
    import ws_oracle
    med = _c0(pkg)
    p, w = ws_oracle.ws_params(pkg)
    ws = pkg.WeightSpaceMedium(p, w)
    ok, good = _scene(ob, 16), ar.default_adaptive()
    cases = {
        "rows": (med, _scene(ob, 16, y_begin=1, y_count=H - 1), good, {}),
        "fewer rows": (med, _scene(ob, 16, y_count=H - 2), good, {}),
        "shards": (med, _scene(ob, 16, shard_count=2), good, {}),
        "spp_step 0": (med, ok, ar.default_adaptive(spp_step=0), {}),
        "threshold 1": (med, ok, ar.default_adaptive(threshold=1), {}),
        "no settings": (med, ok, None, {}),
        "no image": (med, ok, good, {"rad": False}),
        "no sample counts": (med, ok, good, {"cnt": False}),
        "weight-space handle": (ws, ok, good, {}),
        "no samples": (med, _scene(ob, 0), good, {}),
    }
    for name, (handle, scene, adaptive, missing) in cases.items():
        b = Buffers(W, H, fill=7)
        st, info = _status(pkg, handle, scene, adaptive, b, **missing)
        assert st == -1, (name, st)
        out = b.host()
        assert (out["radiance_sum"] == 7).all() and (out["sample_count"] == 7).all() and (out["hit_count"] == 7).all(), name
        assert (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), name
    assert _status(pkg, med, ok, good, Buffers(W, H))[0] == 0
