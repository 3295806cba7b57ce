"""gpis_ws_render_scene_s_adaptive and gpis_ws_render_scene_s_paths_adaptive on the GPU.  A sample is a pure function of
(x, y, k, scene_seed), so an adaptive frame is, pixel by pixel, a concatenation of spp ranges the uniform drivers already render: the
per-sample values come from gpis_ws_render_scene_s / gpis_ws_render_scene_s_paths (one call per k, spp_count = 1), the schedule from
the plain-C restatement (tests/adaptive_ref.py), and image, counts, records and info must equal that composite bit for bit.  Then:
the clamp, the early stop, the uniform limits, chunking, accumulation, the recorded fixture and the bindings, and the refusals.
Nothing has a tolerance but the one test_accumulation derives.

Counters.  The uniform drivers render whole rows, so their per-call counters cannot be taken apart record by record, and a schedule
gives every record its own sample count.  What the schedule's samples cost is therefore measured on the device through the batch
entries: the staged composite (tests/ws_adaptive_ref.py, BatchMarch) marches exactly the segments of exactly those samples, and a
segment costs the same n_eval / n_spec / n_seg there as in the fused frame kernels — test_staged_costs_equal_the_uniform_drivers
checks that on whole frames, where the uniform drivers can be asked.  Where a frame's schedule is uniform (the uniform limit) the
counters are compared with the uniform drivers' own."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import ws_adaptive_ref as wa
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

W, H = wa.W, wa.H
ENTRY = {"lambert": "gpis_ws_render_scene_s_adaptive", "paths": "gpis_ws_render_scene_s_paths_adaptive"}


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return pkg, ob


@pytest.fixture(scope="module")
def cpu(pkg, ob):
    return wa.CpuRenderer(pkg, ob)


class Buffers:
    """device buffers of one frame; fill != 0 makes a write visible"""
    def __init__(self, w=W, h=H, fill=0):
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


def _status(pkg, med, driver, scene, adaptive, b, chunk_log2=0, bounces=wa.BOUNCES, rad=True, cnt=True, no_scene=False):
    """the entry's return value, on raw pointers.  The path entry has no hit_count: b.hit stays as it was filled."""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    head = [med.h, None if no_scene else vp(sc.ctypes.data), None if ad is None else vp(ad.ctypes.data), int(chunk_log2)]
    bufs = [vp(b.rad.data_ptr()) if rad else None, vp(b.cnt.data_ptr()) if cnt else None]
    tail = [vp(b.rec.data_ptr()), vp(info.ctypes.data), vp(stream_ptr())]
    if driver == "lambert":
        st = med.L.lib.gpis_ws_render_scene_s_adaptive(*head, *bufs, vp(b.hit.data_ptr()), *tail)
    else:
        st = med.L.lib.gpis_ws_render_scene_s_paths_adaptive(*head, int(bounces), ctypes.c_float(wa.ALBEDO), *bufs, *tail)
    return st, info


def _adaptive(pkg, med, driver, scene, adaptive=None, into=None, **kw):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, driver, scene, ar.default_adaptive() if adaptive is None else adaptive, b, **kw)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, driver, scene, into=None, bounces=wa.BOUNCES):
    """gpis_ws_render_scene_s / gpis_ws_render_scene_s_paths: (image, hits), the hits of the path driver being none"""
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, hits = into or (torch.zeros(h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    sc = np.array(scene, dtype=pkg.SCENE_S)
    vp = ctypes.c_void_p
    if driver == "lambert":
        st = med.L.lib.gpis_ws_render_scene_s(med.h, vp(sc.ctypes.data), vp(rad.data_ptr()), vp(hits.data_ptr()), vp(stream_ptr()))
    else:
        st = med.L.lib.gpis_ws_render_scene_s_paths(med.h, vp(sc.ctypes.data), int(bounces), ctypes.c_float(wa.ALBEDO), vp(rad.data_ptr()), vp(stream_ptr()))
    assert st == 0, med.L.last_error()
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w), hits.cpu().numpy().view(np.uint32).reshape(h, w)


_COMPOSITES = {}


def _composite(pkg, ob, name):
    """the GPU-sampled composite of a case, computed once: the schedule over per-sample values of the uniform driver"""
    if name not in _COMPOSITES:
        driver, p, w, scene = wa.case_inputs(pkg, ob, name)
        med = pkg.WeightSpaceMedium(p, w)
        _COMPOSITES[name] = wa.frame(lambda one: _uniform(pkg, med, driver, one), scene)
        med.close()
    return _COMPOSITES[name]


def _staged_costs(pkg, cpu, driver, p, w, scene, per_pixel):
    """the device's counters for the samples k < per_pixel[y, x] of every pixel, through the batch entries"""
    med = pkg.WeightSpaceMedium(p, w)
    med.reset_counters()
    _, n_seg = cpu.costs(driver, p, w, scene, per_pixel, march=wa.BatchMarch(pkg, med))
    c = med.counters()
    med.close()
    assert c["n_seg"] == n_seg                   # the composite counted the segments it handed over
    return c


def _equal(got, want):
    for k in ("radiance_sum", "sample_count", "hit_count", "records", "info"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


@pytest.mark.parametrize("name", ["lambert_renewal", "lambert_single", "paths_renewal", "paths_global"])
def test_staged_costs_equal_the_uniform_drivers(env, cpu, name):
    """what the counter checks below stand on: over a whole frame of 3 spp, the staged composite through the batch entries advances
    n_eval, n_spec and n_seg by what one uniform-driver call advances them"""
    pkg, ob = env
    driver, p, w, scene = wa.case_inputs(pkg, ob, name)
    scene["spp_count"] = 3
    med = pkg.WeightSpaceMedium(p, w)
    med.reset_counters()
    img, _ = _uniform(pkg, med, driver, scene)
    want = med.counters()
    med.close()
    got = _staged_costs(pkg, cpu, driver, p, w, scene, np.full((H, W), 3))
    print(name, got, want)
    assert img.max() > 0 and want["n_seg"] > 0 and got == want


@pytest.mark.parametrize("name", sorted(wa.CASES))
def test_composite(env, cpu, name):
    pkg, ob = env
    driver, p, w, scene = wa.case_inputs(pkg, ob, name)
    want = _composite(pkg, ob, name)
    print(name, want["info"], "k_used", want["k_used"], "largest value", want["largest_value"], "counts per pass", [(int(c.min()), int(c.max())) for c in want["counts"]])
    wa.check_schedule(want)
    assert want["largest_value"] <= 65536 and want["radiance_sum"].max() > 0
    if int(scene["spp_count"]) == 40:
        assert int(want["info"]["samples"]) < W * H * 40
    if driver == "lambert":
        assert want["hit_count"].max() > 0
    med = pkg.WeightSpaceMedium(p, w)
    med.reset_counters()
    got = _adaptive(pkg, med, driver, scene)
    c = med.counters()
    med.close()
    _equal(got, want)
    # the samples the schedule used — per record sample_index of them, not the k_used prefix — cost what they cost one by one
    per_tile = want["counts"].sum(axis=0)
    assert np.array_equal(per_tile, want["records"]["sample_index"])
    cost = _staged_costs(pkg, cpu, driver, p, w, scene, want["sample_count"])
    print(name, "counters", c, "the same samples staged", cost)
    assert c == cost and c["n_spec"] >= c["n_eval"] > 0


@pytest.mark.parametrize("name", sorted(wa.CLAMP_CASES))
def test_clamp(env, name):
    pkg, ob = env
    driver, p, w, scene = wa.case_inputs(pkg, ob, name)
    want = _composite(pkg, ob, name)
    print(name, want["info"], "largest value", want["largest_value"], "image max", float(want["radiance_sum"].max()))
    assert want["largest_value"] > 65536 and want["radiance_sum"].max() > 0
    med = pkg.WeightSpaceMedium(p, w)
    _equal(_adaptive(pkg, med, driver, scene), want)
    med.close()


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_all_zero_samples_stop_after_the_first_pass(env, driver):
    """no light for the Lambert frame, one bounce (no next-event estimation) for the path driver"""
    pkg, ob = env
    p, w = wa.medium(pkg, ctx="renewal", n_basis=32)
    med = pkg.WeightSpaceMedium(p, w)
    if driver == "lambert":
        got = _adaptive(pkg, med, driver, wa.scene(ob, light_radiance=0.0))
        assert got["hit_count"].max() > 0
    else:
        got = _adaptive(pkg, med, driver, wa.scene(ob), bounces=1)
    med.close()
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 1, W * H * 16)
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all()
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["running_variance"] == 0).all()


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_threshold_at_or_above_the_spp_is_uniform(env, driver):
    """A frame of one pass below the threshold is one uniform-driver call, bit for bit, counters included.  With several passes
    below the threshold the image is the sequence of the passes' calls accumulated into one buffer."""
    import torch
    pkg, ob = env
    p, w = wa.medium(pkg, ctx="renewal", n_basis=32)
    med = pkg.WeightSpaceMedium(p, w)
    for S, step in ((16, 16), (48, 48), (48, 16), (40, 16)):
        scene = wa.scene(ob, S)
        med.reset_counters()
        got = _adaptive(pkg, med, driver, scene, ar.default_adaptive(spp_step=step, threshold=max(S, 64)) if S > 16 else None)
        c_got = med.counters()
        into = (torch.zeros(H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        med.reset_counters()
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, driver, part, into)
        c_want = med.counters()
        assert want[0].max() > 0
        assert np.array_equal(got["radiance_sum"].view(np.uint32), want[0].view(np.uint32)) and (got["sample_count"] == S).all()
        assert np.array_equal(got["hit_count"], want[1]) and (driver == "paths" or want[1].max() > 0)
        assert (got["records"]["sample_index"] == S).all()
        assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == ((S + step - 1) // step, 0, W * H * S)
        assert c_got == c_want and c_got["n_seg"] > 0, (c_got, c_want)
    med.close()


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_odd_spp_on_a_clipped_frame(env, driver):
    """9 x 6 from the default distance: 3 x 2 records, the last column and the last row of tiles clipped.  5 spp in steps of 2 under a
    threshold no pass reaches are passes of 2, 2 and 1 samples: every record plans a single sample at last, and the uniform driver
    runs odd counts beside it — per k for the composite, then the three passes' calls accumulated into one buffer."""
    import torch
    pkg, ob = env
    p, w = wa.medium(pkg, ctx="renewal", n_basis=32)
    med = pkg.WeightSpaceMedium(p, w)
    scene, settings = ob.default_scene_s(9, 6, 5), ar.default_adaptive(spp_step=2, threshold=64)
    want = wa.frame(lambda one: _uniform(pkg, med, driver, one), scene, settings)
    print(driver, want["info"], "largest value", want["largest_value"], "image max", float(want["radiance_sum"].max()))
    assert want["records"].shape == (2, 3) and [np.unique(c).tolist() for c in want["counts"]] == [[2], [2], [1]]
    assert 0 < want["largest_value"] <= 65536 and (driver == "paths" or want["hit_count"].max() > 0)
    got = _adaptive(pkg, med, driver, scene, settings)
    _equal(got, want)
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (3, 0, 9 * 6 * 5)
    into = (torch.zeros(6 * 9, dtype=torch.float32, device="cuda"), torch.zeros(6 * 9, dtype=torch.int32, device="cuda"))
    for k0, n in ((0, 2), (2, 2), (4, 1)):
        part = scene.copy()
        part["spp_begin"], part["spp_count"] = k0, n
        passes = _uniform(pkg, med, driver, part, into)
    med.close()
    assert np.array_equal(got["radiance_sum"].view(np.uint32), passes[0].view(np.uint32)) and np.array_equal(got["hit_count"], passes[1])


@pytest.mark.parametrize("name", ["lambert_renewal", "paths_renewal"])
def test_chunk_independence(env, name):
    """chunk_log2 8: a full record of the first pass (16 pixels x 16 samples) is exactly one chunk and the clipped bottom-row records
    share chunks; later passes hold records above the chunk (16 pixels x more than 16 samples) and chunks of many count-1 records.
    Everything, counters included, is what the one-chunk passes of chunk_log2 0 give."""
    pkg, ob = env
    driver, p, w, scene = wa.case_inputs(pkg, ob, name)
    counts = _composite(pkg, ob, name)["counts"]
    assert counts[1:].max() * 16 > 256 and (counts[1:] == 1).sum() >= 2
    med = pkg.WeightSpaceMedium(p, w)
    runs = {}
    for l in (0, 8, 10):
        med.reset_counters()
        runs[l] = (_adaptive(pkg, med, driver, scene, chunk_log2=l), med.counters())
    med.close()
    _equal(runs[0][0], _composite(pkg, ob, name))
    for l in (8, 10):
        _equal(runs[l][0], runs[0][0])
        assert runs[l][1] == runs[0][1], (l, runs[l][1], runs[0][1])


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_accumulation(env, driver):
    """Two calls (spp_begin 0 and 64) into the same buffers.  Counts add exactly.  With one pass per call the image is the sum of the
    two single-call images bit for bit; with three passes per call the six pass sums are added one after the other, not pairwise:
    twelve float32 additions of non-negative terms separate the two orders, each off by at most 2^-24 of the final sum."""
    pkg, ob = env
    p, w = wa.medium(pkg, ctx="renewal", n_basis=32)
    med = pkg.WeightSpaceMedium(p, w)
    for S in (16, 48):
        a, b = wa.scene(ob, S), wa.scene(ob, S, spp_begin=64)
        ra, rb = _adaptive(pkg, med, driver, a), _adaptive(pkg, med, driver, b)
        assert not np.array_equal(ra["radiance_sum"], rb["radiance_sum"])
        into = Buffers()
        _adaptive(pkg, med, driver, a, into=into)
        both = _adaptive(pkg, med, driver, b, into=into)
        assert np.array_equal(both["sample_count"], ra["sample_count"] + rb["sample_count"])
        assert np.array_equal(both["hit_count"], ra["hit_count"] + rb["hit_count"])
        assert both["records"].tobytes() == rb["records"].tobytes()              # the records are those of the call
        total = ra["radiance_sum"] + rb["radiance_sum"]
        if S == 16:
            assert np.array_equal(both["radiance_sum"], total)
        else:
            assert int(ra["info"]["passes_rendered"]) == 3 and int(rb["info"]["passes_rendered"]) == 3
            err = np.abs(both["radiance_sum"].astype(np.float64) - total.astype(np.float64))
            print(driver, "largest difference / bound", float((err[total > 0] / (12 * 2.0 ** -24 * total[total > 0])).max()))
            assert (err <= 12 * 2.0 ** -24 * total.astype(np.float64)).all()
    med.close()


def test_fixture_and_bindings(env):
    pkg, ob = env
    g = np.load(wa.GOLDEN)
    for tag, driver in (("lambert", "lambert"), ("paths", "paths")):
        p = np.array(g[tag + "_params"]).view(pkg.PARAMS).reshape(())
        w = np.array(g[tag + "_ws"]).view(pkg.WS_PARAMS).reshape(())
        scene = np.array(g[tag + "_scene"]).view(pkg.SCENE_S).reshape(())
        adaptive = np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S)
        want = {k: g[tag + "_" + k] for k in ("radiance_sum", "sample_count", "hit_count", "records", "info")}
        med = pkg.WeightSpaceMedium(p, w)
        got = _adaptive(pkg, med, driver, scene, adaptive, bounces=int(g["max_bounces"]))
        _equal(got, want)
        assert np.float32(wa.ALBEDO) == g["albedo"]
        if driver == "lambert":
            rad, cnt, hits, rec, info = med.render_scene_s_adaptive(scene, adaptive, want_hits=True, want_records=True)
            _equal({"radiance_sum": rad, "sample_count": cnt, "hit_count": hits, "records": rec, "info": info}, got)
            rad2, cnt2, info2 = med.render_scene_s_adaptive(scene, chunk_log2=9)
        else:
            rad, cnt, rec, info = med.render_scene_s_paths_adaptive(scene, int(g["max_bounces"]), float(g["albedo"]), adaptive, want_records=True)
            _equal({"radiance_sum": rad, "sample_count": cnt, "hit_count": got["hit_count"], "records": rec, "info": info}, got)
            rad2, cnt2, info2 = med.render_scene_s_paths_adaptive(scene, int(g["max_bounces"]), float(g["albedo"]), chunk_log2=9)
        assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
        med.close()


def test_refusals(env):
    pkg, ob = env
    p, w = wa.medium(pkg, ctx="renewal", n_basis=8)
    ws = pkg.WeightSpaceMedium(p, w)
    sc = pkg.Medium(pkg.params_for_config("C0"))
    ok, good = wa.scene(ob, 16), ar.default_adaptive()
    cases = {
        "sparse-convolution handle": (sc, ok, good, {}),
        "rows": (ws, wa.scene(ob, 16, y_begin=1, y_count=H - 1), good, {}),
        "fewer rows": (ws, wa.scene(ob, 16, y_count=H - 2), good, {}),
        "shards": (ws, wa.scene(ob, 16, shard_count=2), good, {}),
        "spp_step 0": (ws, ok, ar.default_adaptive(spp_step=0), {}),
        "threshold 1": (ws, ok, ar.default_adaptive(threshold=1), {}),
        "no samples": (ws, wa.scene(ob, 0), good, {}),
        "no scene": (ws, ok, good, {"no_scene": True}),
        "no settings": (ws, ok, None, {}),
        "no image": (ws, ok, good, {"rad": False}),
        "no sample counts": (ws, ok, good, {"cnt": False}),
        "chunk_log2 7": (ws, ok, good, {"chunk_log2": 7}),
        "chunk_log2 1": (ws, ok, good, {"chunk_log2": 1}),
        "chunk_log2 29": (ws, ok, good, {"chunk_log2": 29}),
        "chunk_log2 -1": (ws, ok, good, {"chunk_log2": -1}),
        "no bounces": (ws, ok, good, {"bounces": 0}),
        "negative bounces": (ws, ok, good, {"bounces": -2}),
        # a first pass of 2^24 + 1 samples per pixel: a full record would hold more than 2^28 samples
        "a record above 2^28 samples": (ws, wa.scene(ob, (1 << 24) + 1), ar.default_adaptive(spp_step=(1 << 24) + 1, threshold=1 << 30), {}),
    }
    for name, (handle, scene, adaptive, how) in cases.items():
        for driver in ("lambert", "paths"):
            if "bounces" in name and driver == "lambert":
                continue
            b = Buffers(fill=7)
            st, info = _status(pkg, handle, driver, scene, adaptive, b, **how)
            assert st == (-2 if "2^28" in name else -1), (name, driver, st)
            out = b.host()
            assert (out["radiance_sum"] == 7).all() and (out["sample_count"] == 7).all() and (out["hit_count"] == 7).all(), (name, driver)
            assert (out["records"].view(np.uint8) == 7).all() and info == np.zeros((), dtype=pkg.ADAPTIVE_INFO), (name, driver)
    for l in (0, 8, 28):
        for driver in ("lambert", "paths"):
            assert _status(pkg, ws, driver, ok, good, Buffers(), chunk_log2=l)[0] == 0, (l, driver)
    # and the sparse-convolution entry keeps refusing a weight-space handle
    b, info = Buffers(fill=7), np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    s16, ad = np.array(ok, dtype=pkg.SCENE_S), np.array(good, dtype=pkg.ADAPTIVE_S)
    assert ws.L.lib.gpis_render_scene_s_adaptive(ws.h, vp(s16.ctypes.data), vp(ad.ctypes.data), vp(b.rad.data_ptr()), vp(b.cnt.data_ptr()), vp(b.hit.data_ptr()),
                                                 vp(b.rec.data_ptr()), vp(info.ctypes.data), vp(stream_ptr())) == -1
    assert (b.host()["radiance_sum"] == 7).all()
    ws.close()
    sc.close()
