"""gpis_fs_render_scene_s_adaptive and gpis_fs_render_scene_s_paths_adaptive on the GPU.  A sample is a pure function of
(x, y, k, scene_seed), so an adaptive frame is, pixel by pixel, a concatenation of spp ranges the uniform drivers already render: the
per-sample values and counts come from gpis_fs_render_scene_s / gpis_fs_render_scene_s_paths (one call per k, spp_count = 1), the
schedule from the plain-C restatement (tests/adaptive_ref.py), and image, sample counts, hit / segment counts, records and info must
equal that composite bit for bit.  Then: the clamp, the early stop, the uniform limits, chunking, accumulation, repeatability, the
recorded fixture (the CPU composite's) and the bindings, the refusals, and the uniform entries' own fixtures on a handle the adaptive
entries have used.  Nothing has a tolerance but the one test_accumulation derives for a re-associated sum."""
import ctypes
import os

import numpy as np
import pytest

import adaptive_ref as ar
import fs_adaptive_ref as fa
from gpu_util import stream_ptr

pytestmark = pytest.mark.gpu

W, H = fa.W, fa.H


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return pkg, ob


class Buffers:
    """device buffers of one frame; fill != 0 makes a write visible.  `hit` is hit_count for the frame driver, seg_count for the
    path driver."""
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


def _status(pkg, med, driver, scene, adaptive, b, bounces=fa.BOUNCES, rad=True, cnt=True, no_scene=False, no_handle=False, no_count=False):
    """the entry's return value, on raw pointers"""
    sc = np.array(scene, dtype=pkg.SCENE_S)
    ad = None if adaptive is None else np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    head = [None if no_handle else med.h, None if no_scene else vp(sc.ctypes.data), None if ad is None else vp(ad.ctypes.data)]
    bufs = [vp(b.rad.data_ptr()) if rad else None, vp(b.cnt.data_ptr()) if cnt else None, None if no_count else vp(b.hit.data_ptr())]
    tail = [vp(b.rec.data_ptr()), vp(info.ctypes.data), vp(stream_ptr())]
    if driver == "lambert":
        st = med.L.lib.gpis_fs_render_scene_s_adaptive(*head, *bufs, *tail)
    else:
        st = med.L.lib.gpis_fs_render_scene_s_paths_adaptive(*head, int(bounces), ctypes.c_float(fa.ALBEDO), *bufs, *tail)
    return st, info


def _adaptive(pkg, med, driver, scene, adaptive=None, into=None, **kw):
    b = into or Buffers(int(scene["width"]), int(scene["height"]))
    st, info = _status(pkg, med, driver, scene, ar.default_adaptive() if adaptive is None else adaptive, b, **kw)
    assert st == 0, med.L.last_error()
    out = b.host()
    out["info"] = info
    return out


def _uniform(pkg, med, driver, scene, into=None, bounces=fa.BOUNCES):
    """gpis_fs_render_scene_s / gpis_fs_render_scene_s_paths: (image, hits or segments)"""
    import torch
    h, w = int(scene["height"]), int(scene["width"])
    rad, cnt = into or (torch.zeros(h * w, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.int32, device="cuda"))
    sc = np.array(scene, dtype=pkg.SCENE_S)
    vp = ctypes.c_void_p
    if driver == "lambert":
        st = med.L.lib.gpis_fs_render_scene_s(med.h, vp(sc.ctypes.data), vp(rad.data_ptr()), vp(cnt.data_ptr()), vp(stream_ptr()))
    else:
        st = med.L.lib.gpis_fs_render_scene_s_paths(med.h, vp(sc.ctypes.data), int(bounces), ctypes.c_float(fa.ALBEDO), vp(rad.data_ptr()), vp(cnt.data_ptr()),
                                                    vp(stream_ptr()))
    assert st == 0, med.L.last_error()
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w), cnt.cpu().numpy().view(np.uint32).reshape(h, w)


_COMPOSITES = {}


def _composite(pkg, ob, name):
    """the GPU-sampled composite of a case, computed once: the schedule over per-sample values of the uniform driver"""
    if name not in _COMPOSITES:
        driver, p, scene = fa.case_inputs(pkg, ob, name)
        med = pkg.Medium(p)
        _COMPOSITES[name] = fa.frame(lambda one: _uniform(pkg, med, driver, one), scene)
        med.close()
    return _COMPOSITES[name]


def _equal(got, want):
    for k in ("radiance_sum", "sample_count", "hit_count", "records", "info"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, a, b)


@pytest.mark.parametrize("name", sorted(dict(fa.CASES, **fa.CASES_64)))
def test_composite(env, name):
    """every context, the short last pass and the 64-point state, both drivers (fs_adaptive_ref.CASES, CASES_64; their schedules and
    their classes of segments are checked on the CPU composite by tests/test_fs_adaptive_cpu.py, the schedule here again)"""
    pkg, ob = env
    driver, p, scene = fa.case_inputs(pkg, ob, name)
    want = _composite(pkg, ob, name)
    print(name, want["info"], "k_used", want["k_used"], "largest value", want["largest_value"], "counts per pass", [(int(c.min()), int(c.max())) for c in want["counts"]])
    fa.check_case_schedule(name, want)
    assert want["largest_value"] <= 65536 and want["radiance_sum"].max() > 0 and want["hit_count"].max() > 0
    if int(scene["spp_count"]) == 40:
        assert int(want["info"]["samples"]) < W * H * 40
    if driver == "paths":
        assert (want["hit_count"] > want["sample_count"]).any()             # segments, not hits
    med = pkg.Medium(p)
    got = _adaptive(pkg, med, driver, scene)
    med.close()
    _equal(got, want)
    assert np.array_equal(want["counts"].sum(axis=0), got["records"]["sample_index"])


@pytest.mark.parametrize("name", sorted(fa.CLAMP_CASES))
def test_clamp(env, name):
    """some values exceed 65536 and count as 0 in the image and the statistics; a clamped path sample's segments still count (the
    composite's segment counts are the uniform driver's, which knows no clamp)"""
    pkg, ob = env
    driver, p, scene = fa.case_inputs(pkg, ob, name)
    want = _composite(pkg, ob, name)
    print(name, want["info"], "largest value", want["largest_value"], "image max", float(want["radiance_sum"].max()))
    assert want["largest_value"] > 65536 and want["radiance_sum"].max() > 0 and want["hit_count"].max() > 0
    med = pkg.Medium(p)
    _equal(_adaptive(pkg, med, driver, scene), want)
    med.close()


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_all_zero_samples_stop_after_the_first_pass(env, driver):
    """a light behind the object for the frame driver, one bounce (no next-event estimation) for the path driver, whose segment of
    the last bounce is marched and counted all the same"""
    pkg, ob = env
    med = pkg.Medium(fa.medium(pkg))
    scene = fa.scene(ob, **(fa.DARK if driver == "lambert" else {}))
    got = _adaptive(pkg, med, driver, scene, bounces=1)
    first = scene.copy()
    first["spp_count"] = 16
    want = _uniform(pkg, med, driver, first, bounces=1)
    med.close()
    assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == (1, 1, W * H * 16)
    assert (got["sample_count"] == 16).all() and (got["radiance_sum"] == 0).all() and (want[0] == 0).all()
    assert (got["records"]["sample_index"] == 16).all() and (got["records"]["running_variance"] == 0).all()
    assert got["hit_count"].max() > 0 and np.array_equal(got["hit_count"], want[1])


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_threshold_at_or_above_the_spp_is_uniform(env, driver):
    """A frame of one pass below the threshold is one uniform-driver call, bit for bit.  With several passes below the threshold the
    image is the sequence of the passes' calls accumulated into one buffer."""
    import torch
    pkg, ob = env
    med = pkg.Medium(fa.medium(pkg))
    for S, step in ((16, 16), (48, 48), (48, 16), (40, 16)):
        scene = fa.scene(ob, S)
        got = _adaptive(pkg, med, driver, scene, ar.default_adaptive(spp_step=step, threshold=max(S, 64)) if S > 16 else None)
        into = (torch.zeros(H * W, dtype=torch.float32, device="cuda"), torch.zeros(H * W, dtype=torch.int32, device="cuda"))
        for k0 in range(0, S, step):
            part = scene.copy()
            part["spp_begin"], part["spp_count"] = k0, min(step, S - k0)
            want = _uniform(pkg, med, driver, part, into)
        assert want[0].max() > 0 and want[1].max() > 0
        assert np.array_equal(got["radiance_sum"].view(np.uint32), want[0].view(np.uint32)) and (got["sample_count"] == S).all()
        assert np.array_equal(got["hit_count"], want[1])
        assert (got["records"]["sample_index"] == S).all()
        assert (int(got["info"]["passes_rendered"]), int(got["info"]["stopped_early"]), int(got["info"]["samples"])) == ((S + step - 1) // step, 0, W * H * S)
    med.close()


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_odd_spp_on_a_clipped_frame(env, driver):
    """9 x 6 from the default distance: 3 x 2 records, the last column and the last row of tiles clipped.  5 spp in steps of 2 under a
    threshold no pass reaches are passes of 2, 2 and 1 samples: every record plans a single sample at last, and the uniform driver
    runs odd counts beside it — per k for the composite, then the three passes' calls accumulated into one buffer."""
    import torch
    pkg, ob = env
    med = pkg.Medium(fa.medium(pkg))
    scene, settings = ob.default_scene_s(9, 6, 5), ar.default_adaptive(spp_step=2, threshold=64)
    want = fa.frame(lambda one: _uniform(pkg, med, driver, one), scene, settings)
    print(driver, want["info"], "largest value", want["largest_value"], "image max", float(want["radiance_sum"].max()))
    assert want["records"].shape == (2, 3) and [np.unique(c).tolist() for c in want["counts"]] == [[2], [2], [1]]
    assert 0 < want["largest_value"] <= 65536 and want["hit_count"].max() > 0
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
    """GPIS_OPT_CHUNK_LOG2 8: a full record of the first pass (16 pixels x 16 samples) is exactly one chunk and the clipped bottom-row
    records share chunks; later passes hold records above the chunk (16 pixels x more than 16 samples) and chunks of many count-1
    records.  Everything is what the one-chunk passes of the default give."""
    pkg, ob = env
    driver, p, scene = fa.case_inputs(pkg, ob, name)
    counts = _composite(pkg, ob, name)["counts"]
    assert counts[1:].max() * 16 > 256 and (counts[1:] == 1).sum() >= 2
    med = pkg.Medium(p)
    runs = {}
    for l in (0, 8, 10):
        med.set_option("chunk_log2", l)
        runs[l] = _adaptive(pkg, med, driver, scene)
    med.close()
    _equal(runs[0], _composite(pkg, ob, name))
    for l in (8, 10):
        _equal(runs[l], runs[0])


@pytest.mark.parametrize("driver", ["lambert", "paths"])
def test_accumulation(env, driver):
    """Two calls (spp_begin 0 and 64) into the same buffers.  Counts add exactly.  With one pass per call the image is the sum of the
    two single-call images bit for bit; with three passes per call the six pass sums are added one after the other, not pairwise:
    twelve float32 additions of non-negative terms separate the two orders, each off by at most 2^-24 of the final sum."""
    pkg, ob = env
    med = pkg.Medium(fa.medium(pkg))
    for S in (16, 48):
        a, b = fa.scene(ob, S), fa.scene(ob, S, spp_begin=64)
        ra, rb = _adaptive(pkg, med, driver, a), _adaptive(pkg, med, driver, b)
        assert not np.array_equal(ra["radiance_sum"], rb["radiance_sum"])
        into = Buffers()
        _adaptive(pkg, med, driver, a, into=into)
        both = _adaptive(pkg, med, driver, b, into=into)
        assert np.array_equal(both["sample_count"], ra["sample_count"] + rb["sample_count"])
        assert np.array_equal(both["hit_count"], ra["hit_count"] + rb["hit_count"]) and both["hit_count"].max() > 0
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


@pytest.mark.parametrize("name", ["lambert_renewal_plus", "paths_renewal_plus"])
def test_two_runs_are_byte_identical(env, name):
    """the order in which workgroups take samples from the work counter leaves no trace"""
    pkg, ob = env
    driver, p, scene = fa.case_inputs(pkg, ob, name)
    med = pkg.Medium(p)
    first, second = _adaptive(pkg, med, driver, scene), _adaptive(pkg, med, driver, scene)
    med.close()
    assert first["radiance_sum"].max() > 0
    _equal(second, first)


def test_fixture_bindings_and_the_uniform_entries_afterwards(env):
    """The recorded CPU composite; the bindings' return conventions; a NULL hit_count / seg_count; and, on the handle the adaptive
    entries have just used (shared workspace, state slots, record array and work counter), the uniform entries' own fixtures."""
    pkg, ob = env
    g = np.load(fa.GOLDEN)
    root = os.path.dirname(fa.GOLDEN)
    for tag, driver in (("lambert", "lambert"), ("paths", "paths")):
        p = np.array(g[tag + "_params"]).view(pkg.PARAMS).reshape(())
        scene = np.array(g[tag + "_scene"]).view(pkg.SCENE_S).reshape(())
        adaptive = np.array(g["adaptive"], dtype=pkg.ADAPTIVE_S)
        want = {k: g[tag + "_" + k] for k in ("radiance_sum", "sample_count", "hit_count", "records", "info")}
        bounces, albedo = int(g["max_bounces"]), float(g["albedo"])
        assert np.float32(fa.ALBEDO) == g["albedo"]
        med = pkg.Medium(p)
        got = _adaptive(pkg, med, driver, scene, adaptive, bounces=bounces)
        _equal(got, want)
        if driver == "lambert":
            rad, cnt, hits, rec, info = med.fs_render_scene_s_adaptive(scene, adaptive, want_hits=True, want_records=True)
            rad2, cnt2, info2 = med.fs_render_scene_s_adaptive(scene)
        else:
            rad, cnt, hits, rec, info = med.fs_render_scene_s_paths_adaptive(scene, bounces, albedo, adaptive, want_segs=True, want_records=True)
            rad2, cnt2, info2 = med.fs_render_scene_s_paths_adaptive(scene, bounces, albedo)
        _equal({"radiance_sum": rad, "sample_count": cnt, "hit_count": hits, "records": rec, "info": info}, got)
        assert np.array_equal(rad2, rad) and np.array_equal(cnt2, cnt) and info2 == info
        b = Buffers(fill=0)
        st, _ = _status(pkg, med, driver, scene, adaptive, b, bounces=bounces, no_count=True)
        out = b.host()
        assert st == 0 and np.array_equal(out["radiance_sum"], rad) and not out["hit_count"].any()
        med.close()
    # the uniform entries after the adaptive ones, on one handle: the path driver's recorded fixture (test_gpu_fs_paths.py), and
    # the frame driver against its own image from a handle no adaptive entry has touched
    gp = np.load(os.path.join(os.path.dirname(fa.GOLDEN), "fs_paths_small.npz"))
    p = np.array(gp["params"]).view(pkg.PARAMS).reshape(())
    scene = np.array(gp["scene"]).view(pkg.SCENE_S).reshape(())
    fresh = pkg.Medium(p)
    want_img, want_hits = fresh.fs_render_scene_s(scene, want_hits=True)
    fresh.close()
    med = pkg.Medium(p)
    for driver in ("paths", "lambert"):
        _adaptive(pkg, med, driver, fa.scene(ob, 32))
    img, segs = med.fs_render_scene_s_paths(scene, int(gp["max_bounces"]), float(gp["albedo"]), want_segs=True)
    assert gp["image"].any() and img.tobytes() == np.ascontiguousarray(gp["image"]).tobytes() and np.array_equal(segs, gp["segs"])
    _adaptive(pkg, med, "paths", fa.scene(ob, 32))
    img, hits = med.fs_render_scene_s(scene, want_hits=True)
    med.close()
    assert want_img.any() and img.tobytes() == want_img.tobytes() and np.array_equal(hits, want_hits)


def test_refusals(env):
    pkg, ob = env
    import ws_oracle
    fs = pkg.Medium(fa.medium(pkg))
    wp, ww = ws_oracle.ws_params(pkg, n_basis=8)
    ws = pkg.WeightSpaceMedium(wp, ww)
    matern = fa.medium(pkg)
    matern["kernel_type"], matern["matern_v"] = 1, 2.5                 # GPIS_KERNEL_MATERN: what fs_check rejects
    sc = pkg.Medium(matern)
    ok, good = fa.scene(ob, 16), ar.default_adaptive()
    cases = {
        "weight-space handle": (ws, ok, good, {}),
        "parameters outside the function-space scope": (sc, ok, good, {}),
        "no handle": (fs, ok, good, {"no_handle": True}),
        "rows": (fs, fa.scene(ob, 16, y_begin=1, y_count=H - 1), good, {}),
        "fewer rows": (fs, fa.scene(ob, 16, y_count=H - 2), good, {}),
        "shards": (fs, fa.scene(ob, 16, shard_count=2), good, {}),
        "spp_step 0": (fs, ok, ar.default_adaptive(spp_step=0), {}),
        "threshold 1": (fs, ok, ar.default_adaptive(threshold=1), {}),
        "no samples": (fs, fa.scene(ob, 0), good, {}),
        "no scene": (fs, ok, good, {"no_scene": True}),
        "no settings": (fs, ok, None, {}),
        "no image": (fs, ok, good, {"rad": False}),
        "no sample counts": (fs, ok, good, {"cnt": False}),
        "no bounces": (fs, ok, good, {"bounces": 0}),
        "negative bounces": (fs, ok, good, {"bounces": -2}),
        # a first pass of 2^24 + 1 samples per pixel: a full record would hold more than 2^28 samples
        "a record above 2^28 samples": (fs, fa.scene(ob, (1 << 24) + 1), ar.default_adaptive(spp_step=(1 << 24) + 1, threshold=1 << 30), {}),
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
    for driver in ("lambert", "paths"):                                 # the handle still renders
        assert _status(pkg, fs, driver, ok, good, Buffers())[0] == 0, driver
    fs.close()
    ws.close()
    sc.close()
