"""The adaptive sample schedule of gpis_render_scene_s_adaptive, checked without a GPU: the declared interface; the statistics of
the restatement (tests/native/adaptive_ref.c) and of the library pinned to numbers recorded from the reference's SampleRecord.hpp
(tests/golden/adaptive_ref_pins.npz); the library's host plan step against the restatement, bit for bit, with the properties of a
plan; and the restated pass loop on a small frame with the CPU oracle's sample values (tests/golden/adaptive_small.npz).  The four
control functions of the reference's integrator are private members that need a scene: their restatement is not pinned to a
reference binary."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar

pytestmark = pytest.mark.skipif(not ar.available(), reason="no C compiler for tests/native/adaptive_ref.c")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_records(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.dtype.itemsize == b.dtype.itemsize and a.dtype.names == b.dtype.names and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _lib_plan(pkg, lib, adaptive, width, height, cur, n, state, records):
    rec = np.ascontiguousarray(records, dtype=pkg.ADAPTIVE_RECORD).copy().reshape(-1)
    st = ctypes.c_uint64(state)
    a = np.array(adaptive, dtype=pkg.ADAPTIVE_S)
    rc = lib.lib.gpis_adaptive_plan_host(a.ctypes.data, width, height, cur, n, ctypes.byref(st), rec.size, rec.ctypes.data)
    return rc, st.value, rec


# ---- sizes and exports
def test_sizes_defaults_and_exports(pkg, lib):
    assert (pkg.ADAPTIVE_S.itemsize, pkg.ADAPTIVE_RECORD.itemsize, pkg.ADAPTIVE_INFO.itemsize) == (16, 24, 16)
    assert (ar.ADAPTIVE_S, ar.RECORD, ar.INFO) == (pkg.ADAPTIVE_S, pkg.ADAPTIVE_RECORD, pkg.ADAPTIVE_INFO)
    got = dict(kv.split("=") for kv in lib.lib.gpis_abi_sizes().decode().split(","))
    assert (int(got["gpis_adaptive_s"]), int(got["gpis_adaptive_record"]), int(got["gpis_adaptive_info"])) == (16, 24, 16)
    a = np.frombuffer(b"\xff" * 16, dtype=pkg.ADAPTIVE_S).copy().reshape(())
    lib.lib.gpis_default_adaptive_s(a.ctypes.data)
    assert (int(a["spp_step"]), int(a["threshold"]), int(a["seed"]), int(a["_pad"])) == (16, 16, 0xBA5EBA11, 0)
    assert a == pkg.default_adaptive_s() and a == ar.default_adaptive()
    header = open(os.path.join(ar.ROOT, "include", "gpis.h")).read()
    assert re.search(r"^#define GPIS_ABI_VERSION 3$", header, flags=re.M)
    declared = set(re.findall(r"^(?:int|void|uint64_t)\s+(gpis_[a-z0-9_]*adaptive[a-z0-9_]*)\s*\(", header, flags=re.M))
    assert declared == {"gpis_default_adaptive_s", "gpis_render_scene_s_adaptive", "gpis_adaptive_plan_host", "gpis_adaptive_rng_init_host",
                        "gpis_adaptive_record_add_host"}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for name in declared:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert name in pkg.GpisLib.SYMBOLS
    assert callable(getattr(pkg.Medium, "render_scene_s_adaptive", None))


# ---- the statistics, pinned to the reference's header
@pytest.fixture(scope="module")
def pins():
    return np.load(ar.PINS)


def test_pins_cover_the_named_sequences(pins):
    off, v = pins["offsets"], pins["values"]
    seqs = [v[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    assert len(seqs) >= 300
    assert any(len(s) > 1 and np.all(s == s[0]) and s[0] != 0 for s in seqs)                              # constant
    assert any(len(s) > 2 and (s != 0).sum() == 1 for s in seqs)                                           # a single spike
    small = [i for i, s in enumerate(seqs) if len(s) > 1 and pins["mean"][i] ** 2 < 1e-3 and pins["error_estimate"][i] > 0]
    assert len(small) >= 50                                                                                # mean^2 under the 1e-3 floor
    assert np.isnan(pins["error_estimate"]).sum() == 2                                                     # no sample, one sample


@pytest.mark.parametrize("who", ["restatement", "library"])
def test_statistics_reproduce_the_reference(pkg, lib, pins, who):
    off, v = pins["offsets"], pins["values"]
    for i in range(len(off) - 1):
        vals = np.ascontiguousarray(v[off[i]:off[i + 1]])
        if who == "restatement":
            rec, var, err = ar.add_samples(vals)
        else:
            rec, out2 = np.zeros((), dtype=pkg.ADAPTIVE_RECORD), np.zeros(2, dtype=np.float32)
            lib.lib.gpis_adaptive_record_add_host(rec.ctypes.data, vals.size, vals.ctypes.data, out2.ctypes.data)
            var, err = out2
        assert int(rec["sample_count"]) == int(pins["sample_count"][i]) == vals.size
        got = np.array([rec["mean"], rec["running_variance"], var, err], dtype=np.float32)
        want = np.array([pins[k][i] for k in ("mean", "running_variance", "variance", "error_estimate")], dtype=np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (i, got, want)


def test_statistics_continue_from_a_record(pkg, lib, pins):
    """a record carried from pass to pass: adding in two parts is adding at once"""
    vals = np.ascontiguousarray(pins["values"][pins["offsets"][100]:pins["offsets"][101]])
    assert vals.size > 8
    whole = ar.add_samples(vals)[0]
    first = ar.add_samples(vals[:5])[0]
    assert _same_records(ar.add_samples(vals[5:], first)[0], whole)
    rec = np.array(first, dtype=pkg.ADAPTIVE_RECORD)
    lib.lib.gpis_adaptive_record_add_host(rec.ctypes.data, vals.size - 5, vals[5:].ctypes.data, None)
    assert _same_records(rec, whole)


# ---- the plan step
def _random_records(rng, gw, gh, kind):
    """records as a pass leaves them: sample_count samples each, a mean and a running variance"""
    n = gw * gh
    rec = np.zeros(n, dtype=ar.RECORD)
    rec["sample_count"] = rng.integers(16, 200, n)
    rec["next_sample_count"] = rng.integers(1, 40, n)
    rec["sample_index"] = rng.integers(16, 400, n)
    rec["adaptive_weight"] = rng.random(n)
    rec["mean"] = (rng.random(n) * np.where(rng.random(n) < 0.3, 0.02, 1.0)).astype(np.float32)
    rv = (rng.random(n) * rec["sample_count"] * 0.1).astype(np.float32)
    if kind == "zero":
        rv[:] = 0
    elif kind == "one":
        rv[:] = 0
        rv[int(rng.integers(0, n))] = 3.5
    elif kind == "equal":
        rec["sample_count"], rec["mean"], rv[:] = 32, 0.5, 2.0
    else:
        rv[rng.random(n) < 0.3] = 0
    rec["running_variance"] = rv
    return rec


# records wide x high -> an image size with clipped tiles; the last is the record grid of 1920 x 1080 (+ clipped edges)
GRIDS = {(1, 1): (3, 2), (5, 3): (18, 12), (6, 4): (22, 14), (481, 271): (1921, 1081)}


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("kind", ["random", "zero", "one", "equal"])
def test_plan_step_equals_the_restatement(pkg, lib, grid, kind):
    gw, gh = grid
    width, height = GRIDS[grid]
    assert ((width + 3) // 4, (height + 3) // 4) == grid
    rng = np.random.default_rng(1000 * gw + gh + len(kind))
    a = ar.default_adaptive()
    state = ar.rng_init(a, width, height)
    for cur, n in ((16, 16), (32, 8), (0, 16), (8, 8)):       # adaptive, a short last pass, and two passes below the threshold
        rec = _random_records(rng, gw, gh, kind)
        want = ar.plan(a, width, height, cur, n, state, rec)
        got = _lib_plan(pkg, lib, a, width, height, cur, n, state, rec)
        assert got[0] == want[0] and got[1] == want[1]
        assert _same_records(got[2], want[2])
        adaptive = cur >= 16
        assert want[0] == (0 if adaptive and kind == "zero" else 1)
        assert np.array_equal(want[2]["sample_index"], rec["sample_index"] + rec["next_sample_count"])
        if want[0] == 0:
            assert want[1] == state and np.array_equal(want[2]["next_sample_count"], rec["next_sample_count"])
            continue
        if not adaptive:
            assert want[1] == state and np.all(want[2]["next_sample_count"] == n)
            assert np.array_equal(_bits(want[2]["adaptive_weight"]), _bits(rec["adaptive_weight"]))
            continue
        assert want[1] != state
        cnt = want[2]["next_sample_count"].astype(np.int64)
        assert cnt.min() >= 1
        # the carry hands out the fractional parts one sample at a time: the sum is within 1 of the fractional total
        w = want[2]["adaptive_weight"]
        budget = np.int64((n - 1) * width * height).astype(np.int32).astype(np.uint32) // 16
        factor = np.float32(np.float64(budget) / np.sum(w.astype(np.float64)))
        frac = (w * factor).astype(np.float32)
        assert abs(int((cnt - 1).sum()) - float(np.sum(frac.astype(np.float64)))) <= 1.0 + 1e-6 * float(frac.sum())
        if kind == "equal":
            assert cnt.max() - cnt.min() <= 1
        state = want[1]


def test_plan_refuses(pkg, lib):
    a = ar.default_adaptive()
    rec = np.zeros(24, dtype=ar.RECORD)
    assert _lib_plan(pkg, lib, a, 22, 14, 0, 16, 1, rec)[0] == 1
    assert _lib_plan(pkg, lib, a, 22, 14, 0, 16, 1, rec[:23])[0] == -1           # not ceil(W/4) * ceil(H/4) records
    assert _lib_plan(pkg, lib, a, 22, 14, 0, 0, 1, rec)[0] == -1                 # an empty pass
    a["threshold"] = 1
    assert _lib_plan(pkg, lib, a, 22, 14, 0, 16, 1, rec)[0] == -1


def test_one_hot_record_raises_the_neighbours_the_two_sweeps_reach(pkg, lib):
    """The forward sweep reads the records below and to the right before they are rewritten, the backward sweep the forward results
    above and to the left: a hot record at (x, y) reaches its four neighbours and the two diagonal ones (x+1, y-1), (x-1, y+1)."""
    gw, gh, width, height = 6, 4, 22, 14
    a = ar.default_adaptive()
    for hx, hy in ((2, 1), (0, 0), (5, 3), (3, 2)):
        rec = np.zeros(gw * gh, dtype=ar.RECORD)
        rec["sample_count"], rec["mean"] = 16, 0.5
        rec["running_variance"][hx + hy * gw] = 1.0
        rc, _, out = ar.plan(a, width, height, 16, 16, ar.rng_init(a, width, height), rec)
        assert rc == 1 and _same_records(out, _lib_plan(pkg, lib, a, width, height, 16, 16, ar.rng_init(a, width, height), rec)[2])
        raised = {(i % gw, i // gw) for i in np.flatnonzero(out["adaptive_weight"] > 0)}
        reach = {(hx, hy), (hx - 1, hy), (hx + 1, hy), (hx, hy - 1), (hx, hy + 1), (hx + 1, hy - 1), (hx - 1, hy + 1)}
        assert raised == {(x, y) for x, y in reach if 0 <= x < gw and 0 <= y < gh}
        assert len(set(out["adaptive_weight"][out["adaptive_weight"] > 0].tolist())) == 1
        cnt = out["next_sample_count"].reshape(gh, gw)
        # a record without weight gets its one sample, and one more where the carry of the fractional parts happens to fire on it
        assert all(cnt[y, x] > 2 for x, y in raised)
        assert all(cnt[y, x] in (1, 2) for y in range(gh) for x in range(gw) if (x, y) not in raised)


def test_sampler_seed_and_the_draws_of_dice_tiles(pkg, lib):
    a = ar.default_adaptive()
    def both(adaptive, w, h):
        want = ar.rng_init(adaptive, w, h)
        assert lib.lib.gpis_adaptive_rng_init_host(np.array(adaptive, dtype=pkg.ADAPTIVE_S).ctypes.data, w, h) == want
        return want
    # UniformSampler(hash32(seed)): the state after the constructor's next2D is a^2 s + (a + 1), then one LCG step per 16 x 16 tile
    mult, mask = 6364136223846793005, (1 << 64) - 1
    x = 0xBA5EBA11
    for f in (lambda x: (~x + (x << 15)), lambda x: x ^ (x >> 12), lambda x: x + (x << 2), lambda x: x ^ (x >> 4), lambda x: x * 2057, lambda x: x ^ (x >> 16)):
        x = f(x) & 0xFFFFFFFF
    state = (x * mult * mult + mult + 1) & mask
    for tiles, (w, h) in ((1, (16, 16)), (2, (17, 16)), (4, (17, 17)), (2 * 1, (22, 14)), (120 * 68, (1920, 1080))):
        s = state
        for _ in range(tiles):
            s = (s * mult + 1) & mask
        assert both(a, w, h) == s, (w, h)
    assert both(a, 16, 16) != both(a, 17, 16) != both(a, 17, 17)          # another ceil(W/16) * ceil(H/16): another stream
    b = ar.default_adaptive(seed=1)
    assert both(b, 16, 16) != both(a, 16, 16)
    # and the stream reaches the plan: the same records, another tile count, other counts
    rng = np.random.default_rng(5)
    rec = _random_records(rng, 6, 4, "random")
    p1 = ar.plan(a, 22, 14, 16, 16, both(a, 22, 14), rec)
    p2 = ar.plan(a, 22, 14, 16, 16, both(a, 16, 16), rec)
    assert p1[1] != p2[1] and not np.array_equal(p1[2]["next_sample_count"], p2[2]["next_sample_count"])


# ---- the whole frame
@pytest.fixture(scope="module")
def small(pkg, ob):
    return ar.small_reference(pkg, ob)


def test_small_frame_schedule_is_not_vacuous(pkg, ob, small):
    info, counts = small["info"], small["counts"]
    assert (int(info["passes_rendered"]), int(info["stopped_early"])) == (3, 0) and counts.shape == (3, 4, 6)
    assert np.all(counts[0] == 16)
    for c in counts[1:]:
        assert (c == 1).any() and (c > 16).any()
    assert not np.array_equal(counts[1], counts[2])
    assert np.array_equal(small["records"]["sample_index"], counts.sum(axis=0))
    per_pixel = np.repeat(np.repeat(small["records"]["sample_index"], 4, axis=0), 4, axis=1)[:ar.SMALL_H, :ar.SMALL_W]
    assert np.array_equal(small["sample_count"], per_pixel)
    assert int(info["samples"]) == int(small["sample_count"].sum())
    assert np.array_equal(small["records"]["sample_count"], _tile_sum(small["sample_count"]))
    # the frame has background (records that never see a hit) and a lit surface
    assert (_tile_sum(small["hit_count"]) == 0).any() and small["radiance_sum"].max() > 0


def _tile_sum(img):
    h, w = img.shape
    pad = np.zeros(((h + 3) // 4 * 4, (w + 3) // 4 * 4), dtype=np.uint64)
    pad[:h, :w] = img
    return pad.reshape(pad.shape[0] // 4, 4, pad.shape[1] // 4, 4).sum(axis=(1, 3))


def test_small_frame_image_is_the_sum_of_uniform_ranges(pkg, ob, small):
    """Per pixel the frame is a concatenation of spp ranges: the oracle's own image of each pass's range, added pass by pass."""
    orc = ob.Oracle(pkg.params_for_config("C0"), threads=ar.THREADS)
    scene = ar.small_scene(ob)
    want = np.zeros((ar.SMALL_H, ar.SMALL_W), dtype=np.float32)
    hits = np.zeros((ar.SMALL_H, ar.SMALL_W), dtype=np.uint32)
    begin = np.zeros((4, 6), dtype=np.uint32)
    for counts in small["counts"]:
        for b, c in sorted({(int(b), int(c)) for b, c in zip(begin.reshape(-1), counts.reshape(-1))}):
            part = np.array(scene).copy()
            part["spp_begin"], part["spp_count"] = b, c
            img, h = orc.render_scene_s(part, want_hits=True)
            sel = np.repeat(np.repeat((begin == b) & (counts == c), 4, axis=0), 4, axis=1)[:ar.SMALL_H, :ar.SMALL_W]
            want[sel] += img[sel]
            hits[sel] += h[sel]
        begin += counts
    assert np.array_equal(_bits(small["radiance_sum"]), _bits(want))
    assert np.array_equal(small["hit_count"], hits)


def test_small_frame_equals_the_fixture(pkg, ob, small):
    g = np.load(ar.GOLDEN)
    assert np.array(g["params"], dtype=pkg.PARAMS) == np.array(pkg.params_for_config("C0"), dtype=pkg.PARAMS)      # field by field
    assert np.array(g["scene"], dtype=pkg.SCENE_S) == np.array(ar.small_scene(ob), dtype=pkg.SCENE_S)
    assert np.array(g["adaptive"], dtype=ar.ADAPTIVE_S) == ar.default_adaptive()
    for k in ("radiance_sum", "sample_count", "hit_count", "records", "info", "counts"):
        assert g[k].shape == small[k].shape and g[k].tobytes() == np.ascontiguousarray(small[k]).tobytes(), k


def test_restated_loop_clamps_and_stops(pkg, ob):
    """renderTile's clamp (values above 65536, infinities and NaN count as 0) and the early stop on a frame without error"""
    def const(value):
        def values(k0, k1):
            v = np.full((8, 8, k1 - k0), value, dtype=np.float32)
            v[:, :4] = 0.25
            return v, np.ones(v.shape, dtype=np.uint8)
        return values
    for bad in (np.inf, -np.inf, np.nan, 65537.0):
        r = ar.frame(ar.default_adaptive(), 8, 8, 48, const(bad))
        assert (int(r["info"]["passes_rendered"]), int(r["info"]["stopped_early"])) == (1, 1)
        assert np.all(r["radiance_sum"][:, 4:] == 0) and np.all(r["radiance_sum"][:, :4] == 4.0) and np.all(r["sample_count"] == 16)
        assert np.all(r["records"]["sample_index"] == 16) and np.all(r["hit_count"] == 16)
    r = ar.frame(ar.default_adaptive(), 8, 8, 48, const(65536.0))
    assert np.all(r["radiance_sum"][:, 4:] == 16 * 65536.0)
