"""gpis_render_scene_s_paths_rgb_adaptive, checked without a GPU: the declared and exported interface; the Vec3f clamp and the
luminance of the library (gpis_adaptive_rgb_value_host) against the plain-C restatement (tests/native/adaptive_rgb_value.c) and
against numbers recorded from the reference's Vec.hpp / SampleRecord.hpp (tests/golden/adaptive_rgb_pins.npz); and the restated
frame (tests/adaptive_paths_rgb_ref.py) on the 22 x 14 frame with the CPU composite's per-sample values
(tests/golden/adaptive_paths_rgb_small.npz)."""
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_paths_rgb_ref as apr
import adaptive_ref as ar

pytestmark = pytest.mark.skipif(not apr.available(), reason="no C compiler for tests/native/adaptive_rgb_value.c")

NEW = ("gpis_render_scene_s_paths_rgb_adaptive", "gpis_adaptive_rgb_value_host")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _lib_value(lib, rgb, want_rgb=True, want_lum=True):
    v = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
    out, lum = np.full_like(v, 7.0), np.full(len(v), 7.0, dtype=np.float32)
    lib.lib.gpis_adaptive_rgb_value_host(len(v), v.ctypes.data, out.ctypes.data if want_rgb else None, lum.ctypes.data if want_lum else None)
    return out, lum


# ---- interface
def test_header_declares_both_entries(pkg):
    header = open(os.path.join(ar.ROOT, "include", "gpis.h")).read()
    for name in NEW:
        assert re.search(r"^(?:extern )?(?:int|void)\s+%s\s*\(" % name, header, flags=re.M), name
    assert re.search(r"^(?:extern )?int gpis_render_scene_s_paths_rgb_adaptive\(gpis_medium \*m, const gpis_scene_s \*s, const gpis_adaptive_s \*a,\s*"
                     r"int max_path_bounces, const float albedo\[3\],\s*float \*radiance_sum3, uint32_t \*sample_count, uint32_t \*seg_count,\s*"
                     r"gpis_adaptive_record \*records, gpis_adaptive_info \*info, void \*stream\);", header, flags=re.M)
    assert re.search(r"^(?:extern )?void gpis_adaptive_rgb_value_host\(size_t n, const float \*rgb_in, float \*rgb_out, float \*luminance\);", header, flags=re.M)


def test_library_exports_both_entries(pkg):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        assert name in pkg.GpisLib.SYMBOLS
    assert callable(getattr(pkg.Medium, "render_scene_s_paths_rgb_adaptive", None))


# ---- clamp and luminance
def _table():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    over = np.nextafter(np.float32(65536), np.float32(np.inf))
    rows = [(0.0, 0.0, 0.0), (0.25, 0.5, 0.75), (1.0, 1.0, 1.0), (3.0, 0.125, 1e-6), (1234.5, 0.001, 65535.0), (1e-30, 1e-38, 1e-45), (-0.5, 0.25, -0.125)]
    for bad in (nan, inf, -inf):
        for c in range(3):
            row = [0.5, 0.25, 0.125]
            row[c] = bad
            rows.append(tuple(row))
    rows += [(65536.0, 65536.0, 65536.0), (65536.0, 1.0, 2.0), (1.0, 65536.0, 2.0), (1.0, 2.0, 65536.0)]              # exactly the limit: kept
    rows += [(over, 1.0, 2.0), (1.0, over, 2.0), (1.0, 2.0, over), (over, over, over)]                                # one step above: zeroed
    rows += [(1e6, 0.01, 0.02), (0.01, 1e6, 0.02), (0.01, 0.02, 1e6)]                                                 # one channel over, two small
    rows += [(-1e9, 1.0, 2.0), (1.0, -1e9, 2.0), (1.0, 2.0, -1e9), (-1e9, -1e9, -1e9), (-3.0e38, 0.0, 0.0)]           # large negative: kept
    rng = np.random.default_rng(7)
    rows += [tuple(r) for r in (rng.random((200, 3)) * 10.0 ** rng.integers(-6, 6, (200, 1))).astype(np.float32)]
    return np.array(rows, dtype=np.float32)


def test_value_host_equals_the_restatement(lib):
    t = _table()
    want_rgb, want_lum, flag = apr.value(t)
    got_rgb, got_lum = _lib_value(lib, t)
    assert np.array_equal(_bits(got_rgb), _bits(want_rgb)) and np.array_equal(_bits(got_lum), _bits(want_lum))
    # what the table is there for
    bad = ~np.isfinite(t).all(axis=1) | (t > 65536).any(axis=1)
    assert np.array_equal(flag.astype(bool), bad) and 16 <= bad.sum() < len(t) - 200
    assert (got_rgb[bad] == 0).all() and (got_lum[bad] == 0).all()
    assert np.array_equal(_bits(got_rgb[~bad]), _bits(t[~bad]))
    kept = (t == 65536).any(axis=1)
    assert kept.sum() == 4 and not bad[kept].any() and got_lum[kept].min() > 0
    neg = (t <= -1e9).any(axis=1) & np.isfinite(t).all(axis=1)
    assert neg.sum() == 5 and not bad[neg].any() and (got_lum[neg] < -1e7).all()
    # either output may be left out
    only_lum = _lib_value(lib, t, want_rgb=False)
    only_rgb = _lib_value(lib, t, want_lum=False)
    assert (only_lum[0] == 7).all() and np.array_equal(_bits(only_lum[1]), _bits(want_lum))
    assert (only_rgb[1] == 7).all() and np.array_equal(_bits(only_rgb[0]), _bits(want_rgb))


@pytest.mark.parametrize("who", ["restatement", "library"])
def test_luminance_and_add_sample_reproduce_the_reference(pkg, lib, who):
    """Vec3f::luminance and SampleRecord::addSample(const Vec3f &) as the reference's own headers compute them"""
    pins = np.load(apr.PINS)
    off, rgb = pins["offsets"], pins["rgb"]
    assert len(off) - 1 >= 200 and len(rgb) == off[-1] and (np.isfinite(rgb) & (rgb <= 65536)).all()          # nothing for the clamp
    lum = apr.value(rgb)[1] if who == "restatement" else _lib_value(lib, rgb)[1]
    assert np.array_equal(_bits(lum), _bits(pins["luminance"]))
    for i in range(len(off) - 1):
        vals = np.ascontiguousarray(lum[off[i]:off[i + 1]])
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


# ---- the restated frame
@pytest.fixture(scope="module")
def small(pkg, ob):
    return apr.small_reference(pkg, ob)


def test_small_frame_schedule_is_a_real_one(pkg, ob, small):
    info, counts = small["info"], small["counts"]
    print("counts per pass", [(int(c.min()), int(c.max())) for c in counts], "k_used", small["k_used"], "clamped", int(small["clamped"].sum()))
    assert (int(info["passes_rendered"]), int(info["stopped_early"])) == (3, 0) and counts.shape == (3, 4, 6)
    assert apr.is_real_schedule(counts)
    assert np.array_equal(small["records"]["sample_index"], counts.sum(axis=0))
    assert int(info["samples"]) == int(small["sample_count"].sum())
    # the frame has emission in three different channels, background records, and nothing for the clamp
    img = small["radiance_sum"]
    assert img.min() >= 0 and img.max() > 0 and not np.array_equal(img[..., 0], img[..., 1]) and not np.array_equal(img[..., 1], img[..., 2])
    assert (small["records"]["mean"] == 0).any() and small["clamped"].sum() == 0 and small["seg_count"].max() > 0


def channel0(clamped_rgb):
    return np.ascontiguousarray(clamped_rgb[..., 0])


def test_the_luminance_drives_the_schedule_not_a_channel(pkg, ob, small):
    other = apr.small_reference(pkg, ob, drive=channel0)
    assert np.array_equal(other["counts"][0], small["counts"][0])
    assert not np.array_equal(other["counts"][1], small["counts"][1])
    assert other["records"]["mean"].tobytes() != small["records"]["mean"].tobytes()


def test_small_frame_equals_the_fixture(pkg, ob, small):
    g = np.load(apr.GOLDEN)
    params, albedo, scene, adaptive = apr.small_inputs(pkg, ob)
    assert np.array(g["params"], dtype=pkg.PARAMS) == np.array(params, dtype=pkg.PARAMS)
    assert np.array(g["scene"], dtype=pkg.SCENE_S) == np.array(scene, dtype=pkg.SCENE_S)
    assert np.array(g["adaptive"], dtype=ar.ADAPTIVE_S) == adaptive
    assert np.array_equal(g["albedo"], albedo) and int(g["max_bounces"]) == apr.SMALL_BOUNCES
    for k in apr.KEYS + ("counts",):
        assert g[k].shape == small[k].shape and g[k].tobytes() == np.ascontiguousarray(small[k]).tobytes(), k
    assert os.path.getsize(apr.GOLDEN) < 1 << 20
