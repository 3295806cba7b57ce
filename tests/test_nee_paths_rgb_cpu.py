"""The CPU composite of gpis_render_scene_s_nee_paths_rgb (tests/nee_paths_rgb_ref.py around tests/native/nee_paths_rgb_shade.c),
pinned without a GPU: to tests/nee_paths_ref.py's mono composite (itself pinned to oracle_render_scene_s_nee) wherever colour
cannot matter, and case by case where it does — the all-zero tests on f and on the throughput, the emission, the first-hit frame.
Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import nee_paths_ref as npr
import nee_paths_rgb_ref as rgb


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not rgb.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", rgb.GREY_CASES)
def test_equal_channels_equal_the_mono_composite(pkg, ob, name):
    mono = npr._surface(pkg, cap_cos=float(rgb.CASES[name](pkg)[1]["cap_cos"]))
    for max_bounces in rgb.BOUNCES:
        want = rgb.mono_reference(pkg, ob, name, max_bounces, mono)
        got = rgb.reference(pkg, ob, name, max_bounces, surface=rgb.grey_surface(pkg, mono))
        for c in range(3):
            assert np.array_equal(_bits(got.image[..., c]), _bits(want.image)), (name, max_bounces, c)
        assert np.array_equal(got.seg_count, want.seg_count)
        assert (got.marched, got.hits, got.light, got.phase) == (want.marched, want.hits, want.light, want.phase)
        assert want.image.any() == (max_bounces > 1)


@pytest.mark.parametrize("name", rgb.GREY_CASES)
def test_copper_channel_equals_the_mono_composite_of_its_surface(pkg, ob, name):
    _, surf = rgb.CASES[name](pkg)
    got = rgb.reference(pkg, ob, name, 4)
    for c in range(3):
        want = rgb.mono_reference(pkg, ob, name, 4, rgb.channel_surface(pkg, surf, c))
        assert want.image.any() and np.array_equal(_bits(got.image[..., c]), _bits(want.image)), (name, c)
        assert np.array_equal(got.seg_count, want.seg_count)
    assert not np.array_equal(got.image[..., 0], got.image[..., 1]) and not np.array_equal(got.image[..., 1], got.image[..., 2])


def test_fresnel_is_the_scalar_function_per_channel(pkg, ob):
    ref, mono = rgb.NeePathsRgbRef(pkg, ob), npr.shade_lib()
    f32 = ctypes.c_float
    surfaces = [rgb.copper(pkg), rgb.copper(pkg, albedo=(0.9, 0.5, 0.25)), rgb.copper(pkg, eta=(0.0, 1.5, 0.0), k=(0.0, 2.5, 3.0), albedo=(0.9, 1.0, 0.5))]
    for surf in surfaces:
        for cos_theta in (1.0, 0.75, 0.3, 1e-3, 0.0):
            got = ref.fresnel(surf, cos_theta)
            for c in range(3):
                want = np.float32(surf["albedo"][c]) * np.float32(mono.nee_paths_conductor_reflectance(f32(surf["eta"][c]), f32(surf["k"][c]), f32(cos_theta)))
                assert _bits(got[c:c + 1])[0] == _bits(np.array([want], dtype=np.float32))[0], (surf, cos_theta, c)
    assert ref.fresnel(surfaces[2], 0.3)[0] == np.float32(0.9)          # eta = k = 0: reflectance 1


def test_zero_channels(pkg, ob):
    """albedo 0 in every channel: f is all zero, no light shadow segment is marched and the path ends at its first hit.  albedo 0 in
    two channels: f and the throughput are zero there only — the light segments are marched and the paths live on, exactly those of
    the full surface, and the live channel equals the full surface's."""
    full = rgb.reference(pkg, ob, "nee", 4)
    black = rgb.reference(pkg, ob, "nee", 4, surface=rgb.copper(pkg, albedo=(0.0, 0.0, 0.0)))
    assert sum(full.light) > 0 and sum(black.light) == 0 and sum(black.phase) == 0 and not black.image.any()
    assert len(black.marched) == 1 and black.marched[0] == full.marched[0] and black.n_seg == black.marched[0]
    one = rgb.reference(pkg, ob, "nee", 4, surface=rgb.copper(pkg, albedo=(0.0, 1.0, 0.0)))
    assert (one.marched, one.hits, one.light, one.phase) == (full.marched, full.hits, full.light, full.phase)
    assert len(one.marched) == 3 and one.marched[2] > 0                # bounce 2 is reached on one live channel
    assert np.array_equal(one.seg_count, full.seg_count)
    assert not one.image[..., 0].any() and not one.image[..., 2].any()
    assert np.array_equal(_bits(one.image[..., 1]), _bits(full.image[..., 1]))
    # the same with the phase estimator in play
    one = rgb.reference(pkg, ob, "mis", 4, surface=rgb.copper(pkg, albedo=(0.0, 0.0, 1.0)))
    full = rgb.reference(pkg, ob, "mis", 4)
    assert np.array_equal(one.seg_count, full.seg_count) and np.array_equal(_bits(one.image[..., 2]), _bits(full.image[..., 2]))


def test_light_off_rule(pkg, ob):
    """cap_radiance zero in every channel: nothing is added, the segments are marched all the same; zero in two channels: the third is
    the full surface's"""
    full = rgb.reference(pkg, ob, "mis", 4)
    dark = rgb.reference(pkg, ob, "mis", 4, surface=rgb.copper(pkg, cap_radiance=(0.0, 0.0, 0.0)))
    assert not dark.image.any() and np.array_equal(dark.seg_count, full.seg_count)
    one = rgb.reference(pkg, ob, "mis", 4, surface=rgb.copper(pkg, cap_radiance=(0.0, 15.0, 0.0)))
    assert np.array_equal(one.seg_count, full.seg_count) and not one.image[..., 0].any() and not one.image[..., 2].any()
    assert np.array_equal(_bits(one.image[..., 1]), _bits(full.image[..., 1]))


def test_emissive_medium(pkg, ob):
    """max_path_bounces = 1: first-hit emission only — one segment per sample that meets the bound, no shadow segment; without the
    emission zeros and nothing marched.  At 4 bounces the emission adds to every channel and a fourth segment is marched."""
    name = rgb.EMISSIVE_CASE
    first = rgb.reference(pkg, ob, name, 1)
    assert first.image.any() and first.marched == [first.n_samples - first.n_miss] and first.n_seg == first.marched[0]
    assert first.hits == [0] and not first.light and not first.phase
    none = rgb.reference(pkg, ob, name, 1, emission=False)
    assert not none.image.any() and not none.seg_count.any() and not none.marched
    with_e, without = rgb.reference(pkg, ob, name, 4), rgb.reference(pkg, ob, name, 4, emission=False)
    assert len(with_e.marched) == 4 and with_e.marched[3] > 0 and len(without.marched) == 3
    assert with_e.marched[:3] == without.marched and (with_e.light, with_e.phase) == (without.light, without.phase)
    assert (with_e.image >= without.image).all() and (with_e.image[first.image > 0] > without.image[first.image > 0]).all()
    # the three weights differ, so no channel is a mono composite of another: the channels differ beyond the surface's colour
    grey = rgb.reference(pkg, ob, name, 4, surface=rgb.grey_surface(pkg, npr._surface(pkg)), emission=False)
    assert not np.array_equal(grey.image[..., 0], grey.image[..., 1]) and not np.array_equal(grey.image[..., 1], grey.image[..., 2])
    # channel 0 carries weight[0], as the mono composite does
    want = rgb.mono_reference(pkg, ob, name, 4, npr._surface(pkg))
    assert np.array_equal(_bits(grey.image[..., 0]), _bits(want.image)) and np.array_equal(grey.seg_count, want.seg_count)


@pytest.mark.parametrize("name", sorted(rgb.CASES))
def test_cases_are_not_vacuous(pkg, ob, name):
    c = rgb.reference(pkg, ob, name, 4)
    print(name, "marched", c.marched, "hits", c.hits, "exits", c.exits, "light", c.light, "visible", c.light_visible, "phase", c.phase)
    assert sum(c.exits) > 0 and c.hits[0] > 0
    assert len(c.marched) >= 3 and c.marched[2] > 0                    # a path alive at bounce 2
    if name != "uni":
        assert sum(c.light_visible) > 0 and sum(c.light) > sum(c.light_visible)
    else:
        assert not sum(c.light)
    if name != "nee":
        assert sum(c.phase) > 0
    else:
        assert not sum(c.phase)
    assert c.image.any() and 0 <= c.n_miss < c.n_samples


def test_fixture_is_current(pkg, ob):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_nee_paths_rgb_golden", os.path.join(os.path.dirname(rgb.GOLDEN), "make_nee_paths_rgb_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want, got = mod.arrays(pkg, ob), np.load(rgb.GOLDEN)
    assert sorted(want) == sorted(got.files)
    for key in want:
        assert np.asarray(want[key]).tobytes() == np.asarray(got[key]).tobytes(), key
    assert os.path.getsize(rgb.GOLDEN) < 1 << 20
