"""The CPU reference of gpis_render_scene_s_paths_rgb (tests/paths_rgb_ref.py over tests/native/paths_rgb_shade.c), checked on the
CPU alone: the declared interface; without emission every channel pinned to the oracle's multi-bounce estimator; the emission
terms accounted for sample by sample from the composite's own records; the inputs shown to exercise every branch (hits at the
last traced bounce, the extra last segment of an emissive medium, three different channels); the composite shown independent of
how a frame is cut into calls; and the record in tests/golden/paths_rgb_small.npz."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import paths_rgb_ref as prr

pytestmark = pytest.mark.skipif(not prr.available(), reason="no C compiler for tests/native/paths_rgb_shade.c")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_entry_is_declared_and_exported(pkg):
    header = open(os.path.join(prr.ROOT, "include", "gpis.h")).read()
    assert re.search(r"^int\s+gpis_render_scene_s_paths_rgb\s*\(gpis_medium \*m, const gpis_scene_s \*s, int max_path_bounces, const float albedo\[3\],\s*"
                     r"float \*radiance_sum3, uint32_t \*seg_count, void \*stream\);", header, flags=re.M)
    assert re.search(r"^#define GPIS_ABI_VERSION 3$", header, flags=re.M)
    assert callable(getattr(pkg.Medium, "render_scene_s_paths_rgb", None))
    assert "gpis_render_scene_s_paths_rgb" in pkg.GpisLib.SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_render_scene_s_paths_rgb$", out, flags=re.M)


@pytest.mark.parametrize("name", prr.PIN_CASES)
def test_without_emission_every_channel_is_the_oracles_estimator(pkg, ob, name):
    """Channel 0 is oracle_render_scene_s_paths(albedo[0]) bit for bit; channels 1 and 2 are the oracle's image of the same medium
    with sigma_a, sigma_s and albedo rolled so that the channel sits first (the ramp colours have three equal components)."""
    params, albedo, _ = prr.CASES[name](pkg)
    params = prr.without_emission(params)
    scene = prr.frame(ob)
    for max_bounces in prr.BOUNCES:
        got = prr.reference(pkg, ob, name, max_bounces, emission=False)
        for c in range(3):
            p = np.array(params).copy()
            p["sigma_a"], p["sigma_s"] = np.roll(params["sigma_a"], -c), np.roll(params["sigma_s"], -c)
            want = ob.Oracle(p, threads=16).render_scene_s_paths(scene, max_bounces, float(np.float32(albedo[c])))
            assert want.any() == (max_bounces > 1)
            assert np.array_equal(_bits(got.image[:, :, c]), _bits(want)), (max_bounces, c, int((got.image[:, :, c] != want).sum()))
    if name == "sigma":
        img = prr.reference(pkg, ob, name, 4, emission=False).image
        assert not np.array_equal(img[:, :, 0], img[:, :, 1]) and not np.array_equal(img[:, :, 1], img[:, :, 2])


def _resum(c, with_emission):
    """every sample's emission recomputed in numpy float32 from the records of the composite's bounce levels, in the stated order:
    per bounce the hit's emission term thr_before * e (the product rounded on its own), then the NEE term"""
    em = np.zeros_like(c.sample_em)
    for lv in c.levels:
        if with_emission:
            hit = lv.hit.astype(bool)
            prod = (lv.thr_before * lv.e).astype(np.float32)
            em[hit] = em[hit] + prod[hit]
        nee = lv.nee.astype(bool)
        add = np.where(lv.vis.astype(bool)[:, None], lv.contrib, np.float32(0))
        em[nee] = em[nee] + add[nee]
    assert em.dtype == np.float32
    return em


def _pixel_sums(c, em, shape):
    img = np.zeros(shape, dtype=np.float32).reshape(-1, 3)
    i = 0
    while i < len(em):
        acc = np.zeros(3, dtype=np.float32)
        j = i
        while j < len(em) and c.pix[j] == c.pix[i]:
            acc = acc + em[j]
            j += 1
        img[c.pix[i]] = img[c.pix[i]] + acc
        i = j
    return img.reshape(shape)


@pytest.mark.parametrize("name", prr.EMISSIVE_CASES)
def test_emission_terms_are_accounted_for(pkg, ob, name):
    for B in prr.BOUNCES:
        on, off = prr.reference(pkg, ob, name, B), prr.reference(pkg, ob, name, B, emission=False)
        # the same paths: the emission changes no draw, no weight and no branch, it only marches one more segment
        assert on.marched[:B - 1] == off.marched and on.hits[:B - 1] == off.hits and on.shadow[:B - 1] == off.shadow
        assert len(on.marched) == B and on.marched[B - 1] > 0 and on.hits[B - 1] > 0, (on.marched, on.hits)
        assert len(on.shadow) == B and on.shadow[B - 1] == 0
        for a, b in zip(on.levels, off.levels):
            assert np.array_equal(_bits(a.contrib), _bits(b.contrib)) and np.array_equal(a.nee, b.nee) and np.array_equal(a.vis, b.vis)
            assert not b.thr_before.any() and not b.e.any()
        # with the emission terms: the emissive composite's sums; without them: the sums of the composite with emission off
        assert np.array_equal(_bits(_resum(on, True)), _bits(on.sample_em))
        assert np.array_equal(_bits(_resum(on, False)), _bits(off.sample_em))
        assert np.array_equal(_bits(_pixel_sums(on, on.sample_em, on.image.shape)), _bits(on.image))
        for lv in on.levels:
            hit = lv.hit.astype(bool)
            assert (lv.thr_before[hit] > 0).all() and (lv.e[hit] > 0).all() and not lv.thr_before[~hit].any()
        assert (on.image >= off.image).all() and (on.image > off.image).any()
        # the segments of the last bounce appear in the counts, pixel by pixel
        last = np.zeros(on.seg_count.size, dtype=np.uint32)
        np.add.at(last, on.pix, on.levels[B - 1].marched.astype(np.uint32))
        assert np.array_equal(on.seg_count, off.seg_count + last.reshape(on.seg_count.shape))
        assert on.n_seg == off.n_seg + on.marched[B - 1]


def test_one_bounce(pkg, ob):
    """with emission max_path_bounces = 1 renders first-hit emission; without, it adds zeros and marches nothing"""
    for name in prr.EMISSIVE_CASES:
        c = prr.reference(pkg, ob, name, 1)
        assert all((c.image[:, :, k] > 0).any() for k in range(3)) and c.marched == [prr.W * prr.H * prr.SPP - c.n_miss] and c.shadow == [0]
        assert c.n_seg == c.marched[0]
    for name in prr.CASES:
        c = prr.reference(pkg, ob, name, 1, emission=False)
        assert not c.image.any() and not c.seg_count.any() and c.marched == []


@pytest.mark.parametrize("name", sorted(prr.CASES))
def test_cases_exercise_every_branch(pkg, ob, name):
    """hits at the last traced bounce, shadow segments at every bounce that has next-event estimation, every channel non-zero"""
    params, albedo, _ = prr.CASES[name](pkg)
    E = prr.emissive(params)
    assert E == (name in prr.EMISSIVE_CASES)
    for B in prr.BOUNCES:
        c = prr.reference(pkg, ob, name, B)
        traced = B if E else B - 1
        assert len(c.marched) == traced and len(c.hits) == traced
        if traced:
            assert c.hits[-1] > 0 and all(s > 0 for s in c.shadow[:B - 1]), (c.hits, c.shadow)
            assert all(c.image[:, :, k].any() for k in range(3))
            assert c.n_seg == sum(c.marched) + sum(c.shadow)
        assert np.isfinite(c.image).all()
    c4, c2 = prr.reference(pkg, ob, name, 4), prr.reference(pkg, ob, name, 2)
    assert not np.array_equal(c4.image, c2.image) and c4.n_seg > c2.n_seg
    if name == "grey":
        assert np.array_equal(c4.image[:, :, 0], c4.image[:, :, 1]) and np.array_equal(c4.image[:, :, 0], c4.image[:, :, 2])
    if name == "rust":
        # three different colour and emission components
        assert not np.array_equal(c4.image[:, :, 0], c4.image[:, :, 1]) and not np.array_equal(c4.image[:, :, 1], c4.image[:, :, 2])
        e = np.concatenate([lv.e[lv.hit.astype(bool)] for lv in c4.levels])
        assert (e[:, 0] != e[:, 1]).any() and (e[:, 1] != e[:, 2]).any() and np.isfinite(e).all()
        one = prr.reference(pkg, ob, name, 1).image
        assert not np.array_equal(one[:, :, 0], one[:, :, 2])


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_composite_does_not_depend_on_the_cutting(pkg, ob, kind):
    """Rows and shards partition the pixels, so the parts add up to the whole frame's image bit for bit.  The spp ranges {0} and
    {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2: there the counts are compared exactly, the image to rounding,
    and three calls of one sample each, which add in the frame's own order, exactly."""
    name = "ramp"
    params, albedo, _ = prr.CASES[name](pkg)
    whole = prr.reference(pkg, ob, name, 4)
    ref, orc = prr.PathsRgbRef(pkg, ob), ob.Oracle(params, threads=16)
    acc, singles = None, []
    for s in prr.parts(ob, kind):
        acc = ref.compose(orc, s, 4, albedo, into=acc)
        singles.append(ref.compose(orc, s, 4, albedo))
    assert np.array_equal(acc.seg_count, whole.seg_count)
    assert acc.marched == whole.marched and acc.hits == whole.hits and acc.shadow == whole.shadow
    if kind != "spp":
        assert np.array_equal(_bits(acc.image), _bits(whole.image))
    else:
        assert np.array_equal(_bits(acc.image), _bits(singles[0].image + singles[1].image))
        assert np.allclose(acc.image, whole.image, rtol=1e-6, atol=0)
        one = None
        for k in range(prr.SPP):
            s = prr.frame(ob)
            s["spp_begin"], s["spp_count"] = k, 1
            one = ref.compose(orc, s, 4, albedo, into=one)
        assert np.array_equal(_bits(one.image), _bits(whole.image)) and np.array_equal(one.seg_count, whole.seg_count)


def test_golden_fixture_regenerates(pkg, ob):
    """tests/golden/paths_rgb_small.npz is what tests/golden/make_paths_rgb_golden.py writes today."""
    sys.path.insert(0, os.path.join(prr.ROOT, "tests", "golden"))
    import make_paths_rgb_golden as mk
    have = np.load(prr.GOLDEN)
    want = mk.arrays(pkg, ob)
    assert sorted(have.files) == sorted(want)

    def same(a, b):          # field by field: the padding bytes of a record are not data
        if b.dtype.names:
            return a.dtype.names == b.dtype.names and a.dtype.itemsize == b.dtype.itemsize and all(same(a[f], b[f]) for f in b.dtype.names)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for k in want:
        assert same(have[k], want[k]), k
    assert os.path.getsize(prr.GOLDEN) < 100 * 1024
