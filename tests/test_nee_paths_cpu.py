"""The CPU reference of gpis_render_scene_s_nee_paths (tests/nee_paths_ref.py over tests/native/nee_paths_shade.c), checked on the
CPU alone: pinned to the oracle's single-interaction estimator and to the oracle's helpers, shown to hold real bounces, shown
independent of how a frame is cut into calls, and recorded in tests/golden/nee_paths_small.npz."""
import ctypes
import os
import sys

import numpy as np
import pytest

import nee_paths_ref as npr

pytestmark = pytest.mark.skipif(not npr.available(), reason="no C compiler for tests/native/nee_paths_shade.c")


@pytest.fixture(scope="module")
def ref(pkg, ob):
    return npr.NeePathsRef(pkg, ob)


@pytest.mark.parametrize("name", npr.PIN_CASES)
def test_two_bounces_are_the_oracles_nee_estimator(pkg, ob, name):
    """max_path_bounces = 2 marches the primary segment and its shadow segments only; C2 has sigma_a = 0 and no mean colour, so
    weight[0] is exactly 1 and E = 0 + 1 * L = L: the image is oracle_render_scene_s_nee's, bit for bit."""
    params, surf, _ = npr.CASES[name](pkg)
    want = ob.Oracle(params, threads=16).render_scene_s_nee(npr.frame(ob), surf)
    got = npr.reference(pkg, ob, name, 2)
    assert want.sum() > 0
    assert np.array_equal(got.image, want), "pixels that differ: %d of %d" % ((got.image != want).sum(), want.size)
    # path segments + shadow segments, per pixel
    assert got.n_seg == got.marched[0] + got.light[0] + got.phase[0] and got.marched[0] == npr.W * npr.H * npr.SPP - got.n_miss
    if name == "uni":
        assert got.light[0] == 0 and got.phase[0] > 0
    elif name == "nee":
        assert got.light[0] > 0 and got.phase[0] == 0
    else:
        assert got.light[0] > 0 and got.phase[0] > 0


def test_shade_helpers_are_the_oracles(ob):
    """conductorReflectance, powerHeuristic, the cap pdf and the tangent frame of nee_paths_shade.c against the oracle's pinning
    surface, bit for bit on random inputs."""
    L, O = npr.shade_lib(), ob.oracle_lib()
    f32 = ctypes.c_float
    for name, n_args in (("conductor_reflectance", 3), ("power_heuristic", 2), ("spherical_cap_pdf", 1)):
        fn = getattr(O, "oracle_" + name)
        fn.argtypes, fn.restype = [f32] * n_args, f32
    rng = np.random.default_rng(11)
    as_bits = lambda v: np.float32(v).view(np.uint32)      # noqa: E731
    for eta, k, c in np.concatenate([rng.uniform(0.0, 4.0, (300, 3)) * (1, 1, 0.25), [(0, 0, 0.3), (0, 2, 0.5), (1.5, 0, 1.0), (0.2, 3.9, 0.0)]]):
        assert as_bits(L.nee_paths_conductor_reflectance(eta, k, c)) == as_bits(O.oracle_conductor_reflectance(eta, k, c)), (eta, k, c)
    for a, b in rng.uniform(0.0, 50.0, (300, 2)) + 1e-3:
        assert as_bits(L.nee_paths_power_heuristic(a, b)) == as_bits(O.oracle_power_heuristic(a, b))
    for c in rng.uniform(-0.99, 0.999, 300):
        assert as_bits(L.nee_paths_spherical_cap_pdf(c)) == as_bits(O.oracle_spherical_cap_pdf(c))
    vp = ctypes.c_void_p
    for _ in range(300):
        n = rng.normal(size=3).astype(np.float32)
        n /= np.linalg.norm(n)
        p = rng.normal(size=3).astype(np.float32)
        for mine, theirs, size, args in (("tangent_frame", "tangent_frame", 9, (n,)), ("frame_to_local", "frame_to_local", 3, (n, p)),
                                         ("frame_to_global", "frame_to_global", 3, (n, p))):
            a, b = np.zeros(size, dtype=np.float32), np.zeros(size, dtype=np.float32)
            getattr(L, "nee_paths_" + mine)(*[x.ctypes.data_as(vp) for x in args], a.ctypes.data_as(vp))
            getattr(O, "oracle_" + theirs)(*[x.ctypes.data_as(vp) for x in args], b.ctypes.data_as(vp))
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (mine, n, p)


@pytest.mark.parametrize("name", npr.PIN_CASES)
def test_the_bounces_are_there(pkg, ob, name):
    """A condition on the reference alone: the rough C2 medium (sigma / lengthScale = 2) sends at least a quarter of the paths that
    hit at bounce 0 into a second hit, and what they gather changes the image."""
    c4, c2 = npr.reference(pkg, ob, name, 4), npr.reference(pkg, ob, name, 2)
    assert len(c4.hits) == 3 and c4.hits[0] == c2.hits[0] > 0
    assert 4 * c4.hits[1] >= c4.hits[0], c4.hits
    assert c4.hits[2] > 0 and c4.marched[1] <= c4.hits[0] and c4.marched[2] <= c4.hits[1]
    assert not np.array_equal(c4.image, c2.image)
    assert c4.n_seg > c2.n_seg


def test_one_bounce_adds_zeros(pkg, ob):
    c = npr.reference(pkg, ob, "mis", 1)
    assert not c.image.any() and not c.seg_count.any() and c.marched == []


@pytest.mark.parametrize("kind", ["rows", "spp", "shards"])
def test_composite_does_not_depend_on_the_cutting(pkg, ob, ref, kind):
    """Rows and shards partition the pixels, so the parts add up to the whole frame's image bit for bit.  The spp ranges {0} and
    {1, 2} add a0 + (a1 + a2) where the whole frame adds (a0 + a1) + a2: there the counts are compared exactly, the image to rounding,
    and three calls of one sample each, which add in the frame's own order, exactly."""
    params, surf, _ = npr.CASES["mis"](pkg)
    whole = npr.reference(pkg, ob, "mis", 4)
    orc = ob.Oracle(params, threads=16)
    acc, singles = None, []
    for s in npr.parts(ob, kind):
        acc = ref.compose(orc, s, surf, 4, into=acc)
        singles.append(ref.compose(orc, s, surf, 4))
    assert np.array_equal(acc.seg_count, whole.seg_count)
    assert acc.marched == whole.marched and acc.hits == whole.hits and acc.light == whole.light and acc.phase == whole.phase
    if kind != "spp":
        assert np.array_equal(acc.image, whole.image)
    else:
        assert np.array_equal(acc.image, singles[0].image + singles[1].image)
        assert np.allclose(acc.image, whole.image, rtol=1e-6, atol=0)
        # one sample per call adds ((0 + a0) + a1) + a2, the whole frame's own order
        one = None
        for k in range(npr.SPP):
            s = npr.frame(ob)
            s["spp_begin"], s["spp_count"] = k, 1
            one = ref.compose(orc, s, surf, 4, into=one)
        assert np.array_equal(one.image, whole.image) and np.array_equal(one.seg_count, whole.seg_count)


def test_golden_fixture_regenerates(pkg, ob):
    """tests/golden/nee_paths_small.npz is what tests/golden/make_nee_paths_golden.py writes today."""
    sys.path.insert(0, os.path.join(npr.ROOT, "tests", "golden"))
    import make_nee_paths_golden as mk
    have = np.load(npr.GOLDEN)
    want = mk.arrays(pkg, ob)
    assert sorted(have.files) == sorted(want)
    def same(a, b):          # field by field: the padding bytes of a record are not data
        if b.dtype.names:
            return a.dtype.names == b.dtype.names and a.dtype.itemsize == b.dtype.itemsize and all(same(a[f], b[f]) for f in b.dtype.names)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    for k in want:
        assert same(have[k], want[k]), k
