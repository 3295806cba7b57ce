"""The CPU composite of gpis_render_scene_s_material_paths_rgb (tests/material_paths_ref.py around
tests/native/material_paths_shade.c), pinned without a GPU: the conductor branch to tests/nee_paths_rgb_ref.py's composite bit for
bit, the Lambert branch to its pieces — the disk sampler to tests/native/paths_rgb_shade.c's, the MIS estimator to its closed form.
Above those pieces the Lambert branch is a restatement of TraceBase.cpp / LambertBsdf.cpp whose parity with the reference is
unpinned."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import material_paths_ref as mp
import nee_paths_rgb_ref as rgb
import paths_rgb_ref

PLAIN = ("mis", "nee", "uni", "mis-colour")


@pytest.fixture(scope="module", autouse=True)
def _needs_the_shade_step():
    if not mp.available():
        pytest.skip("no C compiler for the shade step")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_p = mp._p


def _plain(pkg, ob, name, max_bounces, mats):
    params, _ = mp.PLAIN_CASES[name](pkg)
    return mp.MaterialPathsRef(pkg, ob).compose(ob.Oracle(params, threads=16), mp.frame(ob), mats, max_bounces)


def test_bindings_mirror_the_header(pkg):
    assert pkg.MATERIAL_RGB.itemsize == 48 and pkg.MATERIALS_S.itemsize == 32 + 4 * 48 and pkg.MAX_MATERIALS == 4
    t = pkg.default_materials()
    cu = pkg.default_surface_rgb()
    assert int(t["n_materials"]) == 2 and t["cap_cos"] == cu["cap_cos"] and np.array_equal(t["cap_radiance"], cu["cap_radiance"])
    m = t["material"]
    assert int(m[0]["type"]) == pkg.MATERIAL.CONDUCTOR and np.array_equal(m[0]["eta"], cu["eta"]) and np.array_equal(m[0]["k"], cu["k"])
    assert np.array_equal(m[0]["albedo"], cu["albedo"])
    assert int(m[1]["type"]) == pkg.MATERIAL.LAMBERT and np.array_equal(m[1]["albedo"], np.full(3, 0.8, dtype=np.float32))
    assert not t["material"][2:].tobytes().strip(b"\0")
    header = open(os.path.join(mp.ROOT, "include", "gpis.h")).read()
    for name in ("gpis_default_materials", "gpis_render_scene_s_material_paths_rgb", "gpis_render_scene_s_material_paths_rgb_adaptive"):
        assert name + "(" in header and name in pkg.GpisLib.SYMBOLS
    assert "#define GPIS_MAX_MATERIALS 4" in header


@pytest.mark.parametrize("name", PLAIN)
def test_equal_conductors_equal_the_conductor_composite(pkg, ob, name):
    """every entry of the table the same conductor: image and seg_count of nee_paths_rgb_ref's composite, bit for bit"""
    params, surf = mp.PLAIN_CASES[name](pkg)
    orc = ob.Oracle(params, threads=16)
    for max_bounces in mp.BOUNCES:
        want = rgb.NeePathsRgbRef(pkg, ob).compose(orc, mp.frame(ob), surf, max_bounces)
        for n in (1, 2, 4):
            got = mp.MaterialPathsRef(pkg, ob).compose(orc, mp.frame(ob), mp.table_of_surface(pkg, surf, n), max_bounces)
            assert np.array_equal(_bits(got.image), _bits(want.image)) and np.array_equal(got.seg_count, want.seg_count), (name, max_bounces, n)
            assert (got.marched, got.hits, got.light, got.phase) == (want.marched, want.hits, want.light, want.phase)
        assert want.image.any() == (max_bounces > 1)


def test_equal_conductors_on_the_csg_medium(pkg, ob):
    """the same on a medium whose hits carry both ids: the id moves nothing when the materials are equal"""
    params, _, _ = mp.CASES["mis/cu-la"](pkg)
    surf = rgb.copper(pkg)
    orc = ob.Oracle(params, threads=16)
    want = rgb.NeePathsRgbRef(pkg, ob).compose(orc, mp.frame(ob), surf, 4)
    got = mp.MaterialPathsRef(pkg, ob).compose(orc, mp.frame(ob), mp.table_of_surface(pkg, surf, 2), 4)
    assert got.ids[0][0] >= 100 and got.ids[0][1] >= 100
    assert np.array_equal(_bits(got.image), _bits(want.image)) and np.array_equal(got.seg_count, want.seg_count)


@pytest.mark.parametrize("name", PLAIN)
def test_without_csg_the_other_materials_change_nothing(pkg, ob, name):
    _, surf = mp.PLAIN_CASES[name](pkg)
    one = mp.table_of_surface(pkg, surf, 1)
    padded = np.array(one).copy()
    padded["n_materials"] = 4
    padded["material"][1], padded["material"][2], padded["material"][3] = mp.lambert(pkg), mp.conductor(pkg, albedo=(0.5, 0.5, 0.5)), mp.lambert(pkg, (0.1, 0.2, 0.3))
    a, b = _plain(pkg, ob, name, 4, one), _plain(pkg, ob, name, 4, padded)
    assert a.image.any() and sum(x[0] for x in a.ids) == sum(a.hits) and sum(sum(x[1:]) for x in a.ids) == 0
    assert np.array_equal(_bits(a.image), _bits(b.image)) and np.array_equal(a.seg_count, b.seg_count)
    # and a Lambert material[0] does change it
    lam = np.array(padded).copy()
    lam["material"][0] = mp.lambert(pkg)
    assert not np.array_equal(_plain(pkg, ob, name, 4, lam).image, a.image)


def test_an_id_beyond_the_table_takes_material_0(pkg, ob):
    """n_materials = 1 on the CSG medium: the hits of id 1 are shaded with material[0] — the frame of the table padded with a copy"""
    name = "mis/cu-la"
    la = mp.lambert(pkg)
    one, two = mp.table(pkg, [la]), mp.table(pkg, [la, la])
    a, b = mp.reference(pkg, ob, name, 4, mats=one), mp.reference(pkg, ob, name, 4, mats=two)
    assert a.ids[0][1] >= 100 and a.types[0] == [0, a.hits[0]]
    assert np.array_equal(_bits(a.image), _bits(b.image)) and np.array_equal(a.seg_count, b.seg_count)


def test_lambert_disk_sampler_is_paths_rgb_shade_s(pkg, ob):
    """Given one stream state, the direction and the state after: those of tests/native/paths_rgb_shade.c's bounce.  That step is
    given a hit the light does not reach (no shadow jitter is drawn before the disk pairs); it draws the next segment's jitter after
    them, which is one more draw than the sampler's."""
    ref, lib = mp.MaterialPathsRef(pkg, ob), paths_rgb_ref.shade_lib()
    rng = np.random.default_rng(2207)
    for trial in range(64):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        n32 = n.astype(np.float32)
        scene = np.array(ob.default_scene_s(4, 4, 1), dtype=pkg.SCENE_S).reshape(())
        scene["light_dir"] = -n32                                   # wo.z < 0: no next-event estimation, no jitter
        rays, seg = np.zeros(1, dtype=pkg.RAY_IN), np.zeros(1, dtype=pkg.SEG_OUT)
        rays["dir"][0] = -n32                                       # wi = the normal
        seg["ok"], seg["exited"], seg["aniso"], seg["weight"] = 1, 0, n32.astype(np.float64), 1.0
        state = int(rng.integers(1, 2 ** 63))
        st = np.array([state], dtype=np.uint64)
        albedo = np.ones(3, dtype=np.float32)
        hit, alive, nee = np.ones(1, dtype=np.uint8), np.ones(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        e3, thr, em, thr_b, contrib = (np.zeros(3, dtype=np.float32) for _ in range(5))
        thr[:] = 1.0
        segs, shadow = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=pkg.RAY_IN)
        lib.paths_rgb_shade(_p(scene), 1, 0, 4, 0, _p(albedo), _p(rays), _p(seg), _p(hit), _p(e3), _p(st), _p(thr), _p(em), _p(segs), _p(alive),
                            _p(thr_b), _p(shadow), _p(contrib), _p(nee))
        assert alive[0] == 1 and nee[0] == 0
        w, after = ref.lambert_direction(state, n32)
        assert np.array_equal(_bits(w), _bits(rays["dir"][0])), trial
        after = (after * 6364136223846793005 + 1) % 2 ** 64           # the jitter paths_rgb_shade draws behind the direction
        assert after == int(st[0]), trial


def test_lambert_mis_estimator_has_its_closed_form(pkg, ob):
    """A hit whose normal is the cap axis, seen along the normal, every shadow segment visible: E[L[c]] = albedo[c] / pi *
    cap_radiance[c] * integral over the cap of cos = albedo[c] * cap_radiance[c] * (1 - cap_cos^2).  2^18 streams from fixed seeds
    through the C set-up, shade and gather; tolerance: 4 standard errors of the C step's own sample variance."""
    ref = mp.MaterialPathsRef(pkg, ob)
    n = 1 << 18
    for cap_cos, seed in ((float(pkg.default_surface_rgb()["cap_cos"]), 11), (0.5, 12), (0.0, 13)):
        albedo, radiance = (0.8, 0.6, 0.4), (20.0, 15.0, 10.0)
        mats = mp.table(pkg, [mp.lambert(pkg, albedo)], cap_cos=cap_cos, cap_radiance=radiance)
        scene = np.array(ob.default_scene_s(4, 4, 1), dtype=pkg.SCENE_S).reshape(())
        axis = np.array(scene["light_dir"], dtype=np.float64)
        axis /= np.linalg.norm(axis)
        a32 = np.array([ctypes.c_float(x).value for x in axis], dtype=np.float32)
        # the normal the step derives is aniso / |aniso| in double rounded to float: give it the cap axis the step itself uses
        rays, seg = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=pkg.SEG_OUT)
        rays["dir"] = -a32
        seg["ok"], seg["exited"], seg["aniso"], seg["weight"], seg["scheme"] = 1, 0, a32.astype(np.float64), 1.0, 2
        rng = np.random.default_rng(seed).integers(1, 2 ** 63, size=n).astype(np.uint64)
        alive = np.ones(n, dtype=np.uint8)
        thr, em = np.ones((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
        e, segs = np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.uint32)
        hits, coeff = np.zeros(n, dtype=mp.HIT), np.zeros(n, dtype=pkg.COND_COEFF)
        qh, qn = np.zeros(n, dtype=pkg.NEE_QUERY), np.zeros(n, dtype=pkg.NEE_QUERY)
        shl, shp = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=pkg.RAY_IN)
        ref.lib.mat_paths_setup(_p(scene), _p(mats), n, 0, 2, 0, _p(alive), _p(rays), _p(seg), _p(coeff), _p(e), _p(rng), _p(thr), _p(em), _p(segs),
                                _p(hits), _p(qh), _p(qn))
        assert hits["h"]["hit"].all() and (hits["wi_z"] > 0.999).all()
        ref.lib.mat_paths_shade(_p(scene), _p(mats), n, 0, 1, _p(alive), _p(rays), _p(seg), _p(rng), _p(thr), _p(segs), _p(hits), _p(shl), _p(shp))
        H = hits["h"]
        H["vis_light"], H["vis_phase"] = H["go_light"], H["go_phase"]
        assert H["go_light"].mean() > 0.99 and H["go_phase"].any() and H["go_phase"].all() == (cap_cos == 0.0)
        ref.lib.mat_paths_gather(_p(mats), n, _p(hits), _p(em))
        L = em.astype(np.float64)
        for c in range(3):
            want = albedo[c] * radiance[c] * (1.0 - cap_cos * cap_cos)
            mean, err = L[:, c].mean(), L[:, c].std(ddof=1) / np.sqrt(n)
            print("cap_cos %g channel %d: mean %.6f want %.6f, 4 standard errors %.6f" % (cap_cos, c, mean, want, 4 * err))
            assert abs(mean - want) <= 4 * err, (cap_cos, c, mean, want, err)


def test_csg_frame_exercises_both_materials(pkg, ob):
    for name in ("mis/cu-la", "single/cu-la"):
        c = mp.reference(pkg, ob, name, 4)
        print(name, "ids", c.ids, "types", c.types, "light", c.light, "visible", c.light_visible, "phase", c.phase)
        assert c.ids[0][0] >= 100 and c.ids[0][1] >= 100 and c.types[0] == c.ids[0][:2]
        assert len(c.marched) == 3 and c.marched[2] > 0 and sum(c.light_visible) > 0 and sum(c.phase) > 0 and sum(c.exits) > 0


def test_separate_case_sees_both_ids(pkg, ob):
    c = mp.reference(pkg, ob, "separate/cu-la", 4)
    print("ids", c.ids)
    assert c.ids[0][0] >= 100 and c.ids[0][1] >= 100 and c.image.any()


def test_tables_differ(pkg, ob):
    """swapping the two materials, and two Lambert materials, give other frames and other segment counts"""
    a, b, c = (mp.reference(pkg, ob, "mis/" + t, 4) for t in ("cu-la", "la-cu", "la-la"))
    assert a.types[0] == b.types[0][::-1] and c.types[0][0] == 0
    assert not np.array_equal(a.image, b.image) and not np.array_equal(a.image, c.image) and not np.array_equal(a.seg_count, b.seg_count)


def test_emissive_case(pkg, ob):
    first, full = mp.reference(pkg, ob, mp.EMISSIVE_CASE, 1), mp.reference(pkg, ob, mp.EMISSIVE_CASE, 4)
    assert first.image.any() and first.marched == [first.n_samples - first.n_miss] and not first.light and not first.phase
    assert len(full.marched) == 4 and full.marched[3] > 0 and (full.image >= first.image).all()


def test_fixture_is_current(pkg, ob):
    spec = importlib.util.spec_from_file_location("make_material_paths_golden", os.path.join(os.path.dirname(mp.GOLDEN), "make_material_paths_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want, got = mod.arrays(pkg, ob), np.load(mp.GOLDEN)
    assert sorted(want) == sorted(got.files)
    for key in want:
        assert np.asarray(want[key]).tobytes() == np.asarray(got[key]).tobytes(), key
    assert os.path.getsize(mp.GOLDEN) < 1 << 20
