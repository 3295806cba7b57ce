"""CPU checks of the function-space path frame (gpis_fs_render_scene_s_paths): the declared and exported interface, the pin of
the split shade step (tests/native/fs_paths_shade.c) to ws_paths_shade.c — itself pinned to the oracle of
gpis_render_scene_s_paths by tests/test_ws_paths_cpu.py —, the tie of the composite (tests/fs_paths_ref.py) to the scene
composite at max_bounces = 1, the non-vacuity of every GPU case's composite, the sensitivity of the composite to the two ways of
getting the shadow segment's state wrong, and its recorded fixture."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fs_paths_ref
import fs_scene_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fs_paths_small.npz")
needs_cc = pytest.mark.skipif(not fs_paths_ref.available(), reason="no C compiler for the shade step")
_p = fs_paths_ref._p

# Composite.class_counts() of each case, as recorded when the cases were chosen: samples, miss, path segments, shadow segments,
# paths with >= 2 hits, with >= 3 hits, exits after a hit, ended below, ended without a chord, ended !ok, visible, occluded,
# shadow segments followed by a further path segment
EXPECTED = {
    "absorption_only": [1536, 661, 875, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    "albedo1": [1536, 661, 1530, 461, 175, 85, 369, 0, 0, 28, 263, 198, 461],
    "aniso": [1536, 661, 1463, 441, 103, 32, 226, 0, 0, 232, 191, 250, 441],
    "bounces1": [1536, 661, 875, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0],
    "bounces2": [1536, 661, 1359, 369, 105, 0, 188, 0, 0, 195, 151, 218, 369],
    "bounces4": [1536, 661, 1643, 523, 179, 109, 399, 0, 0, 25, 282, 241, 523],
    "global-14": [1536, 661, 1530, 461, 175, 85, 369, 0, 0, 28, 263, 198, 461],
    "global-64": [192, 81, 192, 55, 23, 16, 42, 0, 0, 0, 30, 25, 55],
    "homogeneous": [1536, 661, 1653, 494, 198, 102, 175, 0, 0, 590, 151, 343, 494],
    "none-12": [1536, 661, 1416, 336, 107, 27, 172, 0, 0, 235, 141, 195, 336],
    "renewal-16": [1536, 661, 1464, 431, 105, 28, 221, 0, 0, 239, 178, 253, 431],
    "renewal_plus-32": [1536, 661, 1531, 462, 169, 90, 389, 0, 0, 10, 266, 196, 462],
}


@pytest.fixture(scope="module")
def ref(pkg, ob):
    return fs_paths_ref.FsPathsRef(pkg, ob)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_path_entry_is_declared():
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    assert re.search(r"^int\s+gpis_fs_render_scene_s_paths\s*\(gpis_medium \*m, const gpis_scene_s \*s, int max_path_bounces, float albedo,\s*"
                     r"float \*radiance_sum, uint32_t \*seg_count, void \*stream\);", header, flags=re.M)
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    assert callable(getattr(pkg.Medium, "fs_render_scene_s_paths", None))
    assert "gpis_fs_render_scene_s_paths" in pkg.GpisLib.SYMBOLS


def test_library_exports_the_path_entry(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    assert re.search(r"\bT gpis_fs_render_scene_s_paths$", out, flags=re.M)


def _same_ray(a, b, skip=("u_jitter",)):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)) for f in a.dtype.names if f not in skip)


@needs_cc
def test_split_shade_step_is_ws_paths_shade(pkg, ob, ref):
    """On the rays and segment results the composite recorded at every bounce level of a 4-bounce frame (hits, exits and !ok
    results among them), with throughputs and stream states of the same run:
      bounce < max - 1 — fs_paths_nee gives ws_paths_shade's nee, contrib and shadow ray (all fields but u_jitter, which
          ws_paths_shade draws and this medium does not read); and fs_paths_bounce, started where ws_paths_shade's stream
          stands after that one draw, gives its next ray (but u_jitter), throughput, alive and end;
      bounce = max - 1 — ws_paths_shade draws no u_shadow, so fs_paths_bounce from the SAME stream state gives the same next
          dir / far_t / throughput / alive / end, and ws_paths_shade's stream is one draw (the next u_jitter) further."""
    p, scene, _, albedo, _ = fs_paths_ref.case(pkg, ob, "bounces4")
    scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    c = ref.compose(p, scene, 4, albedo)
    f32 = ctypes.c_float
    seen = dict(nee=0, lives=0, exited=0, not_ok=0, last=0, below=0, no_chord=0)
    levels = [(b, lv["rays"], lv["seg"], lv) for b, lv in enumerate(c.levels)]
    # This medium's own hits never end a path below the surface or without a chord (fs_paths_ref.EXCLUDED_BY_THE_MEDIUM), so the
    # same records are fed once more with every third ray reversed (wi.z < 0) and every fifth hit point pushed outside the
    # bounding sphere (some bounce directions then have no chord): both files must take those ends alike as well.
    for b, lv in enumerate(c.levels):
        rays_x, seg_x = lv["rays"].copy(), lv["seg"].copy()
        rays_x["dir"][::3] *= np.float32(-1.0)
        seg_x["p"][::5] *= np.float32(1.6)
        levels.append((b, rays_x, seg_x, lv))
    for bounce, rays_in, seg, lv in levels:
        n = len(lv["idx"])
        rng0 = lv["rng_after_shadow"].astype(np.uint64)
        thr0 = (np.float32(0.25) + np.float32(0.75) * (np.arange(n, dtype=np.float32) / np.float32(n))).astype(np.float32)
        for max_bounces in (bounce + 2, bounce + 1):
            last = max_bounces == bounce + 1
            # ws_paths_shade
            rays_w, rng_w, thr_w, alive_w = rays_in.copy(), rng0.copy(), thr0.copy(), np.ones(n, dtype=np.uint8)
            shadow_w, contrib_w = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=np.float32)
            nee_w, end_w = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            ref.lib.ws_paths_shade(_p(scene), n, bounce, max_bounces, f32(albedo), _p(rays_w), _p(seg), _p(rng_w), _p(thr_w), _p(alive_w),
                                   _p(shadow_w), _p(contrib_w), _p(nee_w), _p(end_w))
            # the two halves
            rays_f, thr_f, alive_f = rays_in.copy(), thr0.copy(), np.ones(n, dtype=np.uint8)
            shadow_f, contrib_f = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=np.float32)
            nee_f, end_f = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            ref.lib.fs_paths_nee(_p(scene), n, bounce, max_bounces, f32(albedo), _p(rays_f), _p(seg), _p(thr_f), _p(alive_f),
                                 _p(shadow_f), _p(contrib_f), _p(nee_f), _p(end_f))
            assert np.array_equal(nee_f, nee_w) and np.array_equal(_bits(contrib_f), _bits(contrib_w))
            k = np.nonzero(nee_w)[0]
            assert last == (len(k) == 0)
            assert _same_ray(shadow_f[k], shadow_w[k])
            # where ws_paths_shade drew u_shadow its stream is one transition ahead of the state it was given
            rng_f = rng0.copy()
            rng_f[k] = rng_f[k] * np.uint64(fs_scene_ref.PCG_MULT) + np.uint64(1)
            ref.lib.fs_paths_bounce(_p(scene), n, bounce, f32(albedo), _p(rays_f), _p(seg), _p(rng_f), _p(thr_f), _p(alive_f), _p(end_f))
            assert np.array_equal(alive_f, alive_w) and np.array_equal(end_f, end_w) and np.array_equal(_bits(thr_f), _bits(thr_w))
            live = np.nonzero(alive_w)[0]
            assert _same_ray(rays_f[live], rays_w[live]) and (rays_f["segment"][live] == bounce + 1).all()
            assert np.array_equal(rng_w[live], rng_f[live] * np.uint64(fs_scene_ref.PCG_MULT) + np.uint64(1))     # the next u_jitter
            dead = np.nonzero(alive_w == 0)[0]
            assert np.array_equal(rng_w[dead], rng_f[dead])
            seen["nee"] += len(k)
            seen["lives"] += len(live)
            seen["exited"] += int((end_w == fs_paths_ref.END_EXITED).sum())
            seen["not_ok"] += int((end_w == fs_paths_ref.END_NOT_OK).sum())
            seen["last"] += int(last and len(live) > 0)
            seen["below"] += int((end_w == fs_paths_ref.END_BELOW).sum())
            seen["no_chord"] += int((end_w == fs_paths_ref.END_NO_CHORD).sum())
    assert len(c.levels) == 4 and all(v > 0 for v in seen.values()), seen


@needs_cc
def test_one_bounce_is_the_scene_composites_primary_segment(pkg, ob, ref):
    """max_bounces = 1: one segment per sample that meets the bound, nothing observable after it.  The image is all zero, the
    segment counts are the non-missing samples per pixel, and the segment-0 results and states are those of the primary segments
    of fs_scene_ref.compose on the same scene, bit for bit: camera, sampler and empty state are the existing composite's."""
    p, scene, max_bounces, albedo, _ = fs_paths_ref.case(pkg, ob, "bounces1")
    assert max_bounces == 1
    c = ref.compose(p, scene, 1, albedo)
    assert not c.image.any() and c.n_shadow_seg == 0
    assert int(c.segs.sum()) == c.n_seg == c.n_samples - c.n_miss > 0 and c.n_miss > 0
    want = ref.scene_ref.compose(p, scene)
    assert want.n_samples == c.n_samples and want.n_miss == c.n_miss
    (lv,) = c.levels
    assert lv["seg"].tobytes() == want.last["seg"].tobytes()
    assert lv["states"].tobytes() == want.last["states"].tobytes() and lv["states_after"].tobytes() == want.last["states_after"].tobytes()
    per_pixel = np.zeros(c.segs.size, dtype=np.uint32)
    np.add.at(per_pixel, want.last["pix"], 1)
    assert np.array_equal(c.segs.reshape(-1), per_pixel)


@needs_cc
@pytest.mark.parametrize("name", sorted(fs_paths_ref.CASES))
def test_case_is_not_vacuous(pkg, ob, ref, name):
    """Every class a case can hold is in its frame; the classes it excludes by construction (max_bounces 1, absorption_only, and
    for this medium in every frame the end below the surface / without a chord: fs_paths_ref.EXCLUDED_BY_THE_MEDIUM) are
    asserted absent."""
    p, scene, max_bounces, albedo, impossible = fs_paths_ref.case(pkg, ob, name)
    c = ref.compose(p, scene, max_bounces, albedo)
    fs_paths_ref.check_non_vacuous(c, impossible)
    assert c.n_seg == c.n_path_seg + c.n_shadow_seg == int(c.segs.sum())
    assert c.image.any() == (c.n_visible > 0)
    if name in fs_paths_ref.THREE_HITS:
        assert max_bounces == 4 and c.n_three_hits > 0
    if max_bounces == 1:
        assert not c.image.any() and c.n_seg == c.n_samples - c.n_miss
    assert c.class_counts().tolist() == EXPECTED[name]


def test_a_four_bounce_case_asks_for_three_hits():
    assert any(fs_paths_ref.CASES[n][5] == 4 for n in fs_paths_ref.THREE_HITS)


@needs_cc
@pytest.mark.parametrize("ctx", ["RENEWAL", "RENEWAL_PLUS", "GLOBAL", "NONE"])
def test_composite_is_sensitive_to_the_shadow_state(pkg, ob, ref, ctx):
    """Renewal, Renewal+ and Global condition segment b + 1 on the context the path holds, so continuing from the context the
    shadow segment left (shadow_in_place) changes the image; under NONE it does not, by construction: applyMemory drops the
    values, the next segment reads nothing of the context it is handed (fs_intersect_gp: nc = 0) and rewrites it.  Not taking
    over the shadow segment's sampler state (fork_sampler) changes the draws of the bounce and of every later segment, whatever
    the context."""
    p = fs_scene_ref.fs_params(pkg, ctx, 16, 0.04)
    scene = fs_paths_ref.ws_scene_ref.small_scene(ob, 24, 16, 4, fov=60.0)
    good = ref.compose(p, scene, 3, 0.8)
    assert good.n_nee_then_segment > 0 and good.n_visible > 0
    in_place = ref.compose(p, scene, 3, 0.8, shadow_in_place=True)
    forked = ref.compose(p, scene, 3, 0.8, fork_sampler=True)
    same = np.array_equal(_bits(in_place.image), _bits(good.image)) and np.array_equal(in_place.segs, good.segs)
    assert same == (ctx == "NONE")
    assert not np.array_equal(_bits(forked.image), _bits(good.image))


@needs_cc
def test_composite_equals_fixture(pkg, ob, ref):
    g = np.load(GOLD)
    p = np.array(g["params"]).view(pkg.PARAMS).reshape(())
    scene = np.array(g["scene"]).view(pkg.SCENE_S).reshape(())
    c = ref.compose(p, scene, int(g["max_bounces"]), float(g["albedo"]))
    assert np.array_equal(_bits(c.image), _bits(g["image"])) and g["image"].any()
    assert np.array_equal(c.segs, g["segs"]) and np.array_equal(c.class_counts(), g["class_counts"])
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_fs_paths_golden as mk
    p2, scene2 = mk.fixture_inputs(pkg)
    assert p2.tobytes() == p.tobytes() and np.array(scene2, dtype=pkg.SCENE_S).tobytes() == scene.tobytes()
    assert (mk.MAX_BOUNCES, np.float32(mk.ALBEDO)) == (int(g["max_bounces"]), np.float32(g["albedo"]))
    assert int(p["correlation_context"]) == int(pkg.CTX.RENEWAL_PLUS)
