"""The shapes the other weight-space tests never reach: batches of more segments than any grid of resident waves, so that every
wave of k_ws_march / k_ws_eval walks several segments (realization slice rebuilt in place, LDS block, range flag and tallies carried
over), workspace growth on one handle, a range error late in a long batch, frames in which every wave of k_ws_scene fetches many
samples, and frames of more than one chunk of 2^22 samples (chunk loop, first_pixel != 0, counter reset, record reuse, shards).
Everything is bit for bit: against the plain-C restatement, against the CPU composite, or against the same work cut differently."""
import numpy as np
import pytest

import ws_oracle
import ws_scene_ref
from test_gpu_ws import _same_seg
from test_gpu_ws_scene import _accumulate, _bits, _non_vacuous

pytestmark = pytest.mark.gpu

CHUNK = 2 ** 22                 # kFrameChunk (ws_frame, csrc/gpis_ws_host.hpp)

# name -> ws_params keywords.  N <= 65 except the one N = 300 per-path case.
BATCH_CASES = {
    "per_path-n65": dict(ctx="renewal", n_basis=65),
    "single-fd-n64": dict(ctx="none", single=1, normal=1, n_basis=64),
    "per_path-fd-n8": dict(ctx="renewal_plus", normal=1, n_basis=8),
    "per_path-csg-n63": dict(ctx="global", n_basis=63, mean_additional=True),
    "absorption_only-n16": dict(ctx="renewal", n_basis=16, absorption_only=True),
    "per_path-n300": dict(ctx="renewal", n_basis=300),
}


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


@pytest.fixture(scope="module")
def ref(pkg, ob, wso):
    return ws_scene_ref.SceneRef(pkg, ob, wso)


@pytest.fixture(scope="module")
def waves():
    """32 one-wave workgroups per CU is the hardware ceiling (the 18 KB LDS block allows 8): no grid of resident waves is larger"""
    import torch
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def _batch(pkg, n, seed):
    rng = np.random.default_rng(seed)
    rays, kind = ws_oracle.mixed_rays(pkg, rng, n)
    return rays, kind, ws_oracle.random_queries(pkg, rng, n), rng.permutation(n)


@pytest.mark.parametrize("case", sorted(BATCH_CASES))
def test_batch_above_any_resident_grid(pkg, wso, waves, case):
    n = 3 * waves + 17                  # every wave takes >= 3 segments, with a ragged tail, whatever grid the library picks
    p, w = ws_oracle.ws_params(pkg, **BATCH_CASES[case])
    rays, kind, q, perm = _batch(pkg, n, sorted(BATCH_CASES).index(case))
    assert all((kind == k).sum() > n // 10 for k in range(5))
    m = pkg.WeightSpaceMedium(p, w)
    m.reset_counters()
    out = m.sample_distance_batch(rays)
    c_sd = m.counters()
    vis = m.transmittance_batch(rays)
    c_tr = m.counters()
    v, g, gid = m.eval(q)
    # a segment's result depends neither on the wave that ran it nor on what that wave ran before (no oracle needed)
    _same_seg(m.sample_distance_batch(rays[perm]), out[perm])
    assert np.array_equal(m.transmittance_batch(rays[perm]), vis[perm])
    vp, gp, ip = m.eval(q[perm])
    assert np.array_equal(vp.view(np.uint64), v[perm].view(np.uint64)) and np.array_equal(gp.view(np.uint64), g[perm].view(np.uint64))
    assert np.array_equal(ip, gid[perm])
    m.close()
    want, e_sd = wso.sample_distance(p, w, rays)
    vis_want, e_tr = wso.transmittance(p, w, rays)
    wv, wg, wi = wso.eval(p, w, q)
    print(case, "n", n, "hits", int((want["exited"] == 0).sum()), "ok", int(want["ok"].sum()), "blocked", int((vis_want == 0).sum()), "n_eval", e_sd, e_tr)
    _same_seg(out, want)
    assert np.array_equal(vis, vis_want)
    assert np.array_equal(v.view(np.uint64), wv.view(np.uint64)) and np.array_equal(g.view(np.uint64), wg.view(np.uint64)) and np.array_equal(gid, wi)
    assert c_sd["n_seg"] == n and c_tr["n_seg"] == 2 * n
    assert c_sd["n_eval"] == e_sd and c_tr["n_eval"] == e_sd + e_tr, (c_sd, c_tr, e_sd, e_tr)
    assert (vis_want == 0).sum() > n // 10 and (vis_want != 0).sum() > n // 10
    if not BATCH_CASES[case].get("absorption_only"):
        assert ((want["exited"] == 0) & (want["ok"] == 1)).sum() > n // 10 and (want["exited"] != 0).sum() > n // 10


@pytest.mark.parametrize("kw", [dict(ctx="renewal", n_basis=65), dict(ctx="none", single=1, n_basis=65)], ids=["per_path", "single"])
def test_workspace_growth_on_one_handle(pkg, waves, kw):
    """small call, large call (the per-path workspace and the staging buffers are reallocated), small call again"""
    n = 3 * waves + 17
    p, w = ws_oracle.ws_params(pkg, **kw)
    rays, _, q, _ = _batch(pkg, n, 40)
    small, small_q = rays[5:37], q[5:37]
    m = pkg.WeightSpaceMedium(p, w)
    first = (m.sample_distance_batch(small), m.sample_distance(small), m.transmittance_batch(small), m.eval(small_q))
    large = (m.sample_distance_batch(rays), m.sample_distance(rays), m.transmittance_batch(rays), m.eval(q))
    third = (m.sample_distance_batch(small), m.sample_distance(small), m.transmittance_batch(small), m.eval(small_q))
    m.close()
    fresh = pkg.WeightSpaceMedium(p, w)
    want = (fresh.sample_distance_batch(rays), fresh.sample_distance(rays), fresh.transmittance_batch(rays), fresh.eval(q))
    fresh.close()
    for a, b in ((first, third), (large, want)):
        _same_seg(a[0], b[0])
        _same_seg(a[1], b[1])
        assert np.array_equal(a[2], b[2])
        for x, y in zip(a[3], b[3]):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    _same_seg(large[0][5:37], first[0])
    _same_seg(large[0], large[1])
    assert np.array_equal(large[2][5:37], first[2])


def test_range_flag_after_a_long_batch(pkg, wso, waves):
    """One query beyond the restated cos range late in a batch every wave walks three times: the call is refused (an ordinary
    error return), and the next call on the same handle is clean and right."""
    n = 3 * waves + 17
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=8)
    q = ws_oracle.random_queries(pkg, np.random.default_rng(50), n)
    bad = q.copy()
    late = 2 * waves + 11
    bad["p"][late] = (3e9, 0.0, 0.0)
    m = pkg.WeightSpaceMedium(p, w)
    with pytest.raises(RuntimeError, match="105414350"):
        m.eval(bad)
    v, g, gid = m.eval(q)
    m.close()
    wv, wg, wi = wso.eval(p, w, q)
    assert np.array_equal(v.view(np.uint64), wv.view(np.uint64)) and np.array_equal(g.view(np.uint64), wg.view(np.uint64)) and np.array_equal(gid, wi)


@pytest.mark.parametrize("ctx,single", [("renewal", 0), ("global", 0), ("none", 1)])
def test_frame_where_every_wave_takes_many_samples(pkg, ob, ref, ctx, single):
    p, w = ws_oracle.ws_params(pkg, ctx=ctx, single=single, n_basis=65)
    scene = ws_scene_ref.small_scene(ob, width=96, height=64, spp=5)            # 30 720 samples
    want = ref.compose(p, w, scene)
    _non_vacuous(want, {})
    m = pkg.WeightSpaceMedium(p, w)
    m.reset_counters()
    img, hits = m.render_scene_s(scene, want_hits=True)
    c = m.counters()
    m.close()
    assert np.array_equal(hits, want.hits)
    assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]
    assert c["n_eval"] == want.n_eval and c["n_seg"] == want.n_seg, (c, want.n_eval, want.n_seg)


def _big(ob, spp):
    s = ws_scene_ref.small_scene(ob, width=1000, height=1500, spp=spp, fov=60.0)
    s["tile_size"] = 16
    # Seen from (0, 0, 4) the bounding sphere covers rows 400 - 1100 only and every sample from row 1100 on is a miss: the second
    # chunk would add zeros, wherever it added them.  From (0, 3, 4) the sphere's centre projects onto row 1399, so hits, exits
    # and misses lie on both sides of the chunk boundary (test_frame_of_two_chunks asserts it on the composite of rows 1396 - 1400).
    s["cam_pos"] = (0.0, 3.0, 4.0)
    return s


def _rows(ob, spp, ranges):
    out = []
    for y0, yc in ranges:
        s = _big(ob, spp)
        s["y_begin"], s["y_count"] = y0, yc
        out.append(s)
    return out


def _render_counted(pkg, m, scenes):
    m.reset_counters()
    img, hits = _accumulate(pkg, m, scenes)
    return img, hits, m.counters()


def test_frame_of_two_chunks(pkg, ob, ref):
    """1000 x 1500 x 3 = 4.5 M samples: two chunks, the boundary at pixel 1 398 101 (row 1398, column 101).  (i) The whole frame
    equals the frame accumulated from calls of <= 1000 rows, each a single chunk (the path test_gpu_ws_scene.py pins to the
    composite); (ii) the rows around the boundary equal the CPU composite; the segment counts add up."""
    spp, width, height = 3, 1000, 1500
    assert width * height * spp > CHUNK and (CHUNK // spp) % width != 0
    assert (CHUNK // spp) // width == 1398 and (CHUNK // spp) % width == 101
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=8)
    m = pkg.WeightSpaceMedium(p, w)
    whole, whole_hits, c_whole = _render_counted(pkg, m, [_big(ob, spp)])
    parts = _rows(ob, spp, ((0, 1000), (1000, 500)))
    assert all(int(s["y_count"]) * width * spp <= CHUNK for s in parts)
    got, got_hits, c_parts = _render_counted(pkg, m, parts)
    assert whole_hits[:1398].any() and whole_hits[1399:].any()                 # both chunks hold hits
    assert np.array_equal(got_hits, whole_hits)
    assert np.array_equal(_bits(got), _bits(whole)), np.argwhere(_bits(got) != _bits(whole))[:8]
    assert c_whole["n_seg"] == c_parts["n_seg"] and c_whole["n_eval"] == c_parts["n_eval"], (c_whole, c_parts)
    strip = _rows(ob, spp, ((1396, 5),))[0]
    want = ref.compose(p, w, strip)
    _non_vacuous(want, {})
    m.close()
    assert np.array_equal(whole_hits[1396:1401], want.hits[1396:1401])
    assert np.array_equal(_bits(whole[1396:1401]), _bits(want.image[1396:1401]))


@pytest.mark.parametrize("spp", [3, 9])
def test_sharded_frame_against_its_rows(pkg, ob, spp):
    """Shard 0 of 3 (tile rows 0, 3, ..., 93 of 16 rows, the last one of 12) of the 1000 x 1500 frame against the same rows rendered
    tile row by tile row without shards.  With spp 3 the shard is one chunk; with spp 9 it is 508 000 pixels x 9 = 4.57 M samples,
    two chunks whose boundary (pixel 466 033 of the shard) lies inside a row: first_pixel != 0 under scene_pixel's shard mapping."""
    width, height = 1000, 1500
    shard = _big(ob, spp)
    shard["shard_index"], shard["shard_count"] = 0, 3
    tiles = [(16 * t, min(16, height - 16 * t)) for t in range(0, (height + 15) // 16, 3)]
    n_pix = sum(yc for _, yc in tiles) * width
    if spp == 9:
        assert n_pix * spp > CHUNK and (CHUNK // spp) % width != 0
    p, w = ws_oracle.ws_params(pkg, ctx="global", n_basis=8)
    m = pkg.WeightSpaceMedium(p, w)
    img, hits, c_shard = _render_counted(pkg, m, [shard])
    got, got_hits, c_rows = _render_counted(pkg, m, _rows(ob, spp, tiles))
    m.close()
    mask = np.zeros(height, dtype=bool)
    for y0, yc in tiles:
        mask[y0:y0 + yc] = True
    assert img[mask].any() and not img[~mask].any() and not hits[~mask].any()
    assert np.array_equal(got_hits, hits)
    assert np.array_equal(_bits(got), _bits(img)), np.argwhere(_bits(got) != _bits(img))[:8]
    assert c_shard["n_seg"] == c_rows["n_seg"] and c_shard["n_eval"] == c_rows["n_eval"], (c_shard, c_rows)
