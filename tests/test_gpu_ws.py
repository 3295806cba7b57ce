"""GPU parity of the weight-space GP medium (gpis_ws_*): every result bit for bit against the plain-C restatement
(tests/native/ws_oracle.c, built on demand) and against the recorded fixture tests/golden/ws_small.npz."""
import ctypes
import os

import numpy as np
import pytest

import ws_oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_small.npz")
CTXS = ["global", "renewal_plus", "renewal", "none"]


@pytest.fixture(scope="module")
def wso():
    if not ws_oracle.available():
        pytest.skip("no C compiler for the restatement (the fixture test still runs)")
    return ws_oracle.WsOracle()


def _same_seg(got, want):
    for f in want.dtype.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (f, np.nonzero((a != b).reshape(len(a), -1).any(1))[0][:8], a[:4], b[:4])


def _medium(pkg, **kw):
    p, w = ws_oracle.ws_params(pkg, **kw)
    return pkg.WeightSpaceMedium(p, w), p, w


@pytest.mark.gpu
@pytest.mark.parametrize("n_basis", [0, 1, 63, 64, 65, 300, 301, 1024])
def test_basis_export(pkg, wso, n_basis):
    rng = np.random.default_rng(n_basis)
    pss = rng.integers(0, 2 ** 32, (24, 4), dtype=np.uint64).astype(np.uint32)
    for ctx, single in (("renewal", 0), ("global", 0), ("none", 1)):
        m, p, w = _medium(pkg, ctx=ctx, single=single, n_basis=n_basis)
        got = m.basis(pss)
        m.close()
        want = wso.basis(p, w, pss)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (ctx, single)


@pytest.mark.gpu
@pytest.mark.parametrize("single", [0, 1])
@pytest.mark.parametrize("normal", [0, 1])
def test_eval_value_gradient_id(pkg, wso, single, normal):
    q = ws_oracle.make_queries(pkg, 160, seed=10 + single)
    for extra in (False, True):
        m, p, w = _medium(pkg, ctx="renewal", single=single, normal=normal, mean_additional=extra)
        gv, gg, gi = m.eval(q)
        m.close()
        wv, wg, wi = wso.eval(p, w, q)
        assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64))
        assert np.array_equal(gg.view(np.uint64), wg.view(np.uint64))
        assert np.array_equal(gi, wi)
        if extra:
            assert (wi == 1).any() and (wi == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("single", [0, 1])
def test_sample_distance_and_transmittance(pkg, wso, ctx, single):
    rays = ws_oracle.make_rays(pkg, 48, seed=100 + CTXS.index(ctx) + 10 * single)
    rays["first_scatter"][::3] = 0
    for normal in (0, 1):
        m, p, w = _medium(pkg, ctx=ctx, single=single, normal=normal)
        got = m.sample_distance(rays)
        want, _ = wso.sample_distance(p, w, rays)
        _same_seg(got, want)
        assert (want["exited"] == 0).sum() > 10
        vis = m.transmittance(rays)
        vis_want, _ = wso.transmittance(p, w, rays)
        assert np.array_equal(vis, vis_want)
        # the device-pointer entries equal the host entries
        _same_seg(m.sample_distance_batch(rays), got)
        assert np.array_equal(m.transmittance_batch(rays), vis)
        m.close()


@pytest.mark.gpu
def test_sample_distance_edge_cases(pkg, wso):
    m, p, w = _medium(pkg, ctx="renewal", n_basis=64, mean_additional=True)
    rays = ws_oracle.make_rays(pkg, 12, seed=7)
    rays["far_t"][0] = 0.0                                   # maxT == 0
    rays["far_t"][1:4] = np.inf                              # clamped to near + 2000
    rays["dir"][3] = (0.0, 1.0, 0.0)                         # ... and a miss: the whole 2000 units
    rays["bounce"][4] = p["max_bounces"]                     # bounce cap
    rays["first_scatter"][5:7] = 0                           # the step == 1 rule
    rays["pos"][7] = (0.0, 0.0, 0.5)                         # a start inside the surface
    rays["near_t"][8] = 1.5                                  # near > 0
    out = m.sample_distance(rays)
    want, _ = wso.sample_distance(p, w, rays)
    _same_seg(out, want)
    assert want["ok"][4] == 0 and want["exited"][0] == 1 and want["exited"][3] == 1
    m.close()


@pytest.mark.gpu
def test_refinement_collapse(pkg, wso):
    """The refinement of WSM:262-283 collapses to t = 0 when every candidate keeps the new sign down to intp_factor <= 0.01: a
    start in the 1e-4 gap between two spheres of the CSG mean, marching into the first (the candidates lie behind the start, in the
    second).  With no basis functions the field is the mean alone."""
    m, p, w = None, *ws_oracle.ws_params(pkg, ctx="none", n_basis=0)
    p["has_mean_additional"] = 1
    p["mean_additional"]["type"] = 1
    p["mean_additional"]["center"] = (0.0, 0.0, 2.5)
    p["mean_additional"]["radius"] = 1.4998
    m = pkg.WeightSpaceMedium(p, w)
    rays = ws_oracle.make_rays(pkg, 4, seed=3)
    rays["pos"] = (0.0, 0.0, 1.0001)
    rays["dir"] = (0.0, 0.0, -1.0)
    rays["far_t"] = 3.0
    rays["u_jitter"] = (0.5, 0.25, 0.75, 0.1)
    out = m.sample_distance(rays)
    want, _ = wso.sample_distance(p, w, rays)
    _same_seg(out, want)
    assert (want["t"] == 0.0).all() and (want["exited"] == 0).all()
    m.close()


@pytest.mark.gpu
def test_min_step_zero(pkg, wso):
    """min_step 0 is the reference's (far - near) / 0.0f: +inf (the step is step_size), or NaN when near == far (no march)."""
    m, p, w = None, *ws_oracle.ws_params(pkg, ctx="renewal", n_basis=64)
    p["min_step"] = 0
    m = pkg.WeightSpaceMedium(p, w)
    rays = ws_oracle.make_rays(pkg, 16, seed=21)
    rays["near_t"][3] = rays["far_t"][3] = 1.5
    out = m.sample_distance(rays)
    _same_seg(out, wso.sample_distance(p, w, rays)[0])
    assert (out["exited"] == 0).sum() > 5 and out["exited"][3] == 1
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ramp_type", [0, 1, 2, 3])
def test_ramp_colour_weight(pkg, wso, ramp_type):
    """The mean's "color" ramp scales the weight of a hit (GPM.cpp:316)."""
    m, p, w = None, *ws_oracle.ws_params(pkg, ctx="none", n_basis=65)
    c = p["mean_color"]
    c["enabled"], c["type"] = 1, ramp_type
    c["min"], c["max"], c["start"], c["end"] = 0.2, 0.9, -1.0, 1.0
    c["min2"], c["max2"], c["start2"], c["end2"] = 0.1, 0.6, -0.8, 0.5
    m = pkg.WeightSpaceMedium(p, w)
    rays = ws_oracle.make_rays(pkg, 32, seed=30 + ramp_type)
    out = m.sample_distance(rays)
    want, _ = wso.sample_distance(p, w, rays)
    _same_seg(out, want)
    hit = (want["exited"] == 0) & (want["ok"] == 1)
    assert hit.sum() > 5 and len(np.unique(want["weight"][hit, 0])) > 3
    m.close()


@pytest.mark.gpu
def test_range_flag_counts_only_kept_points(pkg, wso):
    """A march whose discarded speculative points lie beyond the restated cos range, while every point the serial loop evaluates
    lies inside it, is not an error.  One basis function along the ray, a linear mean that changes sign a few steps before the
    argument reaches 105414350, tiny noise."""
    import struct
    p, w = ws_oracle.ws_params(pkg, ctx="none", single=1, n_basis=1, sigma=1e-6)
    b = wso.basis(p, w, np.zeros((1, 4), dtype=np.uint32))[0, 0]          # d.x, d.y, d.z, omega, phi, w of the one function
    d, om, ph = b[:3], float(b[3]), float(b[4])
    T = struct.unpack("<d", struct.pack("<Q", 0x419921FB00000000))[0]    # smallest |x| cos_glibc does not restate
    step = np.float32(0.01)
    ts, t = [], float(np.float32(0.0) + step * np.float32(0.5))       # the march positions (near 0, jitter 0.5)
    while t < 3.0:
        ts.append(t)
        t += float(step)

    def batch(i):                                        # the speculative batch position i is evaluated in (the first holds f0)
        return 0 if i < 31 else 1 + (i - 31) // 32

    rays = ws_oracle.make_rays(pkg, 1, seed=5)
    rays["dir"] = d
    rays["near_t"], rays["far_t"], rays["u_jitter"] = 0.0, 3.0, 0.5
    rd = rays[0]["dir"].astype(np.float64)
    for shift in np.linspace(-1.0, 0.0, 11):            # where the argument crosses T: about one unit along the ray
        rays["pos"] = d * ((T - ph) / om - 1.0 + shift)
        p0 = rays[0]["pos"].astype(np.float64)
        args = [((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]) * om + ph for q in (p0 + tt * rd for tt in ts)]
        k0 = next(i for i, a in enumerate(args) if a >= T)                # first march position beyond the range
        if 40 < k0 and batch(k0) == batch(k0 - 1):
            break
    else:
        pytest.fail("no ray puts the range boundary inside one batch")
    t_star = 0.5 * (ts[k0 - 2] + ts[k0 - 1])               # the sign change: the hit is position k0 - 1, inside the range
    p["mean"]["type"] = 2
    p["mean"]["center"] = p0 + t_star * rd
    p["mean"]["dir"] = -rd
    p["mean"]["scale"] = 1.0
    m = pkg.WeightSpaceMedium(p, w)
    out = m.sample_distance(rays)                          # raised GPIS_ERR_UNSUPPORTED when discarded points counted
    want, _ = wso.sample_distance(p, w, rays)
    _same_seg(out, want)
    assert want["exited"][0] == 0 and ts[k0 - 2] <= want["t"][0] <= ts[k0 - 1]
    c = m.counters()
    assert c["n_spec"] > c["n_eval"]                       # the positions past the hit were evaluated, and dropped
    m.close()


@pytest.mark.gpu
def test_absorption_only(pkg, wso):
    m, p, w = _medium(pkg, ctx="renewal_plus", absorption_only=True)
    rays = ws_oracle.make_rays(pkg, 32, seed=11)
    _same_seg(m.sample_distance(rays), wso.sample_distance(p, w, rays)[0])
    m.close()


@pytest.mark.gpu
def test_counters(pkg, wso):
    m, p, w = _medium(pkg, ctx="renewal")
    rays = ws_oracle.make_rays(pkg, 64, seed=12)
    m.reset_counters()
    m.sample_distance(rays)
    c = m.counters()
    _, n_eval = wso.sample_distance(p, w, rays)
    assert c["n_seg"] == 64 and c["n_eval"] == n_eval and c["n_spec"] >= n_eval
    m.close()


@pytest.mark.gpu
def test_handles_are_not_interchangeable(pkg):
    L = pkg.load_library()
    ws, _, _ = _medium(pkg)
    sc = pkg.Medium(pkg.params_for_config("C0"))
    rays = ws_oracle.make_rays(pkg, 2)
    out = np.zeros(2, dtype=pkg.SEG_OUT)
    vis = np.zeros(2, dtype=np.uint8)
    assert L.lib.gpis_sample_distance_host(ws.h, 2, rays.ctypes.data, out.ctypes.data, None) == -1
    assert L.lib.gpis_transmittance_batch(ws.h, 2, rays.ctypes.data, vis.ctypes.data, None) == -1
    assert L.lib.gpis_fs_sample_distance_host(ws.h, 0, None, None, None) == -1
    assert L.lib.gpis_get_derived(ws.h, np.zeros((), dtype=pkg.DERIVED).ctypes.data) == -1
    assert L.lib.gpis_ws_sample_distance_host(sc.h, 2, rays.ctypes.data, out.ctypes.data) == -1
    assert L.lib.gpis_ws_transmittance_host(sc.h, 2, rays.ctypes.data, vis.ctypes.data) == -1
    ws.close()
    sc.close()


@pytest.mark.gpu
def test_refused_configurations_on_device(pkg):
    L = pkg.load_library()
    for mod in ("step", "matern", "beckmann", "ggx", "mean"):
        p, w = ws_oracle.ws_params(pkg)
        if mod == "step":
            p["step_size"] = 0
        elif mod == "matern":
            p["kernel_type"] = 1
        elif mod in ("beckmann", "ggx"):
            w["normal_method"] = 2 if mod == "beckmann" else 3
        else:
            w["intersect_method"] = 1
        h = ctypes.c_void_p()
        assert L.lib.gpis_ws_create(p.ctypes.data, w.ctypes.data, 0, ctypes.byref(h)) == -2, mod


@pytest.mark.gpu
def test_argument_beyond_restated_range_is_an_error(pkg):
    m, p, w = _medium(pkg, ctx="renewal", n_basis=8)
    q = ws_oracle.make_queries(pkg, 2)
    q["p"][1] = (3e9, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="105414350"):
        m.eval(q)
    q["p"][1] = (0.1, 0.0, 0.0)
    m.eval(q)                                     # the flag was consumed: the next call is clean
    m.close()


@pytest.mark.gpu
def test_fixture(pkg):
    g = np.load(GOLD)
    for k in range(int(g["n_cases"])):
        p = np.array(g["params_%d" % k]).view(pkg.PARAMS).reshape(())
        w = np.array(g["ws_%d" % k]).view(pkg.WS_PARAMS).reshape(())
        m = pkg.WeightSpaceMedium(p, w)
        rays = np.ascontiguousarray(g["rays_%d" % k]).view(pkg.RAY_IN).reshape(-1)
        _same_seg(m.sample_distance(rays), np.ascontiguousarray(g["out_%d" % k]).view(pkg.SEG_OUT).reshape(-1))
        assert np.array_equal(m.transmittance(rays), g["vis_%d" % k])
        q = np.ascontiguousarray(g["queries_%d" % k]).view(pkg.WS_QUERY).reshape(-1)
        v, gr, i = m.eval(q)
        assert np.array_equal(v, g["value_%d" % k]) and np.array_equal(gr, g["grad_%d" % k]) and np.array_equal(i, g["id_%d" % k])
        assert np.array_equal(m.basis(g["pss_%d" % k]), g["basis_%d" % k])
        m.close()
