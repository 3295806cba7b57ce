"""CPU checks of the weight-space GP medium: the C restatement (tests/native/ws_oracle.c) against the reference's primitives and
against GP theory, the ABI mirror of gpis_ws_params, the exported gpis_ws_* symbols and the refusals of gpis_ws_create (which are
decided before any device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ws_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.skipif(not ws_oracle.available(), reason="no C compiler for the restatement")


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as g
    g.build_hip()
    return pkg.load_library()


def test_restatement_primitives_match_reference(wso):
    g = np.load(os.path.join(GOLD, "ref_primitives.npz"))
    assert np.array_equal(wso.xxhash32_4(g["hash4_in"]), g["hash4_out"])
    assert np.array_equal(wso.pcg32_stream(g["pcg_state"], g["pcg_stream"].shape[1]), g["pcg_stream"])
    for i, s in enumerate(g["pcg_state"]):
        assert np.array_equal(wso.box_muller(s, 4), g["box_muller"][i])


def test_restatement_statistics_match_theory(wso, pkg):
    """Per-path realizations at N = 300: mean and covariance of the field over 4096 realizations against the squared-exponential
    prior sigma^2 exp(-d^T diag(aniso) d / (2 l^2)) and the analytic mean, within 4 standard errors."""
    aniso = (1.0, 0.5, 2.0)
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", sigma=0.7, length_scale=0.3, aniso=aniso)
    R = 4096
    p0 = np.array([0.2, -0.1, 0.4])
    offsets = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 0.15], [0.2, -0.1, 0.3]])
    pts = np.concatenate([[p0], p0 + offsets[1:]])
    q = np.zeros(R * len(pts), dtype=pkg.WS_QUERY)
    q["p"] = np.tile(pts, (R, 1))
    q["pixel"][:, 0] = np.repeat(np.arange(R), len(pts))
    q["spp"] = 3
    v, _, _ = wso.eval(p, w, q)
    v = v.reshape(R, len(pts))
    mean = np.array([np.linalg.norm(x) - 1.0 for x in pts])
    f = v - mean
    for k in range(len(pts)):                    # E f = mean
        se = f[:, k].std(ddof=1) / np.sqrt(R)
        assert abs(f[:, k].mean()) < 4 * se, (k, f[:, k].mean(), se)
    s2, l2 = np.float32(0.7) ** 2, np.float32(0.3) ** 2
    for k, d in enumerate(offsets):              # E f(p0) f(p0 + d) = k(d)
        prod = f[:, 0] * f[:, k]
        want = float(s2) * np.exp(-(d * np.array(aniso)) @ d / (2 * float(l2)))
        se = prod.std(ddof=1) / np.sqrt(R)
        assert abs(prod.mean() - want) < 4 * se, (k, prod.mean(), want, se)


def test_restatement_realization_rules(wso, pkg):
    """single_realization ignores pss; GLOBAL drops the segment word; the other contexts draw per segment."""
    pss = np.array([[3, 4, 5, 0], [3, 4, 5, 2], [9, 9, 9, 9]], dtype=np.uint32)
    p, w = ws_oracle.ws_params(pkg, ctx="global", n_basis=17)
    b = wso.basis(p, w, pss)
    assert np.array_equal(b[0], b[1]) and not np.array_equal(b[0], b[2])
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", n_basis=17)
    b = wso.basis(p, w, pss)
    assert not np.array_equal(b[0], b[1])
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", single=1, n_basis=17)
    b = wso.basis(p, w, pss)
    assert np.array_equal(b[0], b[2])
    assert np.allclose(np.linalg.norm(b[0][:, :3], axis=1), 1.0)


def test_ws_params_size_matches_c(lib, pkg, wso):
    got = dict(kv.split("=") for kv in lib.lib.gpis_abi_sizes().decode().split(","))
    assert int(got["gpis_ws_params"]) == pkg.WS_PARAMS.itemsize == wso.lib.ws_oracle_sizes(0)
    assert int(got["gpis_ws_query"]) == pkg.WS_QUERY.itemsize == wso.lib.ws_oracle_sizes(1)
    w = np.zeros((), dtype=pkg.WS_PARAMS)
    lib.lib.gpis_ws_default_params(w.ctypes.data)
    assert w == pkg.default_ws_params()


def test_library_exports_every_ws_symbol(lib):
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s*(gpis_ws_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert len(declared) >= 10
    for name in sorted(declared):
        assert hasattr(lib.lib, name), name
        assert name in lib.SYMBOLS, name


@pytest.mark.parametrize("what", ["step_size_zero", "matern", "gabor", "nonstationary", "grid", "beckmann", "ggx", "intersect_mean",
                                  "too_many_basis"])
def test_refused_configurations(lib, pkg, what):
    p, w = ws_oracle.ws_params(pkg)
    if what == "step_size_zero":
        p["step_size"] = 0.0
    elif what == "matern":
        p["kernel_type"] = 1
    elif what == "gabor":
        p["kernel_type"] = 2
    elif what == "nonstationary":
        p["nonstationary"] = 1
    elif what == "grid":
        p["nonstationary"], p["grid_nonstationary"] = 1, 1
    elif what == "beckmann":
        w["normal_method"] = pkg.NORMAL.BECKMANN
    elif what == "ggx":
        w["normal_method"] = pkg.NORMAL.GGX
    elif what == "intersect_mean":
        w["intersect_method"] = pkg.INTERSECT.MEAN
    elif what == "too_many_basis":
        w["basis_functions"] = pkg.WS_MAX_BASIS + 1
    h = ctypes.c_void_p()
    rc = lib.lib.gpis_ws_create(p.ctypes.data, w.ctypes.data, 0, ctypes.byref(h))
    assert rc == -2 and not h.value, (rc, lib.last_error())      # GPIS_ERR_UNSUPPORTED, with its reason
    assert lib.last_error()


def test_ws_entries_refuse_null_and_foreign_handles(lib):
    """Null handles, and stand-ins for the two handle families: memory whose first word is gpis_params::abi_version (what a
    sparse-convolution handle starts with) or the weight-space tag.  Each family's entries look at that word only, so the
    stand-ins are refused before anything else of them is read."""
    L = lib.lib
    assert L.gpis_ws_sample_distance_host(None, 0, None, None) == -1
    assert L.gpis_ws_eval_batch(None, 0, None, None, None, None, None) == -1
    sc_like = np.zeros(64, dtype=np.uint32)
    sc_like[0] = 3                                      # GPIS_ABI_VERSION
    ws_like = np.zeros(64, dtype=np.uint32)
    ws_like[0] = 0x57534D31                             # kWsHandleTag
    sc, ws = ctypes.c_void_p(sc_like.ctypes.data), ctypes.c_void_p(ws_like.ctypes.data)
    assert L.gpis_ws_sample_distance_host(sc, 0, None, None) == -1
    assert L.gpis_ws_transmittance_batch(sc, 0, None, None, None) == -1
    assert L.gpis_ws_basis_batch(sc, 0, None, None, None) == -1
    assert L.gpis_ws_reset_counters(sc) == -1
    assert L.gpis_sample_distance_batch(ws, 0, None, None, None, None) == -1
    assert L.gpis_transmittance_host(ws, 0, None, None) == -1
    assert L.gpis_fs_sample_distance_batch(ws, 0, None, None, None, None) == -1
    assert L.gpis_get_counters(ws, None, None) == -1
    assert L.gpis_get_derived(ws, np.zeros(1, dtype=np.uint8).ctypes.data) == -1
    assert "handle" in lib.last_error() or "invalid" in lib.last_error()
