"""CPU side of the weight-space fuzz (tests/test_gpu_ws_fuzz.py): the generator of tests/ws_oracle.py draws only blocks the
restatement and gpis_ws_create accept, no fuzz batch is vacuous, the default seed list covers every configuration class, and the
high-precision formula the GPU module measures the device against agrees with the restatement first."""
import ctypes
import os

import numpy as np
import pytest

import ws_oracle

pytestmark = pytest.mark.skipif(not ws_oracle.available(), reason="no C compiler for the restatement")

FIRST = int(os.environ.get("GPIS_FUZZ_FIRST", "0"))
SEEDS = list(range(FIRST, FIRST + int(os.environ.get("GPIS_FUZZ_SEEDS", str(ws_oracle.FUZZ_DEFAULT_SEEDS)))))
_RESULTS = {}


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


def _run(pkg, wso, seed):
    """the restatement's results of fuzz case `seed` (cached: the per-seed test and the coverage test share them)"""
    if seed not in _RESULTS:
        p, w, pss, q, rays = ws_oracle.fuzz_case(pkg, seed)
        out, _ = wso.sample_distance(p, w, rays)             # raises on a block outside the restatement: zero skips
        vis, _ = wso.transmittance(p, w, rays)
        _RESULTS[seed] = (p, w, out, vis, rays)
    return _RESULTS[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_case_is_accepted_and_not_vacuous(pkg, wso, seed):
    p, w, out, vis, rays = _run(pkg, wso, seed)
    print("seed", seed, ws_oracle.describe(p, w), "exits", int((out["exited"] != 0).sum()), "hits ok", int(((out["exited"] == 0) & (out["ok"] == 1)).sum()),
          "blocked", int((vis == 0).sum()), "visible", int((vis != 0).sum()))
    assert (out["exited"] != 0).any()
    if not ws_oracle.absorption_only(p):
        assert ((out["exited"] == 0) & (out["ok"] == 1)).any()
    # the first three rays are visible by construction (far_t 0, an empty segment) or by luck: count real segments only
    real = rays["far_t"] > rays["near_t"]
    assert (vis[real] == 0).any() and (vis[real] != 0).any(), (int((vis[real] == 0).sum()), int((vis[real] != 0).sum()))


def test_default_seed_list_covers_every_class(pkg, wso):
    seen = set()
    for seed in range(ws_oracle.FUZZ_DEFAULT_SEEDS):
        p, w = ws_oracle.fuzz_case(pkg, seed)[:2]
        seen |= ws_oracle.fuzz_classes(pkg, p, w)
    assert seen >= ws_oracle.FUZZ_CLASSES, sorted(ws_oracle.FUZZ_CLASSES - seen)


def test_fuzz_blocks_pass_the_library_validation(pkg):
    """gpis_ws_create decides its refusals before it looks for a device: without one a valid block ends in GPIS_ERR_NO_DEVICE (or
    in a handle, on a GPU machine), never in INVALID_ARG / UNSUPPORTED."""
    import __graft_entry__ as g
    g.build_hip()
    L = pkg.load_library()
    for seed in range(ws_oracle.FUZZ_DEFAULT_SEEDS):
        p, w = ws_oracle.fuzz_case(pkg, seed)[:2]
        h = ctypes.c_void_p()
        rc = L.lib.gpis_ws_create(p.ctypes.data, w.ctypes.data, 0, ctypes.byref(h))
        assert rc not in (-1, -2), (seed, rc, L.last_error())
        if rc == 0:
            L.lib.gpis_destroy(h)


def test_argument_range_of_the_generators(pkg, wso):
    """the generators' comment: no cos argument comes near 105414350"""
    worst = 0.0
    for seed in range(ws_oracle.FUZZ_DEFAULT_SEEDS):
        p, w, pss, q, rays = ws_oracle.fuzz_case(pkg, seed)
        if int(w["basis_functions"]) == 0:
            continue
        b = wso.basis(p, w, pss)
        reach = np.linalg.norm(rays["pos"].astype(np.float64), axis=1).max() + 2000.0
        worst = max(worst, float((np.abs(b[..., 3]) * reach + np.abs(b[..., 4])).max()))
    assert worst < 1e6, worst


@pytest.mark.parametrize("case", sorted(ws_oracle.EXACT_CASES))
def test_exact_formula_agrees_with_the_restatement(pkg, wso, case):
    """The formula's own implementation (ws_oracle.ExactField) against the restatement, under the bound the GPU test uses."""
    p, w, q = ws_oracle.exact_case(pkg, case)
    v, g, _ = wso.eval(p, w, q)
    pss = np.stack([q["pixel"][:, 0], q["pixel"][:, 1], q["spp"], q["segment"]], 1)
    basis = wso.basis(p, w, pss)
    figures = [ws_oracle.ExactField(pkg, p, basis[k]).check(q["p"][k], v[k], g[k], int(w["normal_method"])) for k in range(len(q))]
    print(case, "largest value error %.3g (bound %.3g), largest gradient error / bound %.3f"
          % (max(f[0] for f in figures), max(f[1] for f in figures), max(f[2] for f in figures)))
