"""Randomised weight-space media on the device.  The fixed cases of test_gpu_ws.py share one C0-like parameter block; here seeded
random blocks (context, single / per-path, normal method, basis size, seed, sigma, length scale, anisotropy, step sizes, means
incl. linear, homogeneous and CSG pairs, medium coefficients, colour ramps) and rays of every kind (inside starts as continued
paths, near_t > 0, far_t 0 / inf / == near_t) go through every entry, bit for bit against the plain-C restatement
(tests/native/ws_oracle.c).  tests/test_ws_fuzz_cpu.py checks on the CPU that no case is vacuous and none is skipped.

Independently of the restatement, the device's field values and gradients are measured against the formula itself, evaluated
with mpmath from the device's own exported basis, under a derived rounding bound (ws_oracle.ExactField)."""
import os

import numpy as np
import pytest

import ws_oracle
from test_gpu_ws import _same_seg

pytestmark = pytest.mark.gpu

FIRST = int(os.environ.get("GPIS_FUZZ_FIRST", "0"))
SEEDS = range(FIRST, FIRST + int(os.environ.get("GPIS_FUZZ_SEEDS", str(ws_oracle.FUZZ_DEFAULT_SEEDS))))


@pytest.fixture(scope="module")
def wso():
    return ws_oracle.WsOracle()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_configuration(pkg, wso, seed):
    p, w, pss, q, rays = ws_oracle.fuzz_case(pkg, seed)
    m = pkg.WeightSpaceMedium(p, w)
    got_b, want_b = m.basis(pss), wso.basis(p, w, pss)
    assert got_b.shape == want_b.shape and np.array_equal(got_b.view(np.uint64), want_b.view(np.uint64)), seed
    gv, gg, gi = m.eval(q)
    wv, wg, wi = wso.eval(p, w, q)
    assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)), seed
    assert np.array_equal(gg.view(np.uint64), wg.view(np.uint64)), seed
    assert np.array_equal(gi, wi), seed
    m.reset_counters()
    got = m.sample_distance(rays)
    c_sd = m.counters()
    vis = m.transmittance(rays)
    c_tr = m.counters()
    want, e_sd = wso.sample_distance(p, w, rays)
    vis_want, e_tr = wso.transmittance(p, w, rays)
    print("seed", seed, ws_oracle.describe(p, w), "hits", int((want["exited"] == 0).sum()), "blocked", int((vis_want == 0).sum()),
          "n_eval", e_sd, e_tr)
    _same_seg(got, want)
    assert np.array_equal(vis, vis_want), seed
    assert c_sd["n_eval"] == e_sd and c_tr["n_eval"] == e_sd + e_tr, (seed, c_sd, c_tr, e_sd, e_tr)
    assert c_tr["n_seg"] == 2 * len(rays) and c_tr["n_spec"] >= c_tr["n_eval"]
    # the device-pointer entries
    _same_seg(m.sample_distance_batch(rays), want)
    assert np.array_equal(m.transmittance_batch(rays), vis_want), seed
    m.close()


@pytest.mark.parametrize("case", sorted(ws_oracle.EXACT_CASES))
def test_device_field_against_the_formula(pkg, case):
    """Restatement and kernel share an author and a reading of the reference; this check shares neither.  The device exports its
    own basis (gpis_ws_basis_batch); f(p) = sqrt(sigma^2) sqrt(2 / N) sum_i w_i cos(omega_i d_i.p + phi_i) + mean(p), its analytic
    gradient (conditioned-Gaussian normals) and its central difference with eps = 1e-4 (finite differences) are evaluated from
    that basis with mpmath at 60 digits and compared with gpis_ws_eval_batch.

    The tolerance is derived per query (ws_oracle.ExactField.bound), with u = 2^-53:
        bound = scale sqrt(2 / N) sum_i |w_i| ((N + 4) u + 4 u (|omega_i| |d_i| |p| + |phi_i|)) + 4 u |mean(p)|
    (N + 4) u: the N - 1 additions of the sum whatever their order, the product with w_i, the cos (below one ulp) and the two
    final products, to first order; 4 u (|omega| |d| |p| + |phi|): the rounding of the argument (three products and two sums of
    the dot, the product with omega, the sum with phi), which |cos'| <= 1 passes on unamplified; 4 u |mean(p)|: the mean.  The
    gradient's bound has |w_i omega_i| for |w_i|; the finite-difference gradient adds (bound_f(p + e) + bound_f(p - e)) / (2 eps).
    The exact central difference is taken at the device's own six points (the IEEE sums p +- eps e_c), so the truncation term
    eps^2 / 6 sum_i |w_i| omega_i^3 scale sqrt(2 / N) of a comparison with the derivative is not needed and the bound is that much
    smaller.  The conditioned-Gaussian gradient passes through the reference's shell-embedding Jacobian, which its rounded
    p_c + eps puts about 1e-12 from the identity; ExactField.check explains how the exact value accounts for it.  Each value's
    bound must itself be small: bound <= 1e-9 max(1, |f|)."""
    p, w, q = ws_oracle.exact_case(pkg, case)
    m = pkg.WeightSpaceMedium(p, w)
    v, g, _ = m.eval(q)
    basis = m.basis(np.stack([q["pixel"][:, 0], q["pixel"][:, 1], q["spp"], q["segment"]], 1))
    m.close()
    assert basis.shape == (len(q), int(w["basis_functions"]), 6)
    figures = [ws_oracle.ExactField(pkg, p, basis[k]).check(q["p"][k], v[k], g[k], int(w["normal_method"])) for k in range(len(q))]
    print(case, "largest value error %.3g (bound %.3g), largest gradient error / bound %.3f"
          % (max(f[0] for f in figures), max(f[1] for f in figures), max(f[2] for f in figures)))
