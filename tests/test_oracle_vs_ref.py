"""Pins the oracle's integer layer, ONB, Box–Muller and Eigen expression forms BIT-EXACTLY against
the real reference: tests/golden/ref_pins.npz holds the inputs and the outputs of the reference's own
primitives compiled in place (oracle/_ref/libgpis_ref.so, built from the reference's src/core headers +
sampling/Gaussian.cpp by oracle/Makefile; generator: tests/golden/make_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

f32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.npz")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def libs(ob):
    return ob.oracle_lib(), dict(np.load(GOLD)), ob


def test_xxhash32_all_arities(libs):
    orc, g, ob = libs
    for arity in (1, 2, 3, 4):
        assert np.array_equal(ob.xxhash32(g["xxhash%d_in" % arity]), g["xxhash%d_out" % arity])
    # known answer recorded from the reference run in SURVEY.md §8c
    assert int(ob.xxhash32(np.array([[1, 2, 3, 4]], dtype=np.uint32))[0]) == 2694834884


def test_pcg32_stream_and_float(libs):
    orc, g, ob = libs
    got = ob.pcg32_stream(g["pcg_state"], 64)
    assert np.array_equal(got, g["pcg_stream"])
    for v, want in zip(g["normalized_uint_in"], g["normalized_uint_out"]):
        assert f32(orc.oracle_normalized_uint(ctypes.c_uint32(int(v)))) == want
    for rv, b in zip(g["bernoulli_in"], g["bernoulli_out"]):
        assert b == (-1.0 if f32(rv) < f32(0.5) else 1.0)


def test_cell3d_draw_order(libs):
    """next3D() = Vec3f(next1D(), next1D(), next1D()): g++ evaluates right-to-left, so the first
    draw is z (UniformSampler.hpp:59-61 as compiled by this image's g++ 11.4)."""
    orc, g, ob = libs
    for state, b in zip(g["cell3d_state"], g["cell3d_draws"]):
        a = np.zeros(4 * 32, dtype=f32)
        orc.oracle_cell3d_draws(ctypes.c_uint64(int(state)), 32, P(a))
        assert np.array_equal(a, b)
    raw = ob.pcg32_stream(np.array([12345], dtype=np.uint64), 4)[0]
    u = [f32(orc.oracle_normalized_uint(ctypes.c_uint32(int(r)))) for r in raw]
    d = np.zeros(4, dtype=f32)
    orc.oracle_cell3d_draws(ctypes.c_uint64(12345), 1, P(d))
    assert (d[2], d[1], d[0], d[3]) == (u[0], u[1], u[2], u[3])


def test_tangent_frame_and_vec(libs):
    orc, g, ob = libs
    for i, (n, p) in enumerate(zip(g["frame_n"], g["frame_p"])):
        a = np.zeros(9, dtype=f32)
        orc.oracle_tangent_frame(P(n), P(a))
        assert np.array_equal(a, g["frame_tangent_frame"][i]), n
        for fn in ("frame_to_local", "frame_to_global"):
            x = np.zeros(3, dtype=f32)
            getattr(orc, "oracle_" + fn)(P(n), P(p), P(x))
            assert np.array_equal(x, g["frame_" + fn][i])
        x = np.zeros(3, dtype=f32)
        orc.oracle_vec3_normalized(P(n), P(x))
        assert np.array_equal(x, g["frame_vec3_normalized"][i])


def test_box_muller(libs):
    orc, g, ob = libs
    for i, state in enumerate(g["box_muller_state"]):
        a = np.zeros(8)
        orc.oracle_sample_standard_normal2(ctypes.c_uint64(int(state)), 4, P(a))
        assert np.array_equal(a, g["box_muller_normal2"][i])
        a = np.zeros(2)
        orc.oracle_sample_xy_over_sqrt2(ctypes.c_uint64(int(state)), P(a))
        assert np.array_equal(a, g["box_muller_xy_over_sqrt2"][i])


def test_eigen_expression_forms(libs):
    orc, g, ob = libs
    assert len(g["eig_in_M"]) == 1500
    for it in range(len(g["eig_in_M"])):
        ab, M, B = (np.ascontiguousarray(g["eig_in_" + k][it]) for k in ("ab", "M", "B"))
        s = ctypes.c_float(float(g["eig_in_s"][it]))
        want = lambda k: g["eig_" + k][it]      # noqa: E731
        assert f32(orc.oracle_eig_dist2_ab(P(ab), P(M))) == want("dist2_ab")
        for c in range(3):
            assert f32(orc.oracle_eig_dot_col(P(ab), P(M), c)) == want("dot_col")[c]
        for fn in ("matvec_div", "matvec_mul"):
            x = np.zeros(3, dtype=f32)
            getattr(orc, "oracle_eig_" + fn)(P(M), P(ab), s, P(x))
            assert np.array_equal(x, want(fn))
        x = np.zeros(3, dtype=f32)
        orc.oracle_eig_matvec(P(M), P(ab), P(x))
        assert np.array_equal(x, want("matvec"))
        for fn in ("inverse3", "second_deriv_inv"):
            x = np.zeros(9, dtype=f32)
            getattr(orc, "oracle_eig_" + fn)(P(M), P(x))
            assert np.array_equal(x, want(fn)), (fn, M)
        x = np.zeros(9, dtype=f32)
        orc.oracle_eig_scaled_matmul(ctypes.c_float(0.37), P(M), P(B), P(x))
        assert np.array_equal(x, want("scaled_matmul"))
        x = np.zeros(9, dtype=f32)
        dx = ctypes.c_float()
        orc.oracle_eig_gram(P(M), P(x), ctypes.byref(dx))
        assert np.array_equal(x, want("gram")) and f32(dx.value) == want("gram_det")
        a1, a2 = np.zeros(9, dtype=f32), np.zeros(9, dtype=f32)
        orc.oracle_eig_scale_and_inverse(ctypes.c_float(0.0354), P(M), P(a1), P(a2))
        assert np.array_equal(a1, want("scale_and_inverse")[0]) and np.array_equal(a2, want("scale_and_inverse")[1])
        for is_cov in (0, 1):
            x = np.zeros(9, dtype=f32)
            orc.oracle_eig_invcov_scale(P(M), ctypes.c_float(1.7), ctypes.c_float(0.6), is_cov, P(x))
            assert np.array_equal(x, want("invcov_scale")[is_cov])


def test_fresnel_and_mis_weights(libs):
    """Arithmetic of the conductor NEE estimator against the reference's own
    Fresnel.hpp / SampleWarp.hpp."""
    orc, g, ob = libs
    for n in ("oracle_conductor_reflectance", "oracle_power_heuristic", "oracle_spherical_cap_pdf"):
        fn = getattr(orc, n)
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float] * (3 if "reflectance" in n else (2 if "heuristic" in n else 1))
    bits = lambda v: np.float32(v).view(np.uint32)      # noqa: E731
    assert len(g["fresnel_in"]) == 5 * 405
    for (eta, k, c), want in zip(g["fresnel_in"], g["fresnel_out"]):
        assert bits(orc.oracle_conductor_reflectance(float(eta), float(k), float(c))) == bits(want), (eta, k, c)
    for (a, b), want in zip(g["power_heuristic_in"], g["power_heuristic_out"]):
        assert bits(orc.oracle_power_heuristic(float(a), float(b))) == bits(want)
    for c, want in zip(g["cap_pdf_in"], g["cap_pdf_out"]):
        assert bits(orc.oracle_spherical_cap_pdf(float(c))) == bits(want)
