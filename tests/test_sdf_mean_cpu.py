"""CPU checks of the procedural SDF mean's reference chain: tests/native/sdf_mean_ref.c (the tests' reference, a plain-C restatement)
against tests/golden/sdf_mean_pins.npz (values of the reference's own compiled SdfFunctions / Mat4f::rotAxis), the coverage
condition of the pin set, Mat4f::invert / transformPoint, and the ABI mirror.

Pinning status: the four SDF functions and rotAxis are pinned to the reference's compiled code.  Mat4f::invert / transformPoint are
header-only in the reference and oracle/_ref exports no symbol for them: restated, parity unpinned (checked here against double
arithmetic only).  The wrapper lines of ProceduralMean::mean / dmean_da cannot be compiled here (GPFunctions.hpp needs Boost):
restated, parity unpinned."""
import glob
import os
import re

import numpy as np
import pytest

import sdf_mean_ref
from golden import make_sdf_mean_golden as gen

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
FUNCS = ("knob", "knob_inner", "knob_outer", "two_spheres")

pytestmark = pytest.mark.skipif(not sdf_mean_ref.available(), reason="no C compiler for the restatement")


@pytest.fixture(scope="module")
def ref():
    return sdf_mean_ref.SdfMeanRef()


@pytest.fixture(scope="module")
def pins():
    return dict(np.load(os.path.join(GOLD, "sdf_mean_pins.npz")))


@pytest.mark.parametrize("func", FUNCS)
def test_restatement_equals_pins(ref, pins, func):
    got = ref.eval(func, pins["points"]).view(np.uint32)
    bad = np.nonzero(got != pins[func])[0]
    assert bad.size == 0, (func, bad[:8], pins["points"][bad[:8]])


def test_known_answers(ref):
    """the two values the reference's compiled knob returns (recorded when the pins were first taken)"""
    got = ref.eval("knob", [(0.9, 0.1, -0.2), (0, 0, 0)]).view(np.uint32)
    assert [int(v) for v in got] == [0x3E026B27, 0xBF19999A]
    p = np.array([(0.3, -0.25, 7.0), (1.0, 0.0, 2.0)], dtype=np.float32)
    assert np.array_equal(ref.eval("plane", p), p[:, 1])


def test_pin_points_cover_every_outcome(ref, pins):
    """every min / max of sdKnob, sdKnobOuter and sdBase takes both outcomes over the pin set, every clamp both ends and the interior"""
    assert pins["points"].shape[0] >= 2048 + 1024
    for func in ("knob", "knob_outer"):
        for name, hit in ref.trace(func, pins["points"]).items():
            assert all(hit), (func, name, hit)


def test_rot_axis_equals_pins(ref, pins):
    for a, want in zip(pins["rot_angles"], pins["rot_axis_x"]):
        assert np.array_equal(ref.rot_axis_x(float(a)).view(np.uint32), want[:3, :3])
        assert np.array_equal(want.view(np.float32)[3], [0, 0, 0, 1]) and np.array_equal(want.view(np.float32)[:3, 3], [0, 0, 0])


def test_live_against_reference_build(ref, pins):
    """the same comparison against oracle/_ref itself, on fresh points, where that library exists"""
    live = gen.RefSdf.load()
    if live is None:
        pytest.skip("oracle/_ref/libgpis_ref.so is not built here")
    rng = np.random.default_rng(77)
    p = np.concatenate([rng.uniform(-1.3, 1.3, (700, 3)), rng.normal(0, 20, (60, 3))]).astype(np.float32)
    for func in FUNCS:
        assert np.array_equal(ref.eval(func, p).view(np.uint32), live.eval(func, p).view(np.uint32)), func
    for a in gen.ROT_ANGLES:
        assert np.array_equal(ref.rot_axis_x(a).view(np.uint32), live.rot_axis_x(a)[:3, :3].view(np.uint32))


def test_mat4_invert_and_transform_point(ref):
    """Mat4f::invert (cofactors in float, a zero determinant -> identity) and transformPoint: parity unpinned, so checked against
    double arithmetic to float accuracy, and for the structure the reference's code has"""
    rng = np.random.default_rng(5)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    T = (np.array([[1, 0, 0, 0.3], [0, 1, 0, -0.2], [0, 0, 1, 0.1], [0, 0, 0, 1.0]]) @ rot @ np.diag([1.5, 0.75, 1.25, 1.0])).astype(np.float32)
    inv = ref.invert(T)
    assert inv.dtype == np.float32
    assert np.allclose(inv.astype(np.float64), np.linalg.inv(T.astype(np.float64)), rtol=0, atol=4e-6)
    assert np.array_equal(ref.invert(np.eye(4)), np.eye(4, dtype=np.float32))
    singular = np.array(T)
    singular[:, 1] = 0
    assert np.array_equal(ref.invert(singular), np.eye(4, dtype=np.float32))          # det == 0: Mat4f()
    p = rng.uniform(-2, 2, (64, 3)).astype(np.float32)
    got = ref.transform_point(inv, p)
    f = np.float32
    for k in range(3):      # a11*x + a12*y + a13*z + a14, left to right, each operation rounded to float
        want = f(f(f(f(inv[k, 0] * p[:, 0]) + f(inv[k, 1] * p[:, 1])) + f(inv[k, 2] * p[:, 2])) + inv[k, 3])
        assert np.array_equal(got[:, k], want)


def test_mean_wrapper_and_gradient(ref, pkg):
    """ProceduralMean::mean = max(min, sdf(T^-1 float(a)) * scale + offset) in float; dmean_da = one-sided differences with
    eps = double(0.001f), in the order a, +x, +y, +z; the CSG minimum picks the smaller mean and its slot's gradient"""
    p = pkg.default_params()
    p["mean"]["type"] = pkg.MEAN_TYPE.PROCEDURAL
    p["mean"]["func"] = pkg.SDF_FUNCTION.KNOB
    p["mean"]["scale"], p["mean"]["offset"], p["mean"]["min"] = 0.5, 0.01, -0.05
    rng = np.random.default_rng(11)
    a = rng.uniform(-1.1, 1.1, (300, 3))
    val, gid, grad = ref.mean(p, a)
    f = np.float32
    sd = ref.eval("knob", a.astype(f))
    want = np.maximum(f(-0.05), f(f(sd * f(0.5)) + f(0.01))).astype(np.float64)
    assert np.array_equal(val, want) and not gid.any()
    assert (val == np.float64(f(-0.05))).any() and (val > -0.04).any()
    eps = np.float64(f(0.001))
    for k in range(3):
        b = np.array(a)
        b[:, k] = b[:, k] + eps
        sdk = ref.eval("knob", b.astype(f))
        wk = np.maximum(f(-0.05), f(f(sdk * f(0.5)) + f(0.01))).astype(np.float64)
        assert np.array_equal(grad[:, k], (wk - want) / eps)
    # CSG: knob + sphere of radius 0.5 about (0.6, 0, 0)
    p["has_mean_additional"] = 1
    p["mean_additional"]["type"] = pkg.MEAN_TYPE.SPHERICAL
    p["mean_additional"]["radius"] = 0.5
    p["mean_additional"]["center"] = (0.6, 0.0, 0.0)
    v2, g2, d2 = ref.mean(p, a)
    sph = np.sqrt(((a - (0.6, 0, 0)) ** 2).sum(1)) - 0.5
    assert g2.any() and not g2.all()          # both slots are chosen somewhere
    assert np.array_equal(g2 == 1, sph < val) and np.allclose(v2, np.minimum(val, sph), rtol=0, atol=1e-15)
    assert np.array_equal(d2[g2 == 0], grad[g2 == 0])


def test_abi_mirror(pkg):
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    assert re.search(r"GPIS_MEAN_PROCEDURAL\s*=\s*3\b", header)
    names = re.search(r"typedef enum gpis_sdf_function \{(.*?)\}", header, flags=re.S).group(1)
    order = re.findall(r"GPIS_SDF_([A-Z_]+)", names)
    assert order == ["KNOB", "KNOB_INNER", "KNOB_OUTER", "TWO_SPHERES", "PLANE"]
    assert [getattr(pkg.SDF_FUNCTION, n) for n in order] == [0, 1, 2, 3, 4] and pkg.MEAN_TYPE.PROCEDURAL == 3
    assert re.search(r"#define GPIS_ABI_VERSION 3\b", header)
    assert pkg.MEAN.itemsize == 72 and pkg.MEAN.fields["func"][1] == 20 and pkg.MEAN.fields["center"][1] == 24
    # the word keeps its stored NAME "_pad" (the committed fixtures compare records by field name); "func" is its numpy title
    assert "_pad" in pkg.MEAN.names and "func" not in pkg.MEAN.names and pkg.MEAN.fields["_pad"][1] == 20
    q = pkg.default_params()
    q["mean_additional"]["func"] = 4
    assert int(q["mean_additional"]["_pad"]) == 4 and int(q["mean"]["_pad"]) == 0
    d = pkg.default_params()
    assert int(d["mean"]["func"]) == 0 and int(d["mean_additional"]["func"]) == 0


def test_committed_parameter_records_still_load(pkg):
    """gpis_mean._pad became `func` in the C header; the numpy mirror keeps the name and adds the title.  Every committed .npz that stores a parameter
    record must still convert to the PARAMS record with every field where it was."""
    seen = same = 0
    for path in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        g = np.load(path)
        if "params" not in g.files:
            continue
        raw = np.array(g["params"])
        if raw.dtype == np.uint8:
            p = raw.view(pkg.PARAMS).reshape(())
        else:
            p = pkg.as_params(raw).reshape(())         # what Medium() and the oracle do with a stored record
            if raw.dtype.itemsize == pkg.PARAMS.itemsize:      # the current layout under the old field name: every field where it was
                assert p == np.frombuffer(raw.tobytes(), dtype=pkg.PARAMS).reshape(()), path
                assert p == np.array(raw, dtype=pkg.PARAMS).reshape(()), path
                same += 1
        assert int(p["abi_version"]) == 3, path
        if not os.path.basename(path).startswith("sdf_mean"):          # older fixtures: an analytic mean, the former padding word zero
            assert 0 <= int(p["mean"]["type"]) <= 2 and int(p["mean"]["func"]) == 0, path
        seen += 1
    assert seen >= 5 and same >= 2


def test_analytic_means_of_the_restatement_equal_the_oracle(ref, pkg, ob):
    """The frozen oracle has no mean entry.  With sigma = 0 its evaluators return the mean alone: evaluate_value =
    float(double(0 * noise) + mean), evaluate_gradient = 0 * grad(noise) + float(dmean_da).  So the analytic branch of the C
    restatement (types 0-2, what gpis_mean_* is compared with on the device) is checked against the oracle here, CSG minimum included."""
    import sdf_march_ref as smr
    q = smr.queries(pkg, 257, 23, scale=1.4)
    pts = np.asarray(q["p"], dtype=np.float32).astype(np.float64)
    for typ in (pkg.MEAN_TYPE.HOMOGENEOUS, pkg.MEAN_TYPE.SPHERICAL, pkg.MEAN_TYPE.LINEAR, "csg"):
        p = pkg.params_for_config("C0")
        p["sigma"] = 0.0
        m = p["mean"]
        m["offset"], m["center"], m["radius"], m["dir"], m["scale"], m["min"] = 0.125, (0.1, -0.2, 0.05), 0.8, (0.3, 1.0, -0.2), 0.7, -0.3
        if typ == "csg":
            m["type"] = pkg.MEAN_TYPE.SPHERICAL
            p["has_mean_additional"] = 1
            a = p["mean_additional"]
            a["type"], a["center"], a["dir"], a["scale"] = pkg.MEAN_TYPE.LINEAR, (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 1.0
        else:
            m["type"] = typ
        orc = ob.Oracle(p, threads=4)
        val, gid = orc.eval_value(q)
        grad = orc.eval_gradient(q)
        wv, wi, wg = ref.mean(p, pts)
        assert np.isfinite(val).all() and np.isfinite(grad).all()
        assert np.array_equal(val.view(np.uint32), wv.astype(np.float32).view(np.uint32)), typ
        assert np.array_equal(gid, wi), typ
        if typ == "csg":
            assert wi.any() and not wi.all()
        assert np.array_equal(grad, wg.astype(np.float32) + np.float32(0)), typ
