"""The JSON side of the tabulated mean: `"type": "tabulated"` through the shared key table (include/gpis_json.hpp) as the
stand-alone host adapter reads it.  A small program over libgpis_host.so (tests/native/grid_mean_json.cpp) parses a medium JSON
and prints the mean slots of the gpis_params it yields, or the error.  The "grid" object is the loader's."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sparse-conv-gpis-tungsten_amd", "host")
SRC = os.path.join(ROOT, "tests", "native", "grid_mean_json.cpp")
OUT_DIR = os.path.join(ROOT, "build", "grid_mean_json")
EXE = os.path.join(OUT_DIR, "grid_mean_json")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__ as g
    g.build_hip()
    g.build_host_adapter()
    lib = os.path.join(HOST, "libgpis_host.so")
    deps = [SRC, lib, os.path.join(HOST, "HipSparseConvNoiseMedium.hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(OUT_DIR, exist_ok=True)
        csrc = os.path.join(ROOT, "sparse-conv-gpis-tungsten_amd", "csrc")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", EXE, SRC,
                               "-L", HOST, "-lgpis_host", "-L", csrc, "-lgpis_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + csrc])

    def run(mean, additional=None):
        gp = {"mean": mean, "covariance": {"type": "squared_exponential", "sigma": 0.1, "lengthScale": 0.05}}
        if additional is not None:
            gp["mean_additional"] = additional
        medium = {"type": "sparse_conv_noise", "correlation_context": "none", "sigma_s": 1.0, "gaussian_process": gp}
        out = subprocess.run([EXE], input=json.dumps(medium), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def _slot(text, name):
    m = re.search(r"^%s type=(-?\d+) volume=(-?\d+) offset=(\S+) scale=(\S+)$" % name, text, flags=re.M)
    assert m, text
    f = lambda v: float(np.float32(float(v)))         # %.9g round-trips a float
    return int(m.group(1)), int(m.group(2)), f(m.group(3)), f(m.group(4))


GRID = {"type": "vdb", "file": "bunny.vdb", "interpolate": "linear"}        # left to the loader: readMean does not look at it


def test_tabulated_mean_with_its_defaults(probe):
    out = probe({"type": "tabulated", "grid": GRID})
    assert _slot(out, "mean") == (4, 0, 0.0, 1.0) and "has_mean_additional=0" in out


def test_offset_scale_and_volume(probe):
    f = lambda v: float(np.float32(v))
    out = probe({"type": "tabulated", "grid": GRID, "offset": -0.02, "scale": 12.5, "volume": True})
    assert _slot(out, "mean") == (4, 1, f(-0.02), f(12.5))
    assert _slot(probe({"type": "tabulated", "volume": False, "scale": 2}), "mean") == (4, 0, 0.0, 2.0)


def test_either_slot(probe):
    out = probe({"type": "spherical", "radius": 0.5}, {"type": "tabulated", "grid": GRID, "offset": 0.25, "volume": True})
    assert _slot(out, "mean")[0] == 1 and _slot(out, "mean_additional") == (4, 1, 0.25, 1.0) and "has_mean_additional=1" in out
    out = probe({"type": "tabulated", "grid": GRID}, {"type": "procedural", "func": "plane"})
    assert _slot(out, "mean") == (4, 0, 0.0, 1.0) and _slot(out, "mean_additional")[0] == 3
    out = probe({"type": "tabulated", "scale": 3}, {"type": "tabulated", "volume": True})
    assert _slot(out, "mean") == (4, 0, 0.0, 3.0) and _slot(out, "mean_additional") == (4, 1, 0.0, 1.0)


def test_unknown_type_still_fails_with_the_reference_message(probe):
    assert probe({"type": "mesh"}).strip() == "error: Unsupported mean function type: 'mesh'"
    assert probe({"type": "neural"}).strip() == "error: Unsupported mean function type: 'neural'"
