"""integration/HipWeightSpaceMedium.{hpp,cpp}, the Medium subclass of the weight-space GP medium, compiled against the reference's
REAL plugin interface (Medium.hpp:50-115, MediumSample.hpp, Ray.hpp, PathSampleGenerator.hpp, JsonPtr / JsonObject) with the
recipe of tests/test_integration_compile.py.  Skipped where the reference tree is absent (the GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"

pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present")


def _compile(tmp_path, src):
    obj = str(tmp_path / "binding_ws.o")
    cmd = ["g++", "-std=c++17", "-c", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror=overloaded-virtual",
           "-DCONSTEXPR=constexpr", "-DRAPIDJSON_HAS_STDSTRING=1",
           "-I", os.path.join(REF, "core"), "-isystem", os.path.join(REF, "thirdparty"),
           "-isystem", os.path.join(REF, "thirdparty", "eigen"), "-I", REF,
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "integration"), "-o", obj, src]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600), obj


def test_weight_space_binding_compiles_against_the_real_medium_interface(tmp_path):
    r, obj = _compile(tmp_path, os.path.join(ROOT, "integration", "HipWeightSpaceMedium.cpp"))
    assert r.returncode == 0, r.stderr[-4000:]
    syms = subprocess.run(["nm", "-C", obj], capture_output=True, text=True).stdout
    # every pure virtual of Tungsten::Medium (Medium.hpp:96-108) is defined with the reference's own signature
    for needle in (
        "Tungsten::HipWeightSpaceMedium::sampleDistance(Tungsten::PathSampleGenerator&, Tungsten::Ray const&, "
        "Tungsten::Medium::MediumState&, Tungsten::MediumSample&) const",
        "Tungsten::HipWeightSpaceMedium::transmittance(Tungsten::PathSampleGenerator&, Tungsten::Ray const&, bool, bool, "
        "Tungsten::Medium::MediumState*) const",
        "Tungsten::HipWeightSpaceMedium::isHomogeneous() const",
        "Tungsten::HipWeightSpaceMedium::sigmaA(Tungsten::Vec<float, 3u>) const",
        "Tungsten::HipWeightSpaceMedium::sigmaS(Tungsten::Vec<float, 3u>) const",
        "Tungsten::HipWeightSpaceMedium::sigmaT(Tungsten::Vec<float, 3u>) const",
        "Tungsten::HipWeightSpaceMedium::pdf(Tungsten::PathSampleGenerator&, Tungsten::Ray const&, bool, bool) const",
        "Tungsten::HipWeightSpaceMedium::fromJson(Tungsten::JsonPtr, Tungsten::Scene const&)",
        "Tungsten::HipWeightSpaceMedium::prepareForRender()",
    ):
        assert needle in syms, needle
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    undefined = [l.split()[-1] for l in syms.splitlines() if " U gpis_" in l]
    for want in ("gpis_ws_create", "gpis_ws_sample_distance_host", "gpis_ws_transmittance_host", "gpis_ws_default_params"):
        assert want in undefined, want
    for u in undefined:
        assert u + "(" in header, u


def test_weight_space_binding_is_instantiable_as_a_medium(tmp_path):
    tu = tmp_path / "use_ws.cpp"
    tu.write_text(r'''
#include "HipWeightSpaceMedium.hpp"
#include "sampling/UniformPathSampler.hpp"
#include <memory>
using namespace Tungsten;
std::shared_ptr<Medium> make() { return std::make_shared<HipWeightSpaceMedium>(); }
bool drive(const Medium &m, const Ray &ray)
{
    UniformPathSampler sampler(0xBA5EBA11u);
    Medium::MediumState state;
    state.reset();
    state.info.pixelSampleSegment = Vec4u(1u, 2u, 3u, 0u);
    MediumSample sample;
    bool ok = m.sampleDistance(sampler, ray, state, sample);
    Medium::MediumState shadow = state;
    Vec3f tr = m.transmittance(sampler, ray, false, false, &shadow);
    GPContextHipWs *ctxt = dynamic_cast<GPContextHipWs *>(state.gpContext.get());
    return ok && tr.x() >= 0.f && ctxt && sample.gpId == state.lastGPId;
}
''')
    r, _ = _compile(tmp_path, str(tu))
    assert r.returncode == 0, r.stderr[-4000:]
