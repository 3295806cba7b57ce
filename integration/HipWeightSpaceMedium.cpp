// HipWeightSpaceMedium.cpp — see the header.  Compiles against the reference's real headers with the same command as
// HipSparseConvNoiseMedium.cpp (tests/test_integration_compile_ws.py).  Links against libgpis_hip.so.
#include "HipWeightSpaceMedium.hpp"
#include "TungstenJsonAccess.hpp"

#include "io/JsonObject.hpp"

#include <cmath>
#include <cstring>

namespace Tungsten {

HipWeightSpaceMedium::HipWeightSpaceMedium()
: _handle(nullptr),
  _device(0),
  _sigmaA(0.0f),
  _sigmaS(0.0f),
  _sigmaT(0.0f),
  _absorptionOnly(true)
{
    gpis_default_params(&_params);             // GaussianProcessMedium defaults (GaussianProcessMedium.cpp:86-95)
    gpis_ws_default_params(&_ws);              // WeightSpaceGaussianProcessMedium.cpp:21-32
    _params.single_realization = 0;
    _params.step_size = 0.01f;
    _params.min_step = 8;
    _params.seed = 0;
}

HipWeightSpaceMedium::~HipWeightSpaceMedium()
{
    teardownAfterRender();
}

void HipWeightSpaceMedium::fromJson(JsonPtr value, const Scene &scene)
{
    Medium::fromJson(value, scene);      // phase_function, transmittance, max_bounces (Medium.cpp:29-38)
    _params.max_bounces = _maxBounce;

    // GaussianProcessMedium::fromJson (GaussianProcessMedium.cpp:97-126) and GaussianProcess::fromJson for an inline object
    // (GaussianProcess.cpp:172-190) through the shared key table (include/gpis_json.hpp)
    TungstenJson::vec3f(value, "sigma_a", _params.sigma_a);
    TungstenJson::vec3f(value, "sigma_s", _params.sigma_s);
    TungstenJson::num(value, "density", _params.density);
    std::string ctxtString = "goldfish";
    value.getField("correlation_context", ctxtString);
    _params.correlation_context = gpis_json::correlationContext<TungstenJson>(ctxtString);
    std::string intersectString = "gp_discrete";
    value.getField("intersect_method", intersectString);
    if (intersectString == "gp_discrete")
        _ws.intersect_method = GPIS_INTERSECT_GP_DISCRETE;
    else if (intersectString == "mean")
        _ws.intersect_method = GPIS_INTERSECT_MEAN;            // refused by gpis_ws_create
    else
        FAIL("weight_space_gaussian_process: invalid intersect method '%s'", intersectString);
    std::string normalString = "conditioned_gaussian";
    value.getField("normal_method", normalString);
    if (normalString == "conditioned_gaussian")
        _ws.normal_method = GPIS_NORMAL_CONDITIONED_GAUSSIAN;
    else if (normalString == "finite_differences")
        _ws.normal_method = GPIS_NORMAL_FINITE_DIFFERENCES;
    else if (normalString == "beckmann")
        _ws.normal_method = GPIS_NORMAL_BECKMANN;              // refused by gpis_ws_create
    else if (normalString == "ggx")
        _ws.normal_method = GPIS_NORMAL_GGX;                   // refused by gpis_ws_create
    else
        FAIL("weight_space_gaussian_process: invalid normal sampling method '%s'", normalString);
    if (auto gp = value["gaussian_process"]) {
        if (!gp.isObject())
            FAIL("weight_space_gaussian_process: \"gaussian_process\" must be an inline object");
        gpis_json::readGaussianProcess<TungstenJson>(gp, _params);
    }
    _phaseFunctions.clear();
    _phaseFunctions.push_back(_phaseFunction);     // "additional_phase_functions" needs Scene::fetchPhase (io/Scene.hpp, not included)

    // WeightSpaceGaussianProcessMedium::fromJson, WeightSpaceGaussianProcessMedium.cpp:34-50
    value.getField("basis_functions", _ws.basis_functions);
    bool single = _params.single_realization != 0;
    value.getField("single_realization", single);
    _params.single_realization = single ? 1 : 0;
    value.getField("step_size", _params.step_size);
    uint32 minStep = _params.min_step, seed = _params.seed;
    value.getField("min_step", minStep);
    value.getField("seed", seed);
    _params.min_step = minStep;
    _params.seed = seed;
    int device = _device;
    value.getField("hip_device", device);
    _device = device;
}

rapidjson::Value HipWeightSpaceMedium::toJson(Allocator &allocator) const
{
    static const char *ctxNames[] = {"global", "renewal+", "renewal", "none"};
    static const char *normalNames[] = {"conditioned_gaussian", "finite_differences", "beckmann", "ggx"};
    return JsonObject{Medium::toJson(allocator), allocator,
        "type", "weight_space_gaussian_process",
        "sigma_a", Vec3f(_params.sigma_a[0], _params.sigma_a[1], _params.sigma_a[2]),
        "sigma_s", Vec3f(_params.sigma_s[0], _params.sigma_s[1], _params.sigma_s[2]),
        "density", _params.density,
        "correlation_context", ctxNames[_params.correlation_context],
        "intersect_method", _ws.intersect_method == GPIS_INTERSECT_MEAN ? "mean" : "gp_discrete",
        "normal_method", normalNames[_ws.normal_method & 3],
        "basis_functions", _ws.basis_functions,
        "single_realization", _params.single_realization != 0,
        "step_size", _params.step_size,
        "min_step", _params.min_step,
        "seed", _params.seed
    };
}

void HipWeightSpaceMedium::prepareForRender()
{
    teardownAfterRender();
    _sigmaA = Vec3f(_params.sigma_a[0], _params.sigma_a[1], _params.sigma_a[2])*_params.density;
    _sigmaS = Vec3f(_params.sigma_s[0], _params.sigma_s[1], _params.sigma_s[2])*_params.density;
    _sigmaT = _sigmaA + _sigmaS;
    _absorptionOnly = _sigmaS == 0.0f;
    if (gpis_ws_create(&_params, &_ws, _device, &_handle) != GPIS_OK) {
        _handle = nullptr;
        FAIL("weight_space_gaussian_process: gpis_ws_create failed: %s", gpis_last_error());
    }
}

void HipWeightSpaceMedium::teardownAfterRender()
{
    if (_handle)
        gpis_destroy(_handle);
    _handle = nullptr;
}

void HipWeightSpaceMedium::fillRay(const Ray &ray, const MediumState &state, float jitter, gpis_ray_in &r) const
{
    std::memset(&r, 0, sizeof r);
    for (int i = 0; i < 3; ++i) {
        r.pos[i] = ray.pos()[i];
        r.dir[i] = ray.dir()[i];
        r.last_aniso[i] = state.lastAniso[i];
    }
    r.near_t = ray.nearT();
    r.far_t = ray.farT();
    r.pixel[0] = state.info.pixelSampleSegment.x();
    r.pixel[1] = state.info.pixelSampleSegment.y();
    r.spp = state.info.pixelSampleSegment.z();
    r.segment = state.info.pixelSampleSegment.w();
    r.scene_seed = state.info.sceneSeed;
    r.info_t = state.info.t;
    r.u_jitter = jitter;
    r.first_scatter = state.firstScatter ? 1u : 0u;
    r.bounce = state.bounce;
    r.last_val = state.lastVal;
    r.last_gp_id = state.lastGPId;
}

// intersectGP / sampleGradient leave the realization's context in the state (WeightSpaceGaussianProcessMedium.cpp:160-176)
void HipWeightSpaceMedium::setContext(MediumState &state) const
{
    auto ctxt = std::make_shared<GPContextHipWs>();
    ctxt->pss[0] = state.info.pixelSampleSegment.x();
    ctxt->pss[1] = state.info.pixelSampleSegment.y();
    ctxt->pss[2] = state.info.pixelSampleSegment.z();
    ctxt->pss[3] = state.info.pixelSampleSegment.w();
    state.gpContext = ctxt;
}

// GaussianProcessMedium::sampleDistance, GaussianProcessMedium.cpp:221-341 over WeightSpaceGaussianProcessMedium::intersectGP /
// sampleGradient: the march and the gradient run on the device; the MediumState / MediumSample writes below are the reference's.
bool HipWeightSpaceMedium::sampleDistance(PathSampleGenerator &sampler, const Ray &ray,
        MediumState &state, MediumSample &sample) const
{
    sample.emission = Vec3f(0.0f);
    if (state.bounce >= _maxBounce)
        return false;

    float maxT = ray.farT();
    if (!std::isfinite(maxT))
        maxT = float(double(ray.nearT()) + 2000);
    if (maxT == 0.f) {
        sample.t = maxT;
        sample.weight = Vec3f(1.f);
        sample.pdf = 1.0f;
        sample.exited = true;
        sample.p = ray.pos() + sample.t*ray.dir();
        sample.phase = _phaseFunction.get();
        sample.sparseConv1DSamplingScheme = SparseConv1DSamplingScheme::UNI;
        return true;
    }
    // (GaussianProcessMedium.cpp:250-252 compares maxT with infinity AFTER the clamp above, so an absorption-only medium never
    // ends the path there: it marches the clamped segment like any other, on the device)

    gpis_ray_in r;
    gpis_seg_out o;
    fillRay(ray, state, sampler.next1D(), r);          // the march's one jitter (WeightSpaceGaussianProcessMedium.cpp:247)
    if (gpis_ws_sample_distance_host(_handle, 1, &r, &o) != GPIS_OK)
        FAIL("gpis_ws_sample_distance_host: %s", gpis_last_error());
    setContext(state);

    state.lastGPId = o.gp_id;
    state.sparseConv1DSamplingScheme = SparseConv1DSamplingScheme::UNI;
    sample.exited = o.exited != 0;
    if (_absorptionOnly) {
        state.lastAniso = Vec3d(o.aniso[0], o.aniso[1], o.aniso[2]);
        if (o.weight[0] == 0.f)
            state.firstScatter = false;
    } else {
        state.lastAniso = sample.aniso = Vec3d(o.aniso[0], o.aniso[1], o.aniso[2]);
        state.firstScatter = false;
    }
    if (!o.ok)
        return false;

    sample.t = o.sample_t;
    sample.continuedT = o.continued_t;
    sample.weight = Vec3f(o.weight[0], o.weight[1], o.weight[2]);
    sample.continuedWeight = Vec3f(o.continued_weight[0], o.continued_weight[1], o.continued_weight[2]);
    sample.pdf = 1.0f;
    sample.sparseConv1DSamplingScheme = SparseConv1DSamplingScheme::UNI;
    if (!_absorptionOnly)
        state.advance();
    sample.p = Vec3f(o.p[0], o.p[1], o.p[2]);
    sample.phase = _phaseFunctions[size_t(state.lastGPId) < _phaseFunctions.size() ? state.lastGPId : 0].get();
    sample.gpId = state.lastGPId;
    sample.ctxt = state.gpContext.get();
    state.info.t += sample.t;
    sample.rayInfo = state.info;
    return true;
}

// GaussianProcessMedium::transmittance, GaussianProcessMedium.cpp:343-393: 1 if the segment left the medium, else 0; firstScatter and
// lastAniso change on a hit only (:371-381)
Vec3f HipWeightSpaceMedium::transmittance(PathSampleGenerator &sampler, const Ray &ray, bool /*startOnSurface*/,
        bool /*endOnSurface*/, MediumState *state) const
{
    gpis_ray_in r;
    uint8_t visible = 0;
    fillRay(ray, *state, sampler.next1D(), r);
    if (gpis_ws_transmittance_host(_handle, 1, &r, &visible) != GPIS_OK)      // as sampleDistance: no result of a failed call is used
        FAIL("gpis_ws_transmittance_host: %s", gpis_last_error());
    setContext(*state);
    if (!visible)
        state->firstScatter = false;
    return visible ? Vec3f(1.0f) : Vec3f(0.0f);
}

}
