// HipWeightSpaceMedium.hpp — the binding of the weight-space GP medium (random Fourier features) a Tungsten maintainer drops into
// src/core/media/ next to HipSparseConvNoiseMedium; registered as "weight_space_gaussian_process" (MediumFactory.cpp:13-22).
//
// A `Tungsten::Medium` subclass (src/core/media/Medium.hpp:50-115) that forwards the hot path of
// `WeightSpaceGaussianProcessMedium` (src/core/media/WeightSpaceGaussianProcessMedium.cpp:34-291 under
// GaussianProcessMedium.cpp:221-398) to gpis_ws_sample_distance_host / gpis_ws_transmittance_host of include/gpis.h, one segment
// per call.  Like the other bindings it includes only headers of the reference that compile without Boost / FFTW / OpenVDB, so
// tests/test_integration_compile_ws.py compiles it against the real interface.
//
// Variates: the medium draws exactly one sampler.next1D() per segment that reaches the march (the jitter of
// WeightSpaceGaussianProcessMedium.cpp:247); the binding draws it here and hands it to the device in gpis_ray_in::u_jitter.  The
// realization itself depends on state.info.pixelSampleSegment only, so the device rebuilds it from the ray record.
#ifndef HIPWEIGHTSPACEMEDIUM_HPP_
#define HIPWEIGHTSPACEMEDIUM_HPP_

#include "media/Medium.hpp"
#include "samplerecords/MediumSample.hpp"
#include "math/Ray.hpp"
#include "sampling/PathSampleGenerator.hpp"

#include <gpis.h>

#include <memory>
#include <string>
#include <vector>

namespace Tungsten {

// What MediumState::gpContext points to for this medium (the role of GPContextWeightSpace, WeightSpaceGaussianProcessMedium.hpp:
// 11-16): the pixelSampleSegment the realization was drawn for.  reset() keeps it, as the reference keeps its realization.
struct GPContextHipWs : public GPContext
{
    uint32 pss[4] = {0u, 0u, 0u, 0u};
    virtual void reset() override {}
};

class HipWeightSpaceMedium : public Medium
{
    gpis_params _params;
    gpis_ws_params _ws;
    gpis_medium *_handle;
    int _device;
    Vec3f _sigmaA, _sigmaS, _sigmaT;
    bool _absorptionOnly;
    std::vector<std::shared_ptr<PhaseFunction>> _phaseFunctions;

    void fillRay(const Ray &ray, const MediumState &state, float jitter, gpis_ray_in &r) const;
    void setContext(MediumState &state) const;

public:
    HipWeightSpaceMedium();
    virtual ~HipWeightSpaceMedium();

    virtual void fromJson(JsonPtr value, const Scene &scene) override;
    virtual rapidjson::Value toJson(Allocator &allocator) const override;

    virtual bool isHomogeneous() const override { return false; }      // GaussianProcessMedium.cpp:147-150

    virtual void prepareForRender() override;                          // GaussianProcessMedium.cpp:152-158 + gpis_ws_create
    virtual void teardownAfterRender() override;

    virtual Vec3f sigmaA(Vec3f /*p*/) const override { return _sigmaA; }
    virtual Vec3f sigmaS(Vec3f /*p*/) const override { return _sigmaS; }
    virtual Vec3f sigmaT(Vec3f /*p*/) const override { return _sigmaT; }

    virtual bool sampleDistance(PathSampleGenerator &sampler, const Ray &ray,
            MediumState &state, MediumSample &sample) const override;
    virtual Vec3f transmittance(PathSampleGenerator &sampler, const Ray &ray, bool startOnSurface,
            bool endOnSurface, MediumState *state) const override;
    virtual float pdf(PathSampleGenerator &/*sampler*/, const Ray &/*ray*/, bool /*startOnSurface*/,
            bool /*endOnSurface*/) const override { return 1.0f; }     // GaussianProcessMedium.cpp:395-398

    void setDevice(int device) { _device = device; }
    gpis_medium *handle() const { return _handle; }
    const gpis_params &params() const { return _params; }
    const gpis_ws_params &wsParams() const { return _ws; }
};

}

#endif /* HIPWEIGHTSPACEMEDIUM_HPP_ */
