"""GPU parity of NEE with an out-of-line mean (GPIS_MEAN_PROCEDURAL, GPIS_MEAN_TABULATED), BIT FOR BIT.

nee_shared (csrc/gpis_path.inc) reads the mean's gradient twice, and nee_instance() (csrc/gpis_hip.hip) sends such a medium with 1D
sampling to the all-features instance instead of the 1D one.  The reference is tests/sdf_march_ref.py's SdfComposite.nee_pdf /
nee_grad: the frozen ORACLE's own neePDF / neeGrad on the same medium with the mean replaced by the linear one whose float gradient
is the out-of-line mean's, for queries whose gradient is axis-aligned (tests/test_mean_nee_cpu.py pins that construction to the oracle
on analytic media and asserts, on the reference alone, the counts every case here rests on).

1. gpis_nee_pdf_batch / gpis_nee_grad_batch on the four media of test_gpu_parity.py::test_1d_sampling_and_nee and nine means: planes
   along +y, -x, +z, a clipped plane, the knob, a point- and a linearly sampled grid that varies along z, a CSG pair in both orders;
2. gpis_render_scene_s_nee / gpis_render_scene_s_nee_paths on a plane medium against NeePathsRef.compose over the composite, and on a
   constant grid against oracle_render_scene_s_nee on the homogeneous medium.

No tolerance on any device result."""
import ctypes

import numpy as np
import pytest

import grid_march_ref as gmr
import mean_nee_ref as mnr
import nee_paths_ref as npr
import sdf_mean_ref
from gpu_util import dev_empty, stream_ptr, to_dev, to_host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (sdf_mean_ref.available() and npr.available()), reason="no C compiler for the restatements")]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _medium(pkg, params, grids=(None, None), transforms=(None, None)):
    m = pkg.Medium(params)
    for w in range(2):
        if grids[w] is not None:
            gmr.set_grid(m, w, grids[w])
        if transforms[w] is not None:
            m.set_mean_transform(w, transforms[w])
    return m


# ---- 1. the batch entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(mnr.FAMILY))
@pytest.mark.parametrize("mean", mnr.MEANS)
def test_nee_entries_equal_the_oracle_through_the_standin(pkg, ob, family, mean):
    r = mnr.reference(pkg, ob, family, mean)
    q, want_pdf, want_grad = r["q"], r["pdf"], r["grad"]
    n = len(q)
    assert n >= 128 and (want_pdf > 0).sum() >= 64 and (want_pdf == 0).sum() >= 16
    m = _medium(pkg, *mnr.medium(pkg, family, mean))
    assert int(m.derived()["fast_path"]) == 0
    d_q, d_pdf, d_g = to_dev(q), dev_empty(4 * n), dev_empty(12 * n)
    m.reset_counters()
    m.call("gpis_nee_pdf_batch", ctypes.c_size_t(n), d_q.data_ptr(), d_pdf.data_ptr(), stream_ptr())
    m.call("gpis_nee_grad_batch", ctypes.c_size_t(n), d_q.data_ptr(), d_g.data_ptr(), stream_ptr())
    pdf, grad = to_host(d_pdf, np.float32)[:n], to_host(d_g, np.float32)[:3 * n].reshape(n, 3)
    assert m.counters() == (2 * n, 0)                       # one noise evaluation per query and entry
    bad = np.nonzero((_bits(grad) != _bits(want_grad)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:8], r["gid"][bad[:8]], grad[bad[:3]], want_grad[bad[:3]])
    bad = np.nonzero(_bits(pdf) != _bits(want_pdf))[0]
    assert bad.size == 0, (bad.size, bad[:8], r["gid"][bad[:8]], pdf[bad[:8]], want_pdf[bad[:8]])
    # the host entries are the same kernels behind a staging copy
    assert np.array_equal(_bits(m.nee_pdf(q)), _bits(want_pdf)) and np.array_equal(_bits(m.nee_grad(q)), _bits(want_grad))
    if mean.startswith("plane"):
        # the device does not differentiate the plane analytically: with the plane's own scale in place of the one-sided difference
        # the reference gives another nee_grad (asserted on the reference alone, then on the device's result)
        _, agrad = mnr.analytic_plane_nee(r["comp"], q, mean)
        assert (_bits(agrad) != _bits(want_grad)).any() and (_bits(agrad) != _bits(grad)).any()
    m.close()


# ---- 2. the frame drivers -------------------------------------------------------------------------------------------------------------
def _single(pkg, m, scene, surf):
    """one call of gpis_render_scene_s_nee into a zeroed device buffer"""
    import torch
    scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    h, w = int(scene["height"]), int(scene["width"])
    d_rad = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m.call("gpis_render_scene_s_nee", scene, np.array(surf, dtype=pkg.SURFACE_S), d_rad.data_ptr(), None)
    torch.cuda.synchronize()
    return d_rad.cpu().numpy().reshape(h, w)


def test_plane_frames_equal_the_composite(pkg, ob):
    """the 24 x 20 x 3 frame of tests/nee_paths_ref.py on the half-space x > 0.39 (plane under an axis-permuting transform), 2 and 4
    bounces: image and seg_count equal NeePathsRef.compose with the composite in the oracle's place; the 2-bounce frame is the
    single-interaction driver's"""
    params, grids, tfs = mnr.frame_medium(pkg)
    m = _medium(pkg, params, grids, tfs)
    scene, surf = npr.frame(ob), pkg.default_surface_s()
    for bounces in (2, 4):
        want = mnr.frame_reference(pkg, ob, bounces)
        hits, misses = want.hits[0], want.marched[0] - want.hits[0]
        assert hits >= want.marched[0] // 10 and misses >= want.marched[0] // 10 and want.image.any()
        m.reset_counters()
        img, segs = m.render_scene_s_nee_paths(scene, surf, bounces, want_segs=True)
        assert m.counters()[1] == want.n_seg
        assert np.array_equal(segs, want.seg_count), np.argwhere(segs != want.seg_count)[:8]
        assert np.array_equal(_bits(img), _bits(want.image)), np.argwhere(_bits(img) != _bits(want.image))[:8]
        if bounces == 2:
            assert np.array_equal(_bits(_single(pkg, m, scene, surf)), _bits(want.image))
    m.close()


def test_constant_grid_frame_equals_the_oracle(pkg, ob):
    """a constant grid of 0.25 with offset 0.25 and scale 0.5 is the homogeneous mean 0.25 with gradient exactly 0: both drivers equal
    oracle_render_scene_s_nee on that medium, with no restatement of ours in between"""
    params, grids, hom = mnr.constant_grid_medium(pkg)
    m = _medium(pkg, params, grids)
    scene, surf = npr.frame(ob), pkg.default_surface_s()
    want = ob.Oracle(hom, threads=8).render_scene_s_nee(scene, surf)
    assert want.any()
    got = _single(pkg, m, scene, surf)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8]
    assert np.array_equal(_bits(m.render_scene_s_nee_paths(scene, surf, 2)), _bits(want))
    m.close()
