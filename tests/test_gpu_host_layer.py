"""The host layer of the library (csrc/gpis_host_base.hpp: owning buffers, one error layer, one round trip for the *_host entries):
1. every host-pointer entry returns the bytes of its device-pointer entry while its staging slots grow, are reused larger than
   needed and carry stale bytes, for every null / non-null combination of the optional outputs;
2. the same for the function-space and the weight-space host entries;
3. a handle frees everything it allocated: ten create / use / destroy cycles cost less device memory than one handle holds;
4. the refusals keep their codes and texts and leave the library usable."""
import ctypes

import numpy as np
import pytest

import ws_oracle
from gpu_util import to_dev, dev_empty, to_host, stream_ptr

pytestmark = pytest.mark.gpu

SIZES = (1, 300, 5000, 3, 0, 300)      # grow, grow, reuse with room to spare (stale bytes behind the batch), nothing, reuse
f32, f64, i32 = np.float32, np.float64, np.int32


@pytest.fixture(scope="module")
def env(pkg, ob):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return pkg, pkg.load_library()


def _queries(pkg, dtype, n, seed):
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=dtype)
    q["p"] = rng.uniform(-1.4, 1.4, (n, 3))
    d = rng.standard_normal((2, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    if dtype == pkg.QUERY:
        q["dir"] = d[0]
    else:
        q["ray_dir"], q["normal"] = d[0], d[1]
    q["t_segment"], q["info_t"] = rng.uniform(0, 2, n), rng.uniform(0, 3, n)
    q["pixel"], q["spp"], q["segment"] = rng.integers(0, 1920, (n, 2)), rng.integers(0, 64, n), rng.integers(0, 4, n)
    q["scene_seed"] = 0xBA5EBA11
    q["coeff"]["value_scale"], q["coeff"]["gradient_scale"] = rng.uniform(0.5, 1.5, n), rng.uniform(-1, 1, (n, 3))
    return q


def _entries(pkg):
    """entry -> (inputs of n records, outputs as (dtype, items per record)): the argument lists of gpis_<entry>_host / _batch"""
    def q(n, s): return [_queries(pkg, pkg.QUERY, n, s)]
    def nq(n, s): return [_queries(pkg, pkg.NEE_QUERY, n, s)]
    def pts(n, s): return [np.random.default_rng(s).uniform(-1.4, 1.4, (n, 3))]

    def cond(n, s):
        rng = np.random.default_rng(s + 1)
        return q(n, s) + [rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, (n, 3)).astype(f32)]
    return {"eval_value": (q, [(f32, 1), (i32, 1)]), "eval_gradient": (q, [(f32, 3)]), "conditioning": (cond, [(pkg.COND_COEFF, 1)]),
            "nee_pdf": (nq, [(f32, 1)]), "nee_grad": (nq, [(f32, 3)]), "mean": (pts, [(f64, 1), (i32, 1), (f64, 3)]),
            "mean_color_emission": (pts, [(f32, 3), (f32, 3)])}


def _host_equals_batch(med, entry, n, inputs, outputs, want=None):
    """gpis_<entry>_host on numpy memory against gpis_<entry>_batch on torch buffers: the same bytes in every output asked for
    (want[k] false: a null pointer); outputs start as 0xFF / 0x00 so that a copy that did not happen shows"""
    want = want or [True] * len(outputs)
    size = [n * k * np.dtype(dt).itemsize for dt, k in outputs]
    host = [np.full(b, 0xFF, np.uint8) if w else None for b, w in zip(size, want)]
    med.call("gpis_%s_host" % entry, ctypes.c_size_t(n), *inputs, *host)
    d_in = [to_dev(a) for a in inputs]
    d_out = [dev_empty(b) if w else None for b, w in zip(size, want)]
    med.call("gpis_%s_batch" % entry, ctypes.c_size_t(n), *[t.data_ptr() for t in d_in], *[t.data_ptr() if t is not None else None for t in d_out], stream_ptr())
    for k, (h, d, b) in enumerate(zip(host, d_out, size)):
        if h is not None:
            assert np.array_equal(h, to_host(d, np.uint8)[:b]), (entry, n, want, "output %d" % k)


def test_host_entries_grow_and_reuse_their_slots(env):
    pkg, lib = env
    med = pkg.Medium(pkg.params_for_config("C0"))
    entries = _entries(pkg)
    for entry, (make, outputs) in entries.items():        # one handle: every entry finds the slots as the one before left them
        for k, n in enumerate(SIZES):
            _host_equals_batch(med, entry, n, make(n, 100 + k), outputs)
    for entry, required in (("eval_value", 1), ("mean", 0), ("mean_color_emission", 0)):
        make, outputs = entries[entry]
        optional = len(outputs) - required
        for mask in range(1 << optional):
            want = [True] * required + [bool(mask >> b & 1) for b in range(optional)]
            _host_equals_batch(med, entry, 300, make(300, 7), outputs, want)
    med.close()


def _fs_rays(pkg, n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=pkg.RAY_IN)
    r["pos"] = rng.uniform(-0.5, 0.5, (n, 3))
    d = rng.standard_normal((n, 3))
    r["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r["far_t"] = 0.5 + rng.uniform(0, 0.3, n)
    r["first_scatter"] = 1
    r["pixel"][:, 0] = np.arange(n)
    st = np.zeros(n, dtype=pkg.FS_STATE)
    st["sampler_state"] = rng.integers(1, 2**63, size=n, dtype=np.uint64)
    return r, st


def _fs_params(pkg):
    p = pkg.params_for_config("C0")
    p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL
    p["mean"]["type"], p["mean"]["offset"] = pkg.MEAN_TYPE.HOMOGENEOUS, 0.05
    p["fs_sample_points"], p["fs_step_size"] = 8, 0.04
    return p


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def test_function_space_host_entries(env):
    pkg, lib = env
    med = pkg.Medium(_fs_params(pkg))
    for k, n in enumerate((1, 65, 300, 3)):
        rays, st = _fs_rays(pkg, n, 40 + k)
        for fn, batch in (("sample_distance", med.fs_sample_distance), ("transmittance", med.fs_transmittance)):
            want, st_want = batch(rays, st)        # Medium's fs_* methods are the device-pointer entries on torch buffers
            got, st_got = np.full(n, 0xFF, np.uint8) if fn == "transmittance" else np.zeros(n, dtype=pkg.SEG_OUT), st.copy()
            med.call("gpis_fs_%s_host" % fn, ctypes.c_size_t(n), rays, st_got, got)
            assert np.array_equal(_bytes(got), _bytes(want)) and np.array_equal(_bytes(st_got), _bytes(st_want)), (fn, n)
    med.close()


def test_weight_space_host_entries(env):
    pkg, lib = env
    p, w = ws_oracle.ws_params(pkg, n_basis=20)
    med = pkg.WeightSpaceMedium(p, w)
    for k, n in enumerate((1, 300, 3)):
        rays = ws_oracle.make_rays(pkg, n, seed=60 + k)
        assert np.array_equal(_bytes(med.sample_distance(rays)), _bytes(med.sample_distance_batch(rays))), n
        assert np.array_equal(med.transmittance(rays), med.transmittance_batch(rays)), n
    med.close()


def _cycle(pkg, measure=None):
    """one handle of every kind, each used through its host entries, a frame driver and the entries that allocate for the handle;
    measure() is read while all of them are alive"""
    import torch
    scene = np.array(pkg.default_scene_s(32, 32, 2), dtype=pkg.SCENE_S)
    rad = torch.zeros(32 * 32, dtype=torch.float32, device="cuda")
    sc = pkg.Medium(pkg.params_for_config("C1"))
    sc.build_guide(16, 8)
    rays = ws_oracle.make_rays(pkg, 64, seed=3)
    sc.eval_value(_queries(pkg, pkg.QUERY, 64, 1))
    sc.set_profiling(True)
    sc.sample_distance(rays, want_coeff=True)
    sc.set_profiling(False)
    assert sc.kernel_profile(0)[1] == 1
    sc.transmittance(rays)
    sc.call("gpis_render_scene_s", scene.ctypes.data_as(ctypes.c_void_p), rad.data_ptr(), None, stream_ptr())
    fs = pkg.Medium(_fs_params(pkg))
    r, st = _fs_rays(pkg, 16, 5)
    fs.call("gpis_fs_sample_distance_host", ctypes.c_size_t(16), r, st, np.zeros(16, dtype=pkg.SEG_OUT))
    tab = pkg.params_for_config("C0")
    tab["single_realization"], tab["mean"]["type"] = 0, pkg.MEAN_TYPE.TABULATED
    tm = pkg.Medium(tab)
    tm.set_mean_grid(0, np.full((4, 4, 4), 0.25, f32), np.eye(4))
    tm.mean(np.zeros((8, 3)))
    grid = pkg.params_for_config("C3")
    grid["impulse_density"], grid["grid_nonstationary"] = 8, 1
    gm = pkg.Medium(grid)
    gm.set_variance_grid(np.full((4, 4, 4), 1.0, f32), np.eye(4))
    p, w = ws_oracle.ws_params(pkg, n_basis=20)
    ws = pkg.WeightSpaceMedium(p, w)
    ws.sample_distance(rays)
    ws.transmittance(rays)
    ws.render_scene_s(scene)
    torch.cuda.synchronize()
    held = measure() if measure else None
    for m in (sc, fs, tm, gm, ws):
        m.close()
    return held


def test_destroyed_handles_return_their_memory(env):
    """Ten cycles must cost less device memory than the handles of one cycle hold: a buffer that a handle owns and does not free
    would cost ten times its size.  (What the process keeps for itself — the runtime's pools, torch's cache — is there after
    the first cycle and is not counted.)"""
    import torch
    pkg, lib = env

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]
    before = free()
    footprint = before - _cycle(pkg, free)
    after_first = free()
    for _ in range(10):
        _cycle(pkg)
    drop = after_first - free()
    print("footprint of one cycle %d bytes, drop over ten more cycles %d bytes" % (footprint, drop))
    assert footprint > 0 and drop < footprint, (footprint, drop)


def test_refusals_keep_their_text_and_leave_nothing_behind(env):
    pkg, lib = env
    L = lib.lib
    h = ctypes.c_void_p()
    bad = pkg.params_for_config("C0")
    bad["impulse_density"] = -1
    assert L.gpis_create(bad.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(h)) == -1 and lib.last_error() == "impulse_density out of range"
    p, w = ws_oracle.ws_params(pkg, n_basis=1025)
    assert L.gpis_ws_create(p.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(h)) == -2
    assert lib.last_error() == "gpis_ws_create: basis_functions 1025 outside 0..1024" and not h.value
    p, w = ws_oracle.ws_params(pkg, n_basis=20)
    ws, sc = pkg.WeightSpaceMedium(p, w), pkg.Medium(pkg.params_for_config("C0"))
    q, val = _queries(pkg, pkg.QUERY, 4, 1), np.zeros(4, f32)
    assert L.gpis_eval_value_host(ws.h, 4, q.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert lib.last_error().startswith("gpis_eval_value_host: invalid argument (std_handle(m)")
    rays, out = ws_oracle.make_rays(pkg, 4), np.zeros(4, dtype=pkg.SEG_OUT)
    assert L.gpis_ws_sample_distance_host(sc.h, 4, rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.last_error() == "gpis_ws_sample_distance_host: not a weight-space handle (gpis_ws_create)"
    ws.close()
    sc.close()
    fresh = pkg.Medium(pkg.params_for_config("C0"))
    entry, (make, outputs) = "eval_value", _entries(pkg)["eval_value"]
    _host_equals_batch(fresh, entry, 10, make(10, 9), outputs)
    fresh.close()
