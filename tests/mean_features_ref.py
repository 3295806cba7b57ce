"""TEST INFRASTRUCTURE: the media and ray batches of tests/test_gpu_mean_features.py (CSG pairs, the colour point, the marches outside
C0 and the constant-mean anchors of a procedural / tabulated mean), and their composite references, computed once per process.

tests/test_mean_features_cpu.py asserts on the composite alone what the device tests rest on (both CSG ids among the hits and among
the continued rays, hits and exits in every batch, a hit weight that varies with the colour)."""
import numpy as np

import grid_march_ref as gmr
import sdf_march_ref as smr

f32 = np.float32
N_RAYS = 321
N_QUERIES = 193


def march_base(pkg, ctx):
    """C0 with step_size 0.02 in the given context: the medium of test_march_equals_the_composite"""
    p = pkg.params_for_config("C0")
    p["step_size"] = 0.02
    if ctx != "none":
        p["single_realization"] = 0
        p["correlation_context"] = pkg.CTX.RENEWAL if ctx == "renewal" else pkg.CTX.RENEWAL_PLUS
    return p


def config(pkg, name):
    """the media of tests/test_gpu_sdf_mean.py::_config, with the march's step_size 0.02"""
    if name == "iso-ray":
        p = pkg.params_for_config("C1")
    elif name == "1d-xy":
        p = pkg.params_for_config("C2")
    elif name == "matern":
        p = pkg.params_for_config("C0")
        p["single_realization"], p["correlation_context"] = 0, pkg.CTX.RENEWAL
        p["kernel_type"], p["matern_v"] = 1, 2.5
    else:
        raise ValueError(name)
    p["step_size"] = 0.02
    return p


def csg_pair(pkg, base, pair):
    """(params, grids, transforms): "knob+sphere" = the knob united with a sphere of radius 0.5 about (0.7, 0, 0) (the second slot is
    an analytic mean next to an out-of-line one); "grid+plane" = the tabulated two-sphere grid united with plane, offset 0.3, under
    transform_demo()"""
    if pair == "knob+sphere":
        p = smr.procedural(pkg, base, "knob")
        p["has_mean_additional"] = 1
        p["mean_additional"]["type"] = pkg.MEAN_TYPE.SPHERICAL
        p["mean_additional"]["radius"] = 0.5
        p["mean_additional"]["center"] = (0.7, 0.0, 0.0)
        return p, (None, None), (None, None)
    p = gmr.tabulated(pkg, base)
    p = smr.procedural(pkg, p, "plane", offset=0.3, slot="mean_additional")
    g = gmr.grid(pkg, gmr.sphere_voxels(), gmr.sphere_world_to_index(), "linear")
    return p, (g, None), (None, smr.transform_demo())


def colour(pkg, base, kind):
    """the knob under transform_demo() with a colour field: "ramp" = the two-ramp field of tests/nee_paths_ref.py::_colour, "sandstone" =
    the vector noise of test_sandstone_and_rust_noises (type 4, min = max = 0)"""
    p = smr.procedural(pkg, base, "knob")
    c = p["mean_color"]
    c["enabled"] = 1
    if kind == "ramp":
        c["type"] = 1
        c["min"], c["max"], c["start"], c["end"] = 0.2, 0.9, -1.0, 1.0
        c["min2"], c["max2"], c["start2"], c["end2"] = 0.5, 1.5, -0.5, 0.5
    else:
        c["type"], c["min"], c["max"] = 4, 0.0, 0.0
    return p, (None, None), (smr.transform_demo(), None)


def continued(pkg, first_out, seed):
    """N_RAYS continued segments from the hits of a first-scatter batch, with the state (aniso, gp_id) each hit left"""
    idx = np.nonzero((first_out["exited"] == 0) & (first_out["ok"] != 0))[0]
    pick = idx[np.arange(N_RAYS) % len(idx)]
    r = smr.camera_rays(pkg, N_RAYS, seed, first_scatter=False, state=(0.0, first_out["aniso"][pick], first_out["gp_id"][pick]))
    rng = np.random.default_rng(seed + 1)
    d = rng.normal(size=(N_RAYS, 3))
    r["pos"] = first_out["p"][pick]
    r["dir"] = d / np.linalg.norm(d, axis=1)[:, None]
    r["near_t"] = 0
    r["far_t"] = rng.uniform(0.2, 1.2, N_RAYS)
    r["info_t"] = first_out["sample_t"][pick]
    return r


_memo = {}


def march_reference(pkg, ob, key, medium):
    """the composite's first-scatter and continued batch of `medium` = (params, grids, transforms): a list of dicts (rays, out, coeff,
    trips, vis, n_sd, n_tr), computed once per process under `key` and read-only"""
    if key not in _memo:
        params, grids, tfs = medium
        comp = gmr.GridComposite(pkg, ob, params, grids=grids, transforms=tfs, threads=8)
        rays = smr.camera_rays(pkg, N_RAYS, 5)
        batches = []
        for k in range(2):
            r = rays if k == 0 else continued(pkg, batches[0]["out"], 6)
            w, wc, trips = comp.sample_distance(r, want_coeff=True, want_trips=True)
            n_sd = comp.last_n_eval
            vis = comp.transmittance(r)
            b = dict(rays=r, out=w, coeff=wc, trips=trips, vis=vis, n_sd=n_sd, n_tr=comp.last_n_eval)
            for a in (r, w, wc, trips, vis):
                a.setflags(write=False)
            batches.append(b)
        _memo[key] = (comp, batches)
    return _memo[key]


def summary(b):
    w = b["out"]
    hit = w["exited"] == 0
    return dict(hits=int(hit.sum()), exits=int((~hit).sum()), not_ok=int((w["ok"] == 0).sum()), trips_gt_1=int((b["trips"] > 1).sum()),
                hit_ids=[int((hit & (w["gp_id"] == i)).sum()) for i in (0, 1)],
                last_ids=[int((b["rays"]["last_gp_id"] == i).sum()) for i in (0, 1)])
