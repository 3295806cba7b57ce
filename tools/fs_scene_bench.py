"""Frame time of the function-space scene-S driver (gpis_fs_render_scene_s) against the staged composition of the batch entries:
one JSON document on stdout.

It renders one frame of scene S through a Renewal+ function-space medium (fs_sample_points 32, fs_step_size 0.02 by default) and
reports the fused entry (the whole call, timed with events after a warm-up) and the baseline: gpis_fs_sample_distance_batch on
the frame's valid primary rays plus gpis_fs_transmittance_batch on its lit shadow rays with the states the primary segments left.
Rays and states are prepared and uploaded beforehand (tests/fs_scene_ref.py) and the states restored from device copies before
every run; only the two calls are timed.  Baseline and fused entry run in the same process on the same frame, alternating, best
of --reps each.

    python tools/fs_scene_bench.py [--width 256 --height 256 --spp 8] [--reps 3] [--out profiles/r06_fs_scene_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _gpis_pkg  # noqa: E402
import oracle_bindings as ob  # noqa: E402
import fs_scene_ref  # noqa: E402
import ws_scene_ref  # noqa: E402


def run(pkg, ref, a):
    import torch
    p = fs_scene_ref.fs_params(pkg, a.ctx, a.points, a.step)
    scene = np.array(ws_scene_ref.small_scene(ob, a.width, a.height, a.spp, fov=a.fov), dtype=pkg.SCENE_S).reshape(())
    rays, us, _, n_miss = ref.base.primary_rays(scene)
    st0 = ref.primary_states(scene, rays)
    m = pkg.Medium(p)
    L = m.L.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
    n = len(rays)
    d_rays, d_st0 = up(rays), up(st0)
    d_st = d_st0.clone()
    d_seg = torch.zeros(n * pkg.SEG_OUT.itemsize, dtype=torch.uint8, device=dev)
    # the shadow rays and their states: the device's primary results (bit-identical to the restatement), shaded on the host
    m.L.check(L.gpis_fs_sample_distance_batch(m.h, n, vp(d_rays), vp(d_st), vp(d_seg), sp), "gpis_fs_sample_distance_batch")
    torch.cuda.synchronize(dev)
    seg = d_seg.cpu().numpy().view(pkg.SEG_OUT)
    st1 = d_st.cpu().numpy().view(pkg.FS_STATE)
    shadow, _, hit, lit = ref.base.shade(scene, rays, seg, us)
    idx = np.nonzero(lit)[0]
    ns = len(idx)
    d_sh, d_sst0 = up(shadow[idx]), up(st1[idx])
    d_sst = d_sst0.clone()
    d_vis = torch.zeros(max(ns, 1), dtype=torch.uint8, device=dev)
    npix = int(scene["width"]) * int(scene["height"])
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_hit = torch.zeros(npix, dtype=torch.int32, device=dev)
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)

    def staged():
        m.L.check(L.gpis_fs_sample_distance_batch(m.h, n, vp(d_rays), vp(d_st), vp(d_seg), sp), "gpis_fs_sample_distance_batch")
        m.L.check(L.gpis_fs_transmittance_batch(m.h, ns, vp(d_sh), vp(d_sst), vp(d_vis), sp), "gpis_fs_transmittance_batch")

    def fused():
        m.L.check(L.gpis_fs_render_scene_s(m.h, scene_p, vp(d_rad), vp(d_hit), sp), "gpis_fs_render_scene_s")

    def timed(fn):
        d_st.copy_(d_st0)                            # the batch entries rewrite their states in place
        d_sst.copy_(d_sst0)
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / 1e3

    timed(staged)                                    # warm-up: workspaces, code objects
    timed(fused)
    t_staged, t_fused = [], []
    for _ in range(a.reps):
        t_staged.append(timed(staged))
        t_fused.append(timed(fused))
    vis = d_vis.cpu().numpy()[:ns]
    m.close()
    bs, bf = min(t_staged), min(t_fused)
    n_samples = n + n_miss
    return {
        "context": a.ctx, "fs_sample_points": a.points, "fs_step_size": a.step,
        "samples": n_samples, "valid_primary_rays": n, "shadow_rays": ns, "visible_shadow_rays": int(vis.sum()), "reps": a.reps,
        "fused_seconds_best": bf, "fused_seconds_all": t_fused, "staged_seconds_best": bs, "staged_seconds_all": t_staged,
        "fused_over_staged": bf / bs, "fused_not_slower": bool(bf <= bs),
        "samples_per_s": n_samples / bf, "segments_per_s": (n + ns) / bf, "hit_fraction": float(hit.sum()) / n_samples,
        "staged_state_bytes": int(n + ns) * pkg.FS_STATE.itemsize, "fused_record_bytes": 8 * n_samples,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--fov", type=float, default=35.0)      # the default scene S: every sample meets the bounding sphere
    ap.add_argument("--ctx", default="RENEWAL_PLUS")
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 3)
    pkg = _gpis_pkg.load_package()
    ref = fs_scene_ref.FsSceneRef(pkg, ob)
    doc = {"workload": "scene S (camera z = 4, fov %g, bounding radius 1.5, light (0.5, 0.7, 0.5)), %d x %d x %d spp = %d samples, through the "
                       "function-space GP medium, spherical mean r = 1 (C0-like: sigma 0.1, l 0.05)"
                       % (a.fov, a.width, a.height, a.spp, a.width * a.height * a.spp),
           "fused": "gpis_fs_render_scene_s, the whole call: k_fs_scene (one wave per sample, dynamic work fetch, the state in one slot "
                    "per resident workgroup) + k_fs_scene_sum",
           "staged_baseline": "gpis_fs_sample_distance_batch on the valid primary rays + gpis_fs_transmittance_batch on the lit shadow rays "
                              "with the primary segments' states, all uploaded beforehand; the two calls only (no ray generation, shading, "
                              "state copy or pixel sum)",
           "result": run(pkg, ref, a)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
