"""Frame time of the function-space multi-bounce path driver (gpis_fs_render_scene_s_paths): one JSON document on stdout.

It renders one frame of scene S through a Renewal+ function-space medium (fs_sample_points 32, fs_step_size 0.02, max_bounces 3,
albedo 0.8 by default) and reports the whole call (timed with events after a warm-up, best of --reps) in seconds per frame,
segments per second (path plus shadow segments, read from seg_count) and paths per second.  Next to it stands the segment rate of
the batch entries (k_fs_march): the one measured in this process by gpis_fs_sample_distance_batch on the frame's valid primary
rays from empty states (uploaded beforehand, restored before every run), and the one profiles/r06_fs_scene_bench.json recorded
for the staged scene-S frame (primary plus shadow segments over the two batch calls), with the ratios.

    python tools/fs_paths_bench.py [--width 256 --height 256 --spp 8] [--reps 3] [--out profiles/r07_fs_paths_bench.json]
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

R06 = os.path.join(ROOT, "profiles", "r06_fs_scene_bench.json")


def run(pkg, ref, a):
    import torch
    p = fs_scene_ref.fs_params(pkg, a.ctx, a.points, a.step)
    scene = np.array(ws_scene_ref.small_scene(ob, a.width, a.height, a.spp, fov=a.fov), dtype=pkg.SCENE_S).reshape(())
    rays, _, _, n_miss = ref.base.primary_rays(scene)
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
    npix = int(scene["width"]) * int(scene["height"])
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(npix, dtype=torch.int32, device=dev)
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)

    def batch():
        m.L.check(L.gpis_fs_sample_distance_batch(m.h, n, vp(d_rays), vp(d_st), vp(d_seg), sp), "gpis_fs_sample_distance_batch")

    def fused():
        m.L.check(L.gpis_fs_render_scene_s_paths(m.h, scene_p, a.bounces, ctypes.c_float(a.albedo), vp(d_rad), vp(d_cnt), sp), "gpis_fs_render_scene_s_paths")

    def timed(fn):
        d_st.copy_(d_st0)                            # the batch entry rewrites its states in place
        d_cnt.zero_()
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / 1e3

    timed(batch)                                     # warm-up: workspaces, code objects
    timed(fused)
    t_batch, t_fused = [], []
    for _ in range(a.reps):
        t_batch.append(timed(batch))
        t_fused.append(timed(fused))
    segments = int(d_cnt.cpu().numpy().astype(np.int64).sum())      # of the last fused call
    m.close()
    bb, bf = min(t_batch), min(t_fused)
    n_samples = n + n_miss
    out = {
        "context": a.ctx, "fs_sample_points": a.points, "fs_step_size": a.step, "max_path_bounces": a.bounces, "albedo": a.albedo,
        "samples": n_samples, "paths": n, "segments": segments, "segments_per_path": segments / max(n, 1), "reps": a.reps,
        "seconds_per_frame_best": bf, "seconds_per_frame_all": t_fused,
        "segments_per_s": segments / bf, "paths_per_s": n / bf, "samples_per_s": n_samples / bf,
        "batch_primary_segments": n, "batch_seconds_best": bb, "batch_seconds_all": t_batch, "batch_segments_per_s": n / bb,
        "fused_over_batch_segment_rate": (segments / bf) / (n / bb),
        "state_slot_bytes_per_workgroup": 2 * pkg.FS_STATE.itemsize, "record_bytes": 8 * n_samples,
    }
    if os.path.exists(R06):
        r = json.load(open(R06))["result"]
        rate = (r["valid_primary_rays"] + r["shadow_rays"]) / r["staged_seconds_best"]
        out["r06_staged_batch_segments_per_s"] = rate
        out["fused_over_r06_staged_segment_rate"] = (segments / bf) / rate
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--fov", type=float, default=35.0)      # the default scene S: every sample meets the bounding sphere
    ap.add_argument("--ctx", default="RENEWAL_PLUS")
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--albedo", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.reps = max(a.reps, 3)
    pkg = _gpis_pkg.load_package()
    ref = fs_scene_ref.FsSceneRef(pkg, ob)
    doc = {"workload": "scene S (camera z = 4, fov %g, bounding radius 1.5, light (0.5, 0.7, 0.5)), %d x %d x %d spp = %d samples, multi-bounce "
                       "paths through the function-space GP medium, spherical mean r = 1 (C0-like: sigma 0.1, l 0.05)"
                       % (a.fov, a.width, a.height, a.spp, a.width * a.height * a.spp),
           "fused": "gpis_fs_render_scene_s_paths, the whole call: k_fs_paths (one wave per sample, dynamic work fetch, the whole path in "
                    "the workgroup, two state slots per resident workgroup) + k_fs_paths_sum",
           "batch_baseline": "gpis_fs_sample_distance_batch (k_fs_march) on the frame's valid primary rays from empty states, uploaded "
                             "beforehand; the call only.  Primary segments start unconditioned; the path frame's later segments are "
                             "conditioned and shorter, so the two rates are not of the same segment mix",
           "result": run(pkg, ref, a)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
