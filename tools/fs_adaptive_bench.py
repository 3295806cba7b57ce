"""Adaptive against uniform sampling through the function-space GP medium (gpis_fs_render_scene_s_adaptive against
gpis_fs_render_scene_s, gpis_fs_render_scene_s_paths_adaptive against gpis_fs_render_scene_s_paths, at the same average spp): one
JSON document on stdout.  The pattern is tools/ws_adaptive_bench.py's.

Per driver (lambert, paths), one frame of scene S through the medium of tools/fs_scene_bench.py (Renewal+, 32 sample points, step
0.02):
  (a) frame time of the adaptive entry, of the uniform driver, and of the uniform driver called once per pass of 16 spp — the
      adaptive entry's launch structure without its schedule, which separates the cost of cutting a frame into passes from the
      cost of the schedule —, timed in ONE process in alternating runs (host clock around the whole call between device
      synchronisations, after a warm-up of each, best and all of --reps); the adaptive frame renders info.samples samples;
  (b) what the frames marched: the path driver's seg_count (path plus shadow segments) summed over the image; the frame driver
      exposes hits only, so its cost ratio is given in samples and hits (segments per sample are not counted by the entry);
  (c) the RMSE of both images, each divided by its own counts, against a uniform image of --ref-spp samples per pixel drawn from
      sample indices neither frame uses, and the uniform spp that reaches the adaptive RMSE: estimated from the 1/N law of the
      uniform estimator's MSE and then measured at that spp.

    python tools/fs_adaptive_bench.py [--width 128 --height 128 --spp 64] [--reps 3] [--ref-spp 512] [--bounces 3]
                                      [--out profiles/r19_fs_adaptive_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _gpis_pkg  # noqa: E402
import fs_scene_ref  # noqa: E402

REF_BEGIN = 1 << 20          # first sample index of the reference image: far above any index the timed frames reach


def run_case(pkg, a, driver):
    import torch
    med = pkg.Medium(fs_scene_ref.fs_params(pkg, a.ctx, a.points, a.step))
    L = med.L.lib
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    width, height, spp = a.width, a.height, a.spp
    npix = width * height
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(npix, dtype=torch.int32, device=dev)
    d_aux = torch.zeros(npix, dtype=torch.int32, device=dev)         # hit_count (lambert) / seg_count (paths)
    adaptive = pkg.default_adaptive_s()
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p
    albedo = ctypes.c_float(a.albedo)

    def scene_of(n, begin=0):
        s = pkg.default_scene_s(width, height, n)
        s["spp_begin"] = begin
        return s

    def uniform(s):
        if driver == "lambert":
            med.L.check(L.gpis_fs_render_scene_s(med.h, vp(s.ctypes.data), vp(d_rad.data_ptr()), vp(d_aux.data_ptr()), sp), "gpis_fs_render_scene_s")
        else:
            med.L.check(L.gpis_fs_render_scene_s_paths(med.h, vp(s.ctypes.data), a.bounces, albedo, vp(d_rad.data_ptr()), vp(d_aux.data_ptr()), sp),
                        "gpis_fs_render_scene_s_paths")

    def frame(which, n, begin=0):
        """seconds of one frame into zeroed buffers"""
        s = scene_of(n, begin)
        d_rad.zero_()
        d_cnt.zero_()
        d_aux.zero_()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if which == "adaptive" and driver == "lambert":
            med.L.check(L.gpis_fs_render_scene_s_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), vp(d_rad.data_ptr()), vp(d_cnt.data_ptr()),
                                                          vp(d_aux.data_ptr()), None, vp(info.ctypes.data), sp), "gpis_fs_render_scene_s_adaptive")
        elif which == "adaptive":
            med.L.check(L.gpis_fs_render_scene_s_paths_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), a.bounces, albedo, vp(d_rad.data_ptr()),
                                                                vp(d_cnt.data_ptr()), vp(d_aux.data_ptr()), None, vp(info.ctypes.data), sp),
                        "gpis_fs_render_scene_s_paths_adaptive")
        elif which == "uniform_in_passes":      # the uniform frame cut into the adaptive entry's passes: spp_step samples per call
            for k0 in range(0, n, 16):
                uniform(scene_of(min(16, n - k0), begin + k0))
        else:
            uniform(s)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def image(which, n, begin=0):
        frame(which, n, begin)
        rad = d_rad.cpu().numpy().astype(np.float64)
        return rad / (d_cnt.cpu().numpy().astype(np.float64) if which == "adaptive" else n)

    times = {"uniform": [], "adaptive": [], "uniform_in_passes": []}
    for which in times:                                              # warm-up: workspaces, code objects
        frame(which, 16)
    for _ in range(a.reps):
        for which in times:
            times[which].append(frame(which, spp))
    frame("adaptive", spp)                                           # once more, for its counts
    cnt = d_cnt.cpu().numpy()
    aux_adaptive = int(d_aux.cpu().numpy().astype(np.int64).sum())
    samples_adaptive = int(info["samples"])
    frame("uniform", spp)
    aux_uniform = int(d_aux.cpu().numpy().astype(np.int64).sum())
    aux = "hits" if driver == "lambert" else "segments"
    out = {"driver": driver, "context": a.ctx, "fs_sample_points": a.points, "fs_step_size": a.step, "frame": "%dx%dx%d" % (width, height, spp), "reps": a.reps,
           "passes_rendered": int(info["passes_rendered"]), "stopped_early": int(info["stopped_early"]),
           "uniform": {"samples": npix * spp, aux: aux_uniform},
           "adaptive": {"samples": samples_adaptive, aux: aux_adaptive,
                        "samples_per_pixel": {"min": int(cnt.min()), "max": int(cnt.max()), "mean": float(cnt.mean())}},
           "uniform_in_passes": {"samples": npix * spp}}
    if driver == "paths":
        out["max_bounces"], out["albedo"] = a.bounces, a.albedo
    for which in times:
        out[which]["seconds_per_frame_best"], out[which]["seconds_per_frame_all"] = min(times[which]), times[which]
        out[which]["samples_per_s"] = out[which]["samples"] / min(times[which])
    out["adaptive_over_uniform_frame_time"] = min(times["adaptive"]) / min(times["uniform"])
    out["uniform_in_passes_over_uniform_frame_time"] = min(times["uniform_in_passes"]) / min(times["uniform"])
    out["adaptive_over_uniform_samples"] = samples_adaptive / (npix * spp)
    out["adaptive_over_uniform_" + aux] = aux_adaptive / max(aux_uniform, 1)

    # (c) error against a long uniform image
    ref = np.zeros(npix)
    for k0 in range(0, a.ref_spp, 64):
        n = min(64, a.ref_spp - k0)
        ref += image("uniform", n, REF_BEGIN + k0) * n
    ref /= a.ref_spp

    def rmse(img):
        return float(np.sqrt(np.mean((img - ref) ** 2)))
    e_u, e_a = rmse(image("uniform", spp)), rmse(image("adaptive", spp))
    # the reference's own error adds to both: MSE_measured = MSE + var_ref, var_ref = MSE_uniform(S) * S / ref_spp (1/N law)
    var_ref = e_u ** 2 * spp / (a.ref_spp + spp)
    mse_u, mse_a = e_u ** 2 - var_ref, max(e_a ** 2 - var_ref, 1e-300)
    need = spp * mse_u / mse_a
    out["rmse"] = {"reference_spp": a.ref_spp, "uniform": e_u, "adaptive": e_a, "uniform_spp_for_adaptive_rmse_estimated": need,
                   "note": "estimate: uniform MSE ~ 1/N after subtracting the reference image's own variance from both"}
    n_meas = int(round(need))
    if 1 <= n_meas <= 4 * spp:
        out["rmse"]["uniform_at_estimated_spp"] = {"spp": n_meas, "rmse": rmse(image("uniform", n_meas))}
    med.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ctx", default="RENEWAL_PLUS")
    ap.add_argument("--points", type=int, default=32)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--albedo", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--drivers", default="lambert,paths")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = _gpis_pkg.load_package()
    doc = {"workload": "scene S (camera z = 4, fov 35, bounding radius 1.5, light (0.5, 0.7, 0.5)) through the function-space GP medium, spherical mean "
                       "r = 1 (C0-like: sigma 0.1, l 0.05); adaptive = the *_adaptive entry (spp_step 16, threshold 16, default chunk), uniform = the "
                       "uniform driver of the same build at the same average spp",
           "timing": "host clock around the whole call between device synchronisations, alternating uniform / adaptive / uniform in passes in one "
                     "process after a warm-up frame of each",
           "results": []}
    for driver in a.drivers.split(","):
        doc["results"].append(run_case(pkg, a, driver))
        if a.out:                                                # keep what is measured so far
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
