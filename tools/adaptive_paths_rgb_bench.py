"""Adaptive against uniform sampling of the RGB path driver (gpis_render_scene_s_paths_rgb_adaptive against
gpis_render_scene_s_paths_rgb at the same average spp): one JSON document on stdout, in the pattern of tools/adaptive_bench.py.

Per case (medium of tests/paths_rgb_ref.py: `grey` = C1 with a guide, `rust` = per-path realizations with an fp64 emission):
  (a) frame time of three legs timed in ONE process in alternating runs (host clock around the whole call with a device
      synchronisation on both sides — the adaptive entry synchronises per pass itself —, after a warm-up of each, best and all of
      --reps): the uniform entry; the uniform entry called once per pass of 16 spp, which has the adaptive entry's launch structure
      without its schedule; the adaptive entry.  The adaptive frame renders info.samples samples, not W*H*S;
  (b) the RMSE over the three channels of the uniform and of the adaptive image, each divided by its own counts, against a uniform
      image of --ref-spp samples per pixel drawn from sample indices neither frame uses.

    python tools/adaptive_paths_rgb_bench.py [--cases grey,rust] [--width 256 --height 256 --spp 64 --bounces 4] [--reps 5]
                                             [--ref-spp 1024] [--out profiles/r11_adaptive_paths_rgb_bench.json]
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

REF_BEGIN = 1 << 20          # first sample index of the reference image: far above any index the timed frames reach
LEGS = ("uniform", "uniform_in_passes", "adaptive")


def run_case(pkg, a, case):
    import torch
    import paths_rgb_ref as prr
    params, albedo, guided = prr.CASES[case](pkg)
    med = pkg.Medium(params)
    if guided:
        med.build_guide(*prr.GUIDE)
    width, height, spp = a.width, a.height, a.spp
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    npix = width * height
    d_rad = torch.zeros(3 * npix, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(npix, dtype=torch.int32, device=dev)
    adaptive = pkg.default_adaptive_s()
    step = int(adaptive["spp_step"])
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    alb = np.ascontiguousarray(albedo, dtype=np.float32)
    vp = ctypes.c_void_p
    lib = med.L.lib

    def scene_of(n, begin=0):
        s = pkg.default_scene_s(width, height, n)
        s["spp_begin"] = begin
        return s

    def frame(which, n, begin=0):
        """seconds of one frame into zeroed buffers"""
        s = scene_of(n, begin)
        d_rad.zero_()
        d_cnt.zero_()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if which == "adaptive":
            med.L.check(lib.gpis_render_scene_s_paths_rgb_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), a.bounces, vp(alb.ctypes.data),
                                                                   vp(d_rad.data_ptr()), vp(d_cnt.data_ptr()), None, None, vp(info.ctypes.data), sp),
                        "gpis_render_scene_s_paths_rgb_adaptive")
        elif which == "uniform_in_passes":
            for k0 in range(0, n, step):
                part = scene_of(min(step, n - k0), begin + k0)
                med.L.check(lib.gpis_render_scene_s_paths_rgb(med.h, vp(part.ctypes.data), a.bounces, vp(alb.ctypes.data), vp(d_rad.data_ptr()), None, sp),
                            "gpis_render_scene_s_paths_rgb")
        else:
            med.L.check(lib.gpis_render_scene_s_paths_rgb(med.h, vp(s.ctypes.data), a.bounces, vp(alb.ctypes.data), vp(d_rad.data_ptr()), None, sp),
                        "gpis_render_scene_s_paths_rgb")
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def image(which, n, begin=0):
        frame(which, n, begin)
        rad = d_rad.cpu().numpy().astype(np.float64).reshape(npix, 3)
        return rad / (d_cnt.cpu().numpy().astype(np.float64)[:, None] if which == "adaptive" else n)

    for w in LEGS + LEGS:                                          # warm-up: workspaces, code objects
        frame(w, spp)
    times = {w: [] for w in LEGS}
    for _ in range(a.reps):
        for w in LEGS:
            times[w].append(frame(w, spp))
    frame("adaptive", spp)                                         # once more, for its counts
    cnt = d_cnt.cpu().numpy()
    samples = {"uniform": npix * spp, "uniform_in_passes": npix * spp, "adaptive": int(info["samples"])}
    out = {"case": case, "guided": bool(guided), "width": width, "height": height, "spp": spp, "bounces": a.bounces, "reps": a.reps,
           "passes_rendered": int(info["passes_rendered"]), "stopped_early": int(info["stopped_early"])}
    for w in LEGS:
        best = min(times[w])
        out[w] = {"seconds_per_frame_best": best, "seconds_per_frame_all": times[w], "samples": samples[w], "samples_per_s": samples[w] / best}
    out["adaptive"]["samples_per_pixel"] = {"min": int(cnt.min()), "max": int(cnt.max()), "mean": float(cnt.mean())}
    out["adaptive_over_uniform_frame_time"] = out["adaptive"]["seconds_per_frame_best"] / out["uniform"]["seconds_per_frame_best"]
    out["adaptive_over_uniform_in_passes_frame_time"] = out["adaptive"]["seconds_per_frame_best"] / out["uniform_in_passes"]["seconds_per_frame_best"]

    ref = np.zeros((npix, 3))
    for k0 in range(0, a.ref_spp, 256):
        n = min(256, a.ref_spp - k0)
        ref += image("uniform", n, REF_BEGIN + k0) * n
    ref /= a.ref_spp

    def rmse(img):
        return float(np.sqrt(np.mean((img - ref) ** 2)))
    out["rmse"] = {"reference_spp": a.ref_spp, "uniform": rmse(image("uniform", spp)), "adaptive": rmse(image("adaptive", spp))}
    med.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="grey,rust")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    doc = {"workload": "scene S, RGB multi-bounce paths; adaptive = gpis_render_scene_s_paths_rgb_adaptive (spp_step 16, threshold 16), uniform = "
                       "gpis_render_scene_s_paths_rgb of the same build",
           "timing": "host clock around the whole call between device synchronisations, the three legs alternating in one process after two warm-up frames of each",
           "results": [run_case(pkg, a, c) for c in a.cases.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
