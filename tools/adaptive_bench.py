"""Adaptive against uniform sampling of the scene-S Lambert frame (gpis_render_scene_s_adaptive against gpis_render_scene_s at the same
average spp): one JSON document on stdout.

Per case (medium, frame size, S):
  (a) frame time of both entries — and of the uniform entry called once per pass of 16 spp, which has the adaptive entry's launch
      structure and first-pass sample layout without its schedule —, timed in ONE process in alternating runs (host clock around
      the whole call with a device synchronisation on both sides — the adaptive entry synchronises per pass itself —, after a
      warm-up of each, best and all of --reps) and samples per second; the adaptive frame renders info.samples samples, not W*H*S;
  (b) the RMSE of both images, each divided by its own counts, against a uniform image of --ref-spp samples per pixel drawn from
      sample indices neither frame uses, and the uniform spp that reaches the adaptive RMSE: estimated from the 1/N law of the
      uniform estimator's MSE and then measured at that spp;
  (c) per-pass times — the schedule is deterministic, so pass p is the frame at S = 16 (p+1) less the frame at S = 16 p — and the
      host plan step's time on the frame's final records.

    python tools/adaptive_bench.py [--cases c1:256x256x64,c1:1920x1080x64,c0:256x256x64] [--reps 5] [--ref-spp 1024]
                                   [--guide 16:64] [--out profiles/r10_adaptive_bench.json]
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

REF_BEGIN = 1 << 20          # first sample index of the reference image: far above any index the timed frames reach


def run_case(pkg, a, case):
    import torch
    cfg, shape = case.split(":")
    width, height, spp = (int(v) for v in shape.split("x"))
    med = pkg.Medium(pkg.params_for_config(cfg))
    guided = cfg.lower() == "c1"
    if guided:
        med.build_guide(*(int(v) for v in a.guide.split(":")))
    dev = torch.device("cuda", 0)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    npix = width * height
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(npix, dtype=torch.int32, device=dev)
    d_rec = torch.zeros(((width + 3) // 4) * ((height + 3) // 4) * pkg.ADAPTIVE_RECORD.itemsize, dtype=torch.uint8, device=dev)
    adaptive = pkg.default_adaptive_s()
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    vp = ctypes.c_void_p

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
            med.L.check(med.L.lib.gpis_render_scene_s_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), vp(d_rad.data_ptr()), vp(d_cnt.data_ptr()),
                                                               None, vp(d_rec.data_ptr()), vp(info.ctypes.data), sp), "gpis_render_scene_s_adaptive")
        elif which == "uniform_in_passes":      # the uniform frame cut into the adaptive entry's passes: spp_step samples per call
            for k0 in range(0, n, 16):
                part = scene_of(min(16, n - k0), begin + k0)
                med.L.check(med.L.lib.gpis_render_scene_s(med.h, vp(part.ctypes.data), vp(d_rad.data_ptr()), None, sp), "gpis_render_scene_s")
        else:
            med.L.check(med.L.lib.gpis_render_scene_s(med.h, vp(s.ctypes.data), vp(d_rad.data_ptr()), None, sp), "gpis_render_scene_s")
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def image(which, n, begin=0):
        frame(which, n, begin)
        rad = d_rad.cpu().numpy().astype(np.float64)
        return rad / (d_cnt.cpu().numpy().astype(np.float64) if which == "adaptive" else n)

    for w in ("uniform", "adaptive", "uniform", "adaptive"):       # warm-up: workspaces, code objects
        frame(w, spp)
    frame("uniform_in_passes", spp)
    times = {"uniform": [], "adaptive": [], "uniform_in_passes": []}
    for _ in range(a.reps):
        for w in times:
            times[w].append(frame(w, spp))
    frame("adaptive", spp)                                         # once more, for its counts and records
    samples_adaptive, passes = int(info["samples"]), int(info["passes_rendered"])
    out = {"case": case, "guided": guided, "reps": a.reps, "passes_rendered": passes, "stopped_early": int(info["stopped_early"]),
           "uniform": {"seconds_per_frame_best": min(times["uniform"]), "seconds_per_frame_all": times["uniform"], "samples": npix * spp},
           "adaptive": {"seconds_per_frame_best": min(times["adaptive"]), "seconds_per_frame_all": times["adaptive"], "samples": samples_adaptive},
           "uniform_in_passes": {"seconds_per_frame_best": min(times["uniform_in_passes"]), "seconds_per_frame_all": times["uniform_in_passes"], "samples": npix * spp}}
    for w in times:
        out[w]["samples_per_s"] = out[w]["samples"] / out[w]["seconds_per_frame_best"]
    out["adaptive_over_uniform_frame_time"] = out["adaptive"]["seconds_per_frame_best"] / out["uniform"]["seconds_per_frame_best"]
    cnt = d_cnt.cpu().numpy()
    out["adaptive"]["samples_per_pixel"] = {"min": int(cnt.min()), "max": int(cnt.max()), "mean": float(cnt.mean())}

    # (c) the plan step on the final records, and the passes by difference
    rec = d_rec.cpu().numpy().view(pkg.ADAPTIVE_RECORD).copy()
    plan = []
    for _ in range(3):
        r, st = rec.copy(), ctypes.c_uint64(med.L.lib.gpis_adaptive_rng_init_host(vp(adaptive.ctypes.data), width, height))
        t0 = time.perf_counter()
        rc = med.L.lib.gpis_adaptive_plan_host(vp(adaptive.ctypes.data), width, height, spp, 16, ctypes.byref(st), r.size, vp(r.ctypes.data))
        plan.append(time.perf_counter() - t0)
        assert rc in (0, 1)
    out["host_plan_seconds_best"] = min(plan)
    upto = [min(frame("adaptive", n) for _ in range(max(2, a.reps // 2))) for n in range(16, spp + 1, 16)]
    out["seconds_up_to_pass"] = upto
    out["seconds_per_pass"] = [upto[0]] + [b - x for x, b in zip(upto, upto[1:])]

    # (b) error against a long uniform image
    ref = np.zeros(npix)
    for k0 in range(0, a.ref_spp, 256):
        n = min(256, a.ref_spp - k0)
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
    ap.add_argument("--cases", default="c1:256x256x64,c1:1920x1080x64,c0:256x256x64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--guide", default="16:64", help="guide field of the c1 cases, half_extent_cells:points_per_cell (bench.py's headline guide)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    doc = {"guide": a.guide, "workload": "scene S, Lambert frame; adaptive = gpis_render_scene_s_adaptive (spp_step 16, threshold 16), uniform = gpis_render_scene_s of the "
                       "same build (its kernels and driver are those of the parent commit)",
           "timing": "host clock around the whole call between device synchronisations, alternating uniform / adaptive in one process after two warm-up frames of each",
           "results": [run_case(pkg, a, c) for c in a.cases.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
