"""Adaptive against uniform sampling of the mono path drivers (gpis_render_scene_s_nee_paths_adaptive against
gpis_render_scene_s_nee_paths, gpis_render_scene_s_paths_adaptive against gpis_render_scene_s_paths, at the same average spp): one
JSON document on stdout, in the pattern of tools/adaptive_paths_rgb_bench.py.

Per case (`nee2`, `nee4`: C2 through the NEE entry at 2 and 4 bounces; `lambert4`: C1 with a guide through the Lambert entry at 4):
  (a) frame time of three legs timed in ONE process in alternating runs (host clock around the whole call with a device
      synchronisation on both sides — the adaptive entry synchronises per pass itself —, after a warm-up of each; median, best and
      all of --reps): the uniform entry; the uniform entry called once per pass of 16 spp, which has the adaptive entry's launch
      structure without its schedule; the adaptive entry.  The adaptive frame renders info.samples samples, not W*H*S;
  (b) the RMSE of the uniform and of the adaptive image, each divided by its own counts, against a uniform image of --ref-spp
      samples per pixel rendered with another scene_seed; the RMSE of uniform frames at other spp, and from them (log-log
      interpolation between the two neighbours) the uniform spp whose RMSE is the adaptive frame's.
With --uniform-only only the uniform entries of the cases are timed — and, for `nee2`, gpis_render_scene_s_nee — and a checksum of
each image is printed; --tree PATH takes the package and its library from another built checkout of the project (the parent
commit's), so that a script can alternate the two trees on one box.

    python tools/paths_adaptive_bench.py [--cases nee2,nee4,lambert4] [--width 256 --height 256 --spp 64] [--reps 9]
                                         [--ref-spp 1024] [--uniform-only [--tree PATH]] [--out profiles/r18_paths_adaptive_bench.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REF_SEED = 0x5EED5EED        # scene_seed of the reference image
LEGS = ("uniform", "uniform_in_passes", "adaptive")
ALBEDO = 0.8
GUIDE = (16, 8)
CASES = {"nee2": ("C2", "nee", 2), "nee4": ("C2", "nee", 4), "lambert4": ("C1", "lambert", 4)}
UNIFORM_SPP = (32, 48, 64, 96, 128)


def _stats(ts):
    return {"seconds_per_frame_median": statistics.median(ts), "seconds_per_frame_best": min(ts), "seconds_per_frame_all": ts}


class Driver:
    """the entries of one case on one library"""

    def __init__(self, pkg, lib, config, kind, bounces, width, height):
        import torch
        self.pkg, self.kind, self.bounces, self.width, self.height = pkg, kind, bounces, width, height
        self.med = pkg.Medium(pkg.params_for_config(config), lib=lib)
        if kind == "lambert":
            self.med.build_guide(*GUIDE)
        self.surf = np.array(pkg.default_surface_s(), dtype=pkg.SURFACE_S)
        self.dev = torch.device("cuda", 0)
        self.sp = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.npix = width * height
        self.d_rad = torch.zeros(self.npix, dtype=torch.float32, device=self.dev)
        self.d_cnt = torch.zeros(self.npix, dtype=torch.int32, device=self.dev)
        self.adaptive = pkg.default_adaptive_s()
        self.info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)

    def scene(self, n, begin=0, seed=None):
        s = self.pkg.default_scene_s(self.width, self.height, n)
        s["spp_begin"] = begin
        if seed is not None:
            s["scene_seed"] = seed
        return s

    def uniform(self, s, single=False):
        med, lib, vp = self.med, self.med.L.lib, ctypes.c_void_p
        if single:
            med.L.check(lib.gpis_render_scene_s_nee(med.h, vp(s.ctypes.data), vp(self.surf.ctypes.data), vp(self.d_rad.data_ptr()), self.sp), "gpis_render_scene_s_nee")
        elif self.kind == "nee":
            med.L.check(lib.gpis_render_scene_s_nee_paths(med.h, vp(s.ctypes.data), vp(self.surf.ctypes.data), self.bounces, vp(self.d_rad.data_ptr()), None, self.sp),
                        "gpis_render_scene_s_nee_paths")
        else:
            med.L.check(lib.gpis_render_scene_s_paths(med.h, vp(s.ctypes.data), self.bounces, ctypes.c_float(ALBEDO), vp(self.d_rad.data_ptr()), self.sp),
                        "gpis_render_scene_s_paths")

    def frame(self, which, n, begin=0, seed=None):
        """seconds of one frame into zeroed buffers"""
        import torch
        med, lib, vp = self.med, self.med.L.lib, ctypes.c_void_p
        s = self.scene(n, begin, seed)
        self.d_rad.zero_()
        self.d_cnt.zero_()
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        if which == "adaptive" and self.kind == "nee":
            med.L.check(lib.gpis_render_scene_s_nee_paths_adaptive(med.h, vp(s.ctypes.data), vp(self.adaptive.ctypes.data), vp(self.surf.ctypes.data), self.bounces,
                                                                   vp(self.d_rad.data_ptr()), vp(self.d_cnt.data_ptr()), None, None, vp(self.info.ctypes.data), self.sp),
                        "gpis_render_scene_s_nee_paths_adaptive")
        elif which == "adaptive":
            med.L.check(lib.gpis_render_scene_s_paths_adaptive(med.h, vp(s.ctypes.data), vp(self.adaptive.ctypes.data), self.bounces, ctypes.c_float(ALBEDO),
                                                               vp(self.d_rad.data_ptr()), vp(self.d_cnt.data_ptr()), None, vp(self.info.ctypes.data), self.sp),
                        "gpis_render_scene_s_paths_adaptive")
        elif which == "uniform_in_passes":
            step = int(self.adaptive["spp_step"])
            for k0 in range(0, n, step):
                self.uniform(self.scene(min(step, n - k0), begin + k0, seed))
        else:
            self.uniform(s, single=(which == "single"))
        torch.cuda.synchronize(self.dev)
        return time.perf_counter() - t0

    def image(self, which, n, begin=0, seed=None):
        self.frame(which, n, begin, seed)
        rad = self.d_rad.cpu().numpy().astype(np.float64)
        return rad / (self.d_cnt.cpu().numpy().astype(np.float64) if which == "adaptive" else n)

    def raw(self, which, n):
        self.frame(which, n)
        return self.d_rad.cpu().numpy().copy()


def matched_spp(rmse_by_spp, target):
    """the uniform spp whose RMSE is `target`: log-log interpolation between the two neighbours, extrapolation with the slope of the
    nearest pair outside the measured range"""
    pts = sorted((np.log(n), np.log(r)) for n, r in rmse_by_spp.items())
    t = np.log(target)
    pair = (pts[0], pts[1]) if t >= pts[0][1] else (pts[-2], pts[-1])
    for a, b in zip(pts, pts[1:]):
        if b[1] <= t <= a[1]:
            pair = (a, b)
            break
    (x0, y0), (x1, y1) = pair
    return float(np.exp(x0 + (t - y0) * (x1 - x0) / (y1 - y0)))


def run_uniform_only(pkg, a, case):
    """the uniform entries of the case alone: what a checkout without the adaptive entries can run too"""
    config, kind, bounces = CASES[case]
    d = Driver(pkg, None, config, kind, bounces, a.width, a.height)
    out = {"case": case, "config": config, "width": a.width, "height": a.height, "spp": a.spp, "bounces": bounces, "reps": a.reps, "entries": {}}
    for leg in (("uniform", "single") if case == "nee2" else ("uniform",)):
        name = "gpis_render_scene_s_nee" if leg == "single" else ("gpis_render_scene_s_nee_paths" if kind == "nee" else "gpis_render_scene_s_paths")
        for _ in range(2):
            d.frame(leg, a.spp)
        res = _stats([d.frame(leg, a.spp) for _ in range(a.reps)])
        res["image_sha256"] = hashlib.sha256(d.raw(leg, a.spp).tobytes()).hexdigest()
        out["entries"][name] = res
    d.med.close()
    return out


def run_case(pkg, a, case):
    config, kind, bounces = CASES[case]
    d = Driver(pkg, None, config, kind, bounces, a.width, a.height)
    spp, npix = a.spp, a.width * a.height
    for w in LEGS + LEGS:                                          # warm-up: workspaces, code objects
        d.frame(w, spp)
    times = {w: [] for w in LEGS}
    for _ in range(a.reps):
        for w in LEGS:
            times[w].append(d.frame(w, spp))
    d.frame("adaptive", spp)                                       # once more, for its counts
    cnt = d.d_cnt.cpu().numpy()
    info = d.info
    samples = {"uniform": npix * spp, "uniform_in_passes": npix * spp, "adaptive": int(info["samples"])}
    out = {"case": case, "config": config, "entry": "gpis_render_scene_s_nee_paths" if kind == "nee" else "gpis_render_scene_s_paths", "guided": kind == "lambert",
           "width": a.width, "height": a.height, "spp": spp, "bounces": bounces, "reps": a.reps, "passes_rendered": int(info["passes_rendered"]),
           "stopped_early": int(info["stopped_early"])}
    for w in LEGS:
        out[w] = _stats(times[w])
        out[w]["samples"] = samples[w]
        out[w]["samples_per_s_median"] = samples[w] / out[w]["seconds_per_frame_median"]
    out["adaptive"]["samples_per_pixel"] = {"min": int(cnt.min()), "max": int(cnt.max()), "mean": float(cnt.mean())}
    med = {w: out[w]["seconds_per_frame_median"] for w in LEGS}
    out["adaptive_over_uniform_frame_time"] = med["adaptive"] / med["uniform"]
    out["adaptive_over_uniform_in_passes_frame_time"] = med["adaptive"] / med["uniform_in_passes"]
    out["uniform_in_passes_over_uniform_frame_time"] = med["uniform_in_passes"] / med["uniform"]

    ref = np.zeros(npix)
    for k0 in range(0, a.ref_spp, 256):
        n = min(256, a.ref_spp - k0)
        ref += d.image("uniform", n, k0, REF_SEED) * n
    ref /= a.ref_spp

    # a sample of the NEE estimator can be non-finite (the adaptive entry's clamp counts it as 0, the uniform entry adds it): such
    # pixels are counted and left out of every RMSE, the reference's in all of them
    bad = {"reference": int((~np.isfinite(ref)).sum())}

    def rmse(name, img):
        ok = np.isfinite(ref) & np.isfinite(img)
        bad[name] = int((~np.isfinite(img)).sum())
        return float(np.sqrt(np.mean((img[ok] - ref[ok]) ** 2)))
    by_spp = {n: rmse("uniform_%d" % n, d.image("uniform", n)) for n in sorted(set(UNIFORM_SPP) | {spp})}
    r_adaptive = rmse("adaptive", d.image("adaptive", spp))
    out["rmse"] = {"reference_spp": a.ref_spp, "reference_scene_seed": REF_SEED, "uniform": by_spp[spp], "adaptive": r_adaptive,
                   "uniform_by_spp": {str(n): r for n, r in by_spp.items()}, "uniform_spp_of_the_adaptive_rmse": matched_spp(by_spp, r_adaptive),
                   "non_finite_pixels": bad}
    d.med.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="nee2,nee4,lambert4")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--uniform-only", action="store_true", help="time the uniform entries of the cases alone")
    ap.add_argument("--tree", default=ROOT, help="--uniform-only: the built checkout of the project to load the package from (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if tree != ROOT and not a.uniform_only:
        ap.error("--tree goes with --uniform-only")
    sys.path.insert(0, tree)
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    if a.uniform_only:
        doc = {"workload": "scene S, the uniform mono path entries", "library": os.path.relpath(pkg.library_path(), ROOT),
               "timing": "host clock around the whole call between device synchronisations after two warm-up frames; medians of --reps frames",
               "results": [run_uniform_only(pkg, a, c) for c in a.cases.split(",")]}
    else:
        doc = _adaptive_doc(pkg, a)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def _adaptive_doc(pkg, a):
    return {"workload": "scene S, mono multi-bounce paths; adaptive = gpis_render_scene_s_nee_paths_adaptive / gpis_render_scene_s_paths_adaptive (spp_step 16, "
                       "threshold 16), uniform = gpis_render_scene_s_nee_paths / gpis_render_scene_s_paths of the same build",
           "timing": "host clock around the whole call between device synchronisations, the legs alternating in one process after two warm-up frames of each; "
                     "medians of --reps frames",
           "results": [run_case(pkg, a, c) for c in a.cases.split(",")]}


if __name__ == "__main__":
    main()
