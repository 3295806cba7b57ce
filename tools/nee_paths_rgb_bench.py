"""GPU-box measurement of the RGB conductor NEE / MIS path drivers (gpis_render_scene_s_nee_paths_rgb and its adaptive form) against
the mono entries they extend: one JSON document on stdout (and in --out), in the pattern of tools/nee_paths_bench.py and
tools/paths_adaptive_bench.py.

    python tools/nee_paths_rgb_bench.py [--config C2] [--width 256 --height 256 --spp 8] [--bounces 2,4,8] [--adaptive-spp 64]
                                        [--reps 9] [--out profiles/r21_nee_paths_rgb_bench.json]

Uniform, per max_path_bounces, on one frame of the copper surface (gpis_default_surface_rgb) and the mono surface of its channel 0:
the legs `mono` (gpis_render_scene_s_nee_paths once), `rgb` (the RGB entry once) and `mono_x3` (the mono entry once per channel's
surface: what a coloured conductor frame took before) — timed in ONE process in alternating runs, host clock around the calls
between device synchronisations, after two warm-up frames of each; median, best and all of --reps.  The rays of the three legs are
the same, so the segment counts (the handle's counters) must agree, and every channel of the RGB image must equal the mono image of
that channel's surface; both are checked and recorded.
Adaptive, per max_path_bounces at --adaptive-spp: the legs `uniform` (the RGB entry in one call), `uniform_in_passes` (the RGB entry
once per pass of 16 spp: the adaptive entry's launch structure without its schedule) and `adaptive`; the adaptive frame renders
info.samples samples, not W*H*S.
The device (name, architecture, compute units, the clock the runtime reports) is recorded with the numbers."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import _gpis_pkg  # noqa: E402


def _stats(ts):
    return {"seconds_per_frame_median": statistics.median(ts), "seconds_per_frame_best": min(ts), "seconds_per_frame_all": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", default="2,4,8")
    ap.add_argument("--adaptive-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = _gpis_pkg.load_package()
    med = pkg.Medium(pkg.params_for_config(a.config))
    lib, vp = med.L.lib, ctypes.c_void_p
    npix = a.width * a.height
    copper = np.array(pkg.default_surface_rgb(), dtype=pkg.SURFACE_RGB_S)
    mono = []
    for c in range(3):
        s = np.zeros((), dtype=pkg.SURFACE_S)
        for key in ("eta", "k", "albedo", "cap_radiance"):
            s[key] = copper[key][c]
        s["cap_cos"] = copper["cap_cos"]
        mono.append(s)
    d_rgb = torch.zeros(3 * npix, dtype=torch.float32, device="cuda")
    d_mono = [torch.zeros(npix, dtype=torch.float32, device="cuda") for _ in range(3)]
    d_cnt = torch.zeros(npix, dtype=torch.int32, device="cuda")
    adaptive = np.array(pkg.default_adaptive_s(), dtype=pkg.ADAPTIVE_S)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    sp = vp(torch.cuda.current_stream().cuda_stream)

    def scene(n, begin=0):
        s = np.array(pkg.default_scene_s(a.width, a.height, n), dtype=pkg.SCENE_S)
        s["spp_begin"] = begin
        return s

    def rgb_call(s, bounces):
        med.L.check(lib.gpis_render_scene_s_nee_paths_rgb(med.h, vp(s.ctypes.data), vp(copper.ctypes.data), bounces, vp(d_rgb.data_ptr()), None, sp),
                    "gpis_render_scene_s_nee_paths_rgb")

    def frame(leg, bounces, n):
        """(seconds, segments) of one frame of `leg` into zeroed buffers"""
        s = scene(n)
        d_rgb.zero_()
        d_cnt.zero_()
        for t in d_mono:
            t.zero_()
        med.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg in ("mono", "mono_x3"):
            for c in range(1 if leg == "mono" else 3):
                med.L.check(lib.gpis_render_scene_s_nee_paths(med.h, vp(s.ctypes.data), vp(mono[c].ctypes.data), bounces, vp(d_mono[c].data_ptr()), None, sp),
                            "gpis_render_scene_s_nee_paths")
        elif leg in ("rgb", "uniform"):
            rgb_call(s, bounces)
        elif leg == "uniform_in_passes":
            step = int(adaptive["spp_step"])
            for k0 in range(0, n, step):
                rgb_call(scene(min(step, n - k0), k0), bounces)
        else:
            med.L.check(lib.gpis_render_scene_s_nee_paths_rgb_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), vp(copper.ctypes.data), bounces,
                                                                       vp(d_rgb.data_ptr()), vp(d_cnt.data_ptr()), None, None, vp(info.ctypes.data), sp),
                        "gpis_render_scene_s_nee_paths_rgb_adaptive")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, med.counters()[1]

    def timed(legs, bounces, n):
        for leg in legs + legs:                                        # warm-up: workspaces, code objects
            frame(leg, bounces, n)
        times, segs = {leg: [] for leg in legs}, {}
        for _ in range(a.reps):
            for leg in legs:                                           # alternating, so that a busy host touches every leg alike
                dt, segs[leg] = frame(leg, bounces, n)
                times[leg].append(dt)
        return times, segs

    prop = torch.cuda.get_device_properties(0)
    doc = {"workload": "scene-S conductor NEE/MIS paths %s %dx%d, copper (gpis_default_surface_rgb) against the mono surfaces of its channels" % (a.config, a.width, a.height),
           "timing": "host clock around the calls of a leg between device synchronisations, the legs alternating in one process after two warm-up frames of each; "
                     "medians of --reps frames",
           "device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                      "clock_rate_khz": getattr(prop, "clock_rate", None), "note": "one device, one session; clocks as the runtime reports them, not pinned"},
           "reps": a.reps, "uniform": [], "adaptive": []}
    bounces_list = [int(b) for b in a.bounces.split(",")]
    legs = ("mono", "rgb", "mono_x3")
    for b in bounces_list:
        times, segs = timed(legs, b, a.spp)
        frame("mono_x3", b, a.spp)
        want = [t.cpu().numpy() for t in d_mono]
        frame("rgb", b, a.spp)
        got = d_rgb.cpu().numpy().reshape(npix, 3)
        row = {"max_path_bounces": b, "spp": a.spp, "samples": npix * a.spp, "segments": {leg: int(segs[leg]) for leg in legs},
               "same_segments": bool(segs["rgb"] == segs["mono"] and segs["mono_x3"] == 3 * segs["mono"]),
               "channels_equal_mono": [bool(np.array_equal(got[:, c].view(np.uint32), want[c].view(np.uint32))) for c in range(3)],
               "image_sum": [float(got[:, c].sum()) for c in range(3)]}
        for leg in legs:
            row[leg] = _stats(times[leg])
        m = {leg: row[leg]["seconds_per_frame_median"] for leg in legs}
        row["rgb_over_mono_frame_time"] = m["rgb"] / m["mono"]
        row["rgb_over_mono_x3_frame_time"] = m["rgb"] / m["mono_x3"]
        row["rgb_Msegments_per_s"] = segs["rgb"] / m["rgb"] / 1e6
        doc["uniform"].append(row)
    legs = ("uniform", "uniform_in_passes", "adaptive")
    for b in bounces_list:
        n = a.adaptive_spp
        times, _ = timed(legs, b, n)
        frame("adaptive", b, n)
        cnt = d_cnt.cpu().numpy()
        samples = {"uniform": npix * n, "uniform_in_passes": npix * n, "adaptive": int(info["samples"])}
        row = {"max_path_bounces": b, "spp": n, "passes_rendered": int(info["passes_rendered"]), "stopped_early": int(info["stopped_early"]),
               "samples_per_pixel": {"min": int(cnt.min()), "max": int(cnt.max()), "mean": float(cnt.mean())}}
        for leg in legs:
            row[leg] = _stats(times[leg])
            row[leg]["samples"] = samples[leg]
            row[leg]["Msamples_per_s_median"] = samples[leg] / row[leg]["seconds_per_frame_median"] / 1e6
        m = {leg: row[leg]["seconds_per_frame_median"] for leg in legs}
        row["adaptive_over_uniform_frame_time"] = m["adaptive"] / m["uniform"]
        row["adaptive_over_uniform_in_passes_frame_time"] = m["adaptive"] / m["uniform_in_passes"]
        row["uniform_in_passes_over_uniform_frame_time"] = m["uniform_in_passes"] / m["uniform"]
        doc["adaptive"].append(row)
    med.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
