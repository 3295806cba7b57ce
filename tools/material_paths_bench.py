"""GPU-box measurement of the RGB path drivers whose material is chosen per hit by the GP id
(gpis_render_scene_s_material_paths_rgb and its adaptive form): one JSON document on stdout (and in --out), in the pattern of
tools/nee_paths_rgb_bench.py.

    python tools/material_paths_bench.py [--config C2] [--width 256 --height 256 --spp 8] [--bounces 2,4,8] [--adaptive-spp 64]
                                         [--reps 9] [--out profiles/r22_material_paths_bench.json]

The medium is --config made CSG: the minimum of its mean and a sphere of radius 0.6 at (0.55, 0.35, 0.6), so hits carry both ids.
Uniform, per max_path_bounces, the legs `conductor` (gpis_render_scene_s_nee_paths_rgb with copper), `all_copper` (the new entry
with a table of two coppers: the same launches and segments, so the ratio of the two is the cost of the per-lane switch; images and
segment counts must be equal, which is checked and recorded) and `copper_lambert` (gpis_default_materials: segments per second) —
timed in ONE process in alternating runs, host clock around the calls between device synchronisations, after two warm-up frames of
each; median, best and all of --reps.
Adaptive, per max_path_bounces at --adaptive-spp with gpis_default_materials: the legs `uniform` (the new entry in one call),
`uniform_in_passes` (once per pass of 16 spp: the adaptive entry's launch structure without its schedule) and `adaptive`; the
adaptive frame renders info.samples samples, not W*H*S.
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
    params = pkg.params_for_config(a.config)
    params["has_mean_additional"] = 1
    extra = params["mean_additional"]
    extra["type"], extra["center"], extra["radius"] = pkg.MEAN_TYPE.SPHERICAL, (0.55, 0.35, 0.6), 0.6
    med = pkg.Medium(params)
    lib, vp = med.L.lib, ctypes.c_void_p
    npix = a.width * a.height
    copper = np.array(pkg.default_surface_rgb(), dtype=pkg.SURFACE_RGB_S)
    mixed = np.array(pkg.default_materials(), dtype=pkg.MATERIALS_S)
    coppers = mixed.copy()
    coppers["material"][1] = coppers["material"][0]
    d_rgb = torch.zeros(3 * npix, dtype=torch.float32, device="cuda")
    d_seg = torch.zeros(npix, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(npix, dtype=torch.int32, device="cuda")
    adaptive = np.array(pkg.default_adaptive_s(), dtype=pkg.ADAPTIVE_S)
    info = np.zeros((), dtype=pkg.ADAPTIVE_INFO)
    sp = vp(torch.cuda.current_stream().cuda_stream)

    def scene(n, begin=0):
        s = np.array(pkg.default_scene_s(a.width, a.height, n), dtype=pkg.SCENE_S)
        s["spp_begin"] = begin
        return s

    def mat_call(s, table, bounces):
        med.L.check(lib.gpis_render_scene_s_material_paths_rgb(med.h, vp(s.ctypes.data), vp(table.ctypes.data), bounces, vp(d_rgb.data_ptr()),
                                                               vp(d_seg.data_ptr()), sp), "gpis_render_scene_s_material_paths_rgb")

    def frame(leg, bounces, n):
        """(seconds, segments) of one frame of `leg` into zeroed buffers"""
        s = scene(n)
        d_rgb.zero_()
        d_seg.zero_()
        d_cnt.zero_()
        med.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "conductor":
            med.L.check(lib.gpis_render_scene_s_nee_paths_rgb(med.h, vp(s.ctypes.data), vp(copper.ctypes.data), bounces, vp(d_rgb.data_ptr()),
                                                              vp(d_seg.data_ptr()), sp), "gpis_render_scene_s_nee_paths_rgb")
        elif leg == "all_copper":
            mat_call(s, coppers, bounces)
        elif leg in ("copper_lambert", "uniform"):
            mat_call(s, mixed, bounces)
        elif leg == "uniform_in_passes":
            step = int(adaptive["spp_step"])
            for k0 in range(0, n, step):
                mat_call(scene(min(step, n - k0), k0), mixed, bounces)
        else:
            med.L.check(lib.gpis_render_scene_s_material_paths_rgb_adaptive(med.h, vp(s.ctypes.data), vp(adaptive.ctypes.data), vp(mixed.ctypes.data), bounces,
                                                                            vp(d_rgb.data_ptr()), vp(d_cnt.data_ptr()), None, None, vp(info.ctypes.data), sp),
                        "gpis_render_scene_s_material_paths_rgb_adaptive")
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
    doc = {"workload": "scene-S RGB paths, %s made CSG (sphere of radius 0.6 at (0.55, 0.35, 0.6)), %dx%d: the conductor entry against the material "
                       "entry with two coppers, and copper + Lambert (gpis_default_materials)" % (a.config, a.width, a.height),
           "timing": "host clock around the calls of a leg between device synchronisations, the legs alternating in one process after two warm-up frames of each; "
                     "medians of --reps frames",
           "device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                      "clock_rate_khz": getattr(prop, "clock_rate", None), "note": "one device, one session; clocks as the runtime reports them, not pinned"},
           "reps": a.reps, "uniform": [], "adaptive": []}
    bounces_list = [int(b) for b in a.bounces.split(",")]
    legs = ("conductor", "all_copper", "copper_lambert")
    for b in bounces_list:
        times, segs = timed(legs, b, a.spp)
        frame("conductor", b, a.spp)
        want, want_seg = d_rgb.cpu().numpy().copy(), d_seg.cpu().numpy().copy()
        frame("all_copper", b, a.spp)
        got, got_seg = d_rgb.cpu().numpy(), d_seg.cpu().numpy()
        row = {"max_path_bounces": b, "spp": a.spp, "samples": npix * a.spp, "segments": {leg: int(segs[leg]) for leg in legs},
               "all_copper_equals_conductor": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_seg, want_seg)
                                                   and segs["all_copper"] == segs["conductor"])}
        for leg in legs:
            row[leg] = _stats(times[leg])
        m = {leg: row[leg]["seconds_per_frame_median"] for leg in legs}
        row["all_copper_over_conductor_frame_time"] = m["all_copper"] / m["conductor"]
        row["copper_lambert_over_conductor_frame_time"] = m["copper_lambert"] / m["conductor"]
        for leg in legs:
            row[leg + "_Msegments_per_s"] = segs[leg] / m[leg] / 1e6
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
