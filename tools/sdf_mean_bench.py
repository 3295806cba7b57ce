"""Frame time of a medium with a procedural SDF mean (GPIS_MEAN_PROCEDURAL) against the unit sphere: one JSON document on stdout.

Two frames per medium: 256 x 256 x 8 of gpis_render_scene_s (Lambert, one segment plus a shadow ray per sample) and a 4-bounce
frame of gpis_render_scene_s_paths_rgb.  Media are C0-like (world space, rho = 8), in two variants: single realization and per-path
Renewal.  Three means each:

    sphere          the spherical mean as it routes today (single realization: the fast / cooperative kernels; Renewal: spec_3d)
    sphere-generic  the SAME surface forced through the all-features instance: the CSG minimum of the spherical mean and a `plane`
                    procedural mean with offset = 100, which never wins.  The step from `sphere` is the cost of the generic instance.
    knob            the knob.  The step from `sphere-generic` is the cost of the SDF (and of a different surface).

`sphere` and `sphere-generic` must give the same image (bit for bit on the per-path media); the tool asserts it.  Timing: device events around the whole
driver call, media alternating in one process after a warm-up frame of each, best and all of --reps.

    python tools/sdf_mean_bench.py [--width 256 --height 256 --spp 8 --bounces 4] [--reps 5] [--out profiles/r14_sdf_mean_bench.json]
    python tools/sdf_mean_bench.py --headline '<json line of bench.py>' --headline-parent '<json line>' --out ...   # adds the two lines (no GPU)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALBEDO = (0.8, 0.6, 0.4)
MEANS = ("sphere", "sphere-generic", "knob")
VARIANTS = ("single-realization", "renewal")


def medium_params(pkg, variant, mean):
    p = pkg.params_for_config("C0")
    if variant == "renewal":
        p["single_realization"] = 0
        p["correlation_context"] = pkg.CTX.RENEWAL
    if mean == "knob":
        p["mean"]["type"] = pkg.MEAN_TYPE.PROCEDURAL
        p["mean"]["func"] = pkg.SDF_FUNCTION.KNOB
        p["mean"]["scale"], p["mean"]["offset"] = 1.0, 0.0
        p["mean"]["min"] = -np.finfo(np.float32).max
    elif mean == "sphere-generic":
        p["has_mean_additional"] = 1
        a = p["mean_additional"]
        a["type"], a["func"] = pkg.MEAN_TYPE.PROCEDURAL, pkg.SDF_FUNCTION.PLANE
        a["scale"], a["offset"], a["min"] = 1.0, 100.0, -np.finfo(np.float32).max
    return p


def run_variant(pkg, a, variant):
    import torch
    scene = np.array(pkg.default_scene_s(a.width, a.height, a.spp), dtype=pkg.SCENE_S).reshape(())
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    npix = a.width * a.height
    alb = np.array(ALBEDO, dtype=np.float32)
    media = {m: pkg.Medium(medium_params(pkg, variant, m)) for m in MEANS}
    d_mono = {m: torch.zeros(npix, dtype=torch.float32, device=dev) for m in MEANS}
    d_rgb = {m: torch.zeros(3 * npix, dtype=torch.float32, device=dev) for m in MEANS}

    def frame(kind, m):
        h = media[m]
        if kind == "lambert":
            h.L.check(h.L.lib.gpis_render_scene_s(h.h, scene_p, ctypes.c_void_p(d_mono[m].data_ptr()), None, sp), "gpis_render_scene_s")
        else:
            h.L.check(h.L.lib.gpis_render_scene_s_paths_rgb(h.h, scene_p, a.bounces, alb.ctypes.data_as(ctypes.c_void_p),
                                                            ctypes.c_void_p(d_rgb[m].data_ptr()), None, sp), "gpis_render_scene_s_paths_rgb")

    def timed(kind, m):
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        frame(kind, m)
        t1.record(stream)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / 1e3

    out = {"variant": variant, "fast_path": {m: int(media[m].derived()["fast_path"]) for m in MEANS}}
    for kind in ("lambert", "paths_rgb"):
        times = {m: [] for m in MEANS}
        counters = {}
        for m in MEANS:                              # warm-up: workspaces, code objects; and the work counters of one frame
            timed(kind, m)
            media[m].reset_counters()
            timed(kind, m)
            counters[m] = media[m].counters()
        for _ in range(a.reps):
            for m in MEANS:
                times[m].append(timed(kind, m))
        for m in MEANS:                              # one frame of each into zeroed buffers, for the comparison of the images
            (d_mono if kind == "lambert" else d_rgb)[m].zero_()
            timed(kind, m)
        img = {m: (d_mono if kind == "lambert" else d_rgb)[m].cpu().numpy() for m in MEANS}
        # the same surface: bit for bit where both run the exact lane-per-ray path (per-path media); the cooperative kernels of a
        # single-realization sphere sum the gradient in another order (their aniso agrees to 1e-5, not bit for bit)
        same = np.array_equal(img["sphere"].view(np.uint32), img["sphere-generic"].view(np.uint32))
        assert same or (out["fast_path"]["sphere"] and np.allclose(img["sphere"], img["sphere-generic"], rtol=1e-3, atol=1e-3 * a.spp)), \
            "%s: the forced-generic sphere renders another image" % kind
        assert img["knob"].any()
        best = {m: min(times[m]) for m in MEANS}
        out[kind] = {m: {"seconds_per_frame_best": best[m], "seconds_per_frame_all": times[m], "n_eval": counters[m][0], "n_seg": counters[m][1],
                         "samples_per_s": a.width * a.height * a.spp / best[m]} for m in MEANS}
        out[kind]["sphere_images_bit_equal"] = bool(same)
        out[kind]["generic_over_sphere"] = best["sphere-generic"] / best["sphere"]
        out[kind]["knob_over_generic"] = best["knob"] / best["sphere-generic"]
        out[kind]["knob_over_generic_per_eval"] = (best["knob"] / max(counters["knob"][0], 1)) / (best["sphere-generic"] / max(counters["sphere-generic"][0], 1))
    for m in MEANS:
        media[m].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--headline", default=None, help="the JSON line bench.py printed for this commit: stored, nothing is run")
    ap.add_argument("--headline-parent", default=None, help="the JSON line bench.py printed for the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.headline or a.headline_parent:
        doc = json.load(open(a.out))
        doc["bench_py_headline"] = {"this_commit": json.loads(a.headline) if a.headline else None,
                                    "parent_commit": json.loads(a.headline_parent) if a.headline_parent else None}
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        return
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    doc = {"workload": "scene S, %d x %d x %d spp = %d samples; gpis_render_scene_s and gpis_render_scene_s_paths_rgb (max_path_bounces %d, albedo %s); "
                       "C0-like media: world space, rho = 8, step_size 0.01" % (a.width, a.height, a.spp, a.width * a.height * a.spp, a.bounces, ALBEDO),
           "timing": "device events around the whole driver call, the three media alternating in one process after a warm-up frame of each",
           "media": {"sphere": "spherical mean, routed as ever", "sphere-generic": "min(spherical mean, plane procedural mean + 100): the same surface on the all-features instance",
                     "knob": "procedural mean, func = knob"},
           "results": [run_variant(pkg, a, v) for v in VARIANTS]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
