"""Frame rate of the weight-space path driver (gpis_ws_render_scene_s_paths): one JSON document on stdout.

For a single-realization medium and per-path media under the contexts GLOBAL and RENEWAL, N = 300 basis functions, it renders one
frame of scene S at --bounces path bounces and reports seconds per frame, samples/s, segments/s, evaluations/s and n_spec / n_eval
(the whole call, timed with events after a warm-up, best of --reps).  The yardstick is the single-scatter frame driver on the same
frame: run tools/ws_scene_bench.py on the same device in the same session and set the segments/s side by side.

    python tools/ws_paths_bench.py [--width 256 --height 256 --spp 8 --bounces 4] [--reps 3] [--out profiles/r06_ws_paths_bench.json]
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
import ws_oracle  # noqa: E402

FORMS = {"single": dict(ctx="renewal", single=1), "per_path_global": dict(ctx="global", single=0),
         "per_path_renewal": dict(ctx="renewal", single=0)}


def run(pkg, form, scene, bounces, albedo, reps):
    import torch
    p, w = ws_oracle.ws_params(pkg, n_basis=300, **FORMS[form])
    m = pkg.WeightSpaceMedium(p, w)
    L = m.L.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
    npix = int(scene["width"]) * int(scene["height"])
    n_samples = npix * int(scene["spp_count"])
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)

    def frame():
        m.L.check(L.gpis_ws_render_scene_s_paths(m.h, scene.ctypes.data_as(ctypes.c_void_p), int(bounces), ctypes.c_float(albedo),
                                                 ctypes.c_void_p(d_rad.data_ptr()), sp), "gpis_ws_render_scene_s_paths")

    frame()                                          # warm-up: workspace, code object
    torch.cuda.synchronize(dev)
    times, counters = [], None
    for _ in range(reps):
        m.reset_counters()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        frame()
        b.record(stream)
        torch.cuda.synchronize(dev)
        times.append(a.elapsed_time(b) / 1e3)
        counters = m.counters()
    m.close()
    best = min(times)
    return {"form": form, "basis_functions": 300, "max_bounces": bounces, "albedo": albedo, "samples": n_samples, "reps": reps,
            "seconds_best": best, "seconds_all": times, "samples_per_s": n_samples / best, "segments_per_s": counters["n_seg"] / best,
            "evals_per_s": counters["n_eval"] / best, "n_seg": counters["n_seg"], "n_eval": counters["n_eval"],
            "segments_per_sample": counters["n_seg"] / n_samples, "evals_per_segment": counters["n_eval"] / max(counters["n_seg"], 1),
            "n_spec_over_n_eval": counters["n_spec"] / max(counters["n_eval"], 1), "image_mean": float(d_rad.mean().item()) / (reps + 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--albedo", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forms", default="single,per_path_global,per_path_renewal")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = _gpis_pkg.load_package()
    scene = ob.default_scene_s(a.width, a.height, a.spp)
    doc = {"workload": "scene S (camera z = 4, fov 35, bounding radius 1.5, light (0.5, 0.7, 0.5)), %d x %d x %d spp = %d samples, %d path "
                       "bounces, albedo %g, through the weight-space GP medium, N = 300, spherical mean r = 1 (C0-like: sigma 0.1, l 0.05), "
                       "step 0.01" % (a.width, a.height, a.spp, a.width * a.height * a.spp, a.bounces, a.albedo),
           "entry": "gpis_ws_render_scene_s_paths, the whole call: k_ws_paths (one wave per sample, the whole path in the wave, dynamic work "
                    "fetch, one realization per segment word) + k_ws_paths_sum + the range-flag read",
           "results": [run(pkg, f, scene, a.bounces, a.albedo, max(a.reps, 1)) for f in a.forms.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
