"""Frame rate of the weight-space scene-S driver (gpis_ws_render_scene_s) against the staged composition of the batch entries:
one JSON document on stdout.

For a single-realization and a per-path (renewal) medium with N = 300 basis functions it renders one frame of scene S and reports
samples/s, segments/s, evaluations/s, n_spec / n_eval and the hit fraction of the fused entry (the whole call, timed with events
after a warm-up), and the baseline: gpis_ws_sample_distance_batch on the frame's valid primary rays plus
gpis_ws_transmittance_batch on its shadow rays, both prepared and uploaded beforehand (tests/ws_scene_ref.py), the sum of the two
launches only.  Baseline and fused entry run in the same process on the same frame, alternating, best of --reps each.

    python tools/ws_scene_bench.py [--width 256 --height 256 --spp 8] [--reps 3] [--out profiles/r05_ws_scene_bench.json]
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
import ws_scene_ref  # noqa: E402


def run(pkg, ref, form, scene, rays, us, n_miss, reps):
    import torch
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", single=1 if form == "single" else 0, n_basis=300)
    m = pkg.WeightSpaceMedium(p, w)
    L = m.L.lib
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to(dev)
    d_seg = torch.zeros(n * pkg.SEG_OUT.itemsize, dtype=torch.uint8, device=dev)
    # the shadow rays of this medium: the device's primary results (bit-identical to the restatement), shaded on the host
    m.L.check(L.gpis_ws_sample_distance_batch(m.h, n, vp(d_rays), vp(d_seg), sp), "gpis_ws_sample_distance_batch")
    seg = d_seg.cpu().numpy().view(pkg.SEG_OUT)
    shadow, _, hit, lit = ref.shade(scene, rays, seg, us)
    shadow = np.ascontiguousarray(shadow[lit != 0])
    ns = len(shadow)
    d_sh = torch.from_numpy(shadow.view(np.uint8).reshape(-1).copy()).to(dev)
    d_vis = torch.zeros(max(ns, 1), dtype=torch.uint8, device=dev)
    npix = int(scene["width"]) * int(scene["height"])
    d_rad = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_hit = torch.zeros(npix, dtype=torch.int32, device=dev)
    scene_p = np.array(scene, dtype=pkg.SCENE_S).reshape(()).ctypes.data_as(ctypes.c_void_p)

    def staged():
        m.L.check(L.gpis_ws_sample_distance_batch(m.h, n, vp(d_rays), vp(d_seg), sp), "gpis_ws_sample_distance_batch")
        m.L.check(L.gpis_ws_transmittance_batch(m.h, ns, vp(d_sh), vp(d_vis), sp), "gpis_ws_transmittance_batch")

    def fused():
        m.L.check(L.gpis_ws_render_scene_s(m.h, scene_p, vp(d_rad), vp(d_hit), sp), "gpis_ws_render_scene_s")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / 1e3

    staged()                                         # warm-up: workspaces, code objects
    fused()
    torch.cuda.synchronize(dev)
    t_staged, t_fused = [], []
    counters = None
    for _ in range(reps):
        t_staged.append(timed(staged))
        m.reset_counters()
        t_fused.append(timed(fused))
        counters = m.counters()
    m.close()
    bs, bf = min(t_staged), min(t_fused)
    n_samples = n + n_miss
    return {
        "form": form, "basis_functions": 300, "samples": n_samples, "valid_primary_rays": n, "shadow_rays": ns, "reps": reps,
        "fused_seconds_best": bf, "fused_seconds_all": t_fused, "staged_seconds_best": bs, "staged_seconds_all": t_staged,
        "fused_over_staged": bf / bs, "fused_not_slower": bool(bf <= bs),
        "samples_per_s": n_samples / bf, "segments_per_s": counters["n_seg"] / bf, "evals_per_s": counters["n_eval"] / bf,
        "n_seg": counters["n_seg"], "n_eval": counters["n_eval"], "n_spec_over_n_eval": counters["n_spec"] / max(counters["n_eval"], 1),
        "hit_fraction": float(hit.sum()) / n_samples,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forms", default="single,per_path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = _gpis_pkg.load_package()
    ref = ws_scene_ref.SceneRef(pkg, ob)
    scene = ob.default_scene_s(a.width, a.height, a.spp)
    rays, us, _, n_miss = ref.primary_rays(scene)
    doc = {"workload": "scene S (camera z = 4, fov 35, bounding radius 1.5, light (0.5, 0.7, 0.5)), %d x %d x %d spp = %d samples, through "
                       "the weight-space GP medium, N = 300, spherical mean r = 1 (C0-like: sigma 0.1, l 0.05), step 0.01"
                       % (a.width, a.height, a.spp, a.width * a.height * a.spp),
           "fused": "gpis_ws_render_scene_s, the whole call: k_ws_scene (one wave per sample, dynamic work fetch, realization reuse "
                    "under single / GLOBAL) + k_ws_scene_sum + the range-flag read",
           "staged_baseline": "gpis_ws_sample_distance_batch on the valid primary rays + gpis_ws_transmittance_batch on the shadow rays, "
                              "rays uploaded beforehand; the two calls only (no ray generation, shading or pixel sum)",
           "results": [run(pkg, ref, f, scene, rays, us, n_miss, max(a.reps, 3)) for f in a.forms.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
