"""GPU-box measurement of the multi-bounce conductor NEE / MIS path driver (gpis_render_scene_s_nee_paths): one JSON document on
stdout (and in --out).
usage: python tools/nee_paths_bench.py [--config C2] [--width 256 --height 256 --spp 8] [--bounces 2,4,8] [--reps 5] [--out FILE]

Per max_path_bounces: seconds per frame (the fastest of --reps calls after one warm-up call, host clock around a call that ends in
a device synchronise), segments and paths per second (segments from the handle's counters).  In the same run, alternating with
it call by call, gpis_render_scene_s_nee on the same frame: with max_path_bounces = 2 both march the same segments, so the ratio
of the two frame times is what the bounce bookkeeping costs.  The two images are compared."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import _gpis_pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C2")
ap.add_argument("--width", type=int, default=256)
ap.add_argument("--height", type=int, default=256)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--bounces", default="2,4,8")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
import torch  # noqa: E402
pkg = _gpis_pkg.load_package()
med = pkg.Medium(pkg.params_for_config(a.config))
scene = np.array(pkg.default_scene_s(a.width, a.height, a.spp), dtype=pkg.SCENE_S)
surf = np.array(pkg.default_surface_s(), dtype=pkg.SURFACE_S)
rad = torch.zeros(a.width * a.height, dtype=torch.float32, device="cuda")
n = a.width * a.height * a.spp
vp = ctypes.c_void_p


def frame(max_bounces):
    """(seconds, segments, image) of one call; max_bounces 0: gpis_render_scene_s_nee"""
    rad.zero_()
    med.reset_counters()
    torch.cuda.synchronize()
    t = time.perf_counter()
    if max_bounces:
        med.call("gpis_render_scene_s_nee_paths", scene.ctypes.data_as(vp), surf.ctypes.data_as(vp), max_bounces, rad.data_ptr(), None, None)
    else:
        med.call("gpis_render_scene_s_nee", scene.ctypes.data_as(vp), surf.ctypes.data_as(vp), rad.data_ptr(), None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return dt, med.counters()[1], rad.cpu().numpy()


bounces = [int(b) for b in a.bounces.split(",")]
kinds = [0] + bounces
best, segs, images = {}, {}, {}
for k in kinds:
    frame(k)                           # warm-up: code objects, workspace
for _ in range(a.reps):
    for k in kinds:                    # alternating, so that a busy host touches every kind alike
        dt, segs[k], images[k] = frame(k)
        best[k] = min(best.get(k, dt), dt)
doc = {"workload": "scene-S conductor NEE/MIS paths %s %dx%dx%d" % (a.config, a.width, a.height, a.spp), "samples": n, "reps": a.reps,
       "timing": "host clock around one call and a device synchronise, fastest of reps, one warm-up call before",
       "single_interaction": {"entry": "gpis_render_scene_s_nee", "seconds_per_frame": best[0], "segments": segs[0],
                              "Msegments_per_s": segs[0] / best[0] / 1e6, "Mpaths_per_s": n / best[0] / 1e6},
       "paths": []}
for k in bounces:
    doc["paths"].append({"max_path_bounces": k, "seconds_per_frame": best[k], "segments": segs[k], "segments_per_path": segs[k] / n,
                         "Msegments_per_s": segs[k] / best[k] / 1e6, "Mpaths_per_s": n / best[k] / 1e6, "image_sum": float(images[k].sum())})
if 2 in best:
    doc["two_bounces_over_single_interaction"] = {"time_ratio": best[2] / best[0], "same_segments": bool(segs[2] == segs[0]),
                                                  "same_image": bool(np.array_equal(images[2].view(np.uint32), images[0].view(np.uint32)))}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
