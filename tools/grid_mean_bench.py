"""Frame time of a medium with a tabulated mean (GPIS_MEAN_TABULATED: a dense SDF voxel grid) against the same surface as an
analytic mean on the same kernels: one JSON document on stdout.

Two frames per medium: 256 x 256 x 8 of gpis_render_scene_s (Lambert, one segment plus a shadow ray per sample) and a 4-bounce
frame of gpis_render_scene_s_paths_rgb.  Media are C0-like (world space, rho = 8), in two variants: single realization and per-path
Renewal.  Four means each, all on the all-features path instance:

    sphere-generic  the spherical mean of C0 forced through the all-features instance (tools/sdf_mean_bench.py): what to compare with
    knob            the procedural knob of that tool
    grid-64         the SAME sphere as a 64^3 linear-interpolated SDF grid over [-1.5, 1.5]^3 (1 MiB of voxels: resident in L2)
    grid-256        the same sphere as a 256^3 grid (64 MiB of voxels)

The step from sphere-generic to a grid is the cost of the lookup: one evaluation of the mean is 8 per-lane gathers, one gradient 32.
There is no bar on these times: they are a record.  Timing: device events around the whole driver call, media alternating in one
process after a warm-up frame of each, best and all of --reps.

    python tools/grid_mean_bench.py [--width 256 --height 256 --spp 8 --bounces 4] [--reps 5] [--out profiles/r15_grid_mean_bench.json]
    python tools/grid_mean_bench.py --headline '<json line of bench.py>' --headline-parent '<json line>' --out ...   # adds the two lines (no GPU)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sdf_mean_bench as smb          # noqa: E402

ALBEDO = smb.ALBEDO
GRIDS = {"grid-64": 64, "grid-256": 256}
MEANS = ("sphere-generic", "knob") + tuple(GRIDS)
VARIANTS = smb.VARIANTS
HALF = 1.5                             # the grid covers [-HALF, HALF]^3


def medium_params(pkg, variant, mean):
    if mean not in GRIDS:
        return smb.medium_params(pkg, variant, mean)
    p = smb.medium_params(pkg, variant, "sphere")
    p["mean"]["type"] = pkg.MEAN_TYPE.TABULATED
    p["mean"]["offset"], p["mean"]["scale"], p["mean"]["func"] = 0.0, 1.0, 0
    return p


def sphere_grid(center, radius, n):
    """(voxels[k, j, i], world -> index) of |p - center| - radius on n^3 voxels over [-HALF, HALF]^3"""
    c = (np.arange(n, dtype=np.float32) / np.float32(n - 1) * 2 - 1) * np.float32(HALF)
    z, y, x = np.meshgrid(c - np.float32(center[2]), c - np.float32(center[1]), c - np.float32(center[0]), indexing="ij", sparse=True)
    vox = (np.sqrt(x * x + y * y + z * z) - np.float32(radius)).astype(np.float32)
    s = (n - 1) / (2 * HALF)
    T = np.array([[s, 0, 0, HALF * s], [0, s, 0, HALF * s], [0, 0, s, HALF * s], [0, 0, 0, 1]], dtype=np.float32)
    return vox, T


def make_medium(pkg, variant, mean):
    m = pkg.Medium(medium_params(pkg, variant, mean))
    if mean in GRIDS:
        sph = smb.medium_params(pkg, variant, "sphere")["mean"]
        vox, T = sphere_grid(sph["center"], float(sph["radius"]), GRIDS[mean])
        m.set_mean_grid(0, vox, T, "linear")
    return m


def run_variant(pkg, a, variant):
    import torch
    scene = np.array(pkg.default_scene_s(a.width, a.height, a.spp), dtype=pkg.SCENE_S).reshape(())
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    npix = a.width * a.height
    alb = np.array(ALBEDO, dtype=np.float32)
    media = {m: make_medium(pkg, variant, m) for m in MEANS}
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
        # the grids sample the sphere's SDF: the same surface up to the trilinear interpolation error, so the images agree in the mean
        ref = float(img["sphere-generic"].mean())
        rel = {m: abs(float(img[m].mean()) - ref) / ref for m in GRIDS}
        assert all(img[m].any() for m in MEANS), kind
        best = {m: min(times[m]) for m in MEANS}
        out[kind] = {m: {"seconds_per_frame_best": best[m], "seconds_per_frame_all": times[m], "n_eval": counters[m][0], "n_seg": counters[m][1],
                         "samples_per_s": a.width * a.height * a.spp / best[m]} for m in MEANS}
        out[kind]["grid_image_mean_relative_difference"] = rel
        for m in GRIDS:
            out[kind][m + "_over_generic"] = best[m] / best["sphere-generic"]
            out[kind][m + "_over_generic_per_eval"] = (best[m] / max(counters[m][0], 1)) / (best["sphere-generic"] / max(counters["sphere-generic"][0], 1))
        out[kind]["knob_over_generic"] = best["knob"] / best["sphere-generic"]
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
           "timing": "device events around the whole driver call, the four media alternating in one process after a warm-up frame of each",
           "media": {"sphere-generic": "min(spherical mean, plane procedural mean + 100): the sphere on the all-features instance",
                     "knob": "procedural mean, func = knob",
                     "grid-64": "tabulated mean: the sphere's SDF on 64^3 voxels over [-1.5, 1.5]^3, linear interpolation (1 MiB)",
                     "grid-256": "tabulated mean: the sphere's SDF on 256^3 voxels over [-1.5, 1.5]^3, linear interpolation (64 MiB)"},
           "results": [run_variant(pkg, a, v) for v in VARIANTS]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
