"""Time of baking a neural SDF mean into a tabulated slot (gpis_bake_mean_network: the exact fp64 evaluator of
csrc/gpis_nn_mean.hpp on a voxel lattice), and the frame time of the baked medium: one JSON document on stdout.

Bakes: 64^3 and 256^3 voxels over [-1.5, 1.5]^3 of two networks — the 32-wide "blob" of tests/golden/nn (network A) and a seeded
[3,64],[64,64]x3,[64,1] network.  Device events around the whole entry (weight upload, the launches, the grid's installation; no
voxel read-back), best and all of --reps.  Beside each:

    cpu            the C restatement of tests/native/nn_mean_ref.c on --threads threads in the same run.  256^3 is timed on a slab of
                   256 x 256 x --cpu-slab voxels and scaled by the voxel count (the voxels are independent); 64^3 is timed whole.
    issue roof     the vector-fp64 issue bound: every multiply-add of a layer is an unfused multiply and an add (the reference's
                   arithmetic), a wave64 fp64 instruction holds a SIMD's issue for 4 cycles (profiles/r02_valu_issue_cycles.json:
                   3.65-3.82; the fp32 figure of MI355X_MICROARCH.md's constants table, 2 cycles, doubled), 4 SIMDs x 256 CUs at
                   2.4 GHz: 39.3e12 lane-instructions/s.  Sines, bias adds, stores and the idle lanes of the last wave are not counted.

Frames: 256 x 256 x 8 of gpis_render_scene_s and a 4-bounce gpis_render_scene_s_paths_rgb on three media of tools/grid_mean_bench.py's
kind: `grid-64` (that tool's sphere grid), `baked-64` (network A baked on 64^3) and `handed-64` (the baked voxels read back and handed
to a second medium through gpis_set_mean_grid).  baked-64 and handed-64 run the same kernels on the same voxels: their times coincide
up to the run's spread and their images are equal bit for bit (asserted).  There is no bar on any of these times: they are a record.

    python tools/nn_bake_bench.py [--reps 5] [--threads 16] [--out profiles/r16_nn_bake_bench.json]
    python tools/nn_bake_bench.py --headline '<json line of bench.py>' ... --headline-parent '<json line>' ... --out ...   # adds the lines (no GPU)
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)

import grid_mean_bench as gmb         # noqa: E402
import sdf_mean_bench as smb          # noqa: E402

SIZES = (64, 256)
LANE_INSTRUCTIONS_PER_S = 256 * 4 * 64 / 4 * 2.4e9          # CUs x SIMDs x lanes / cycles per wave64 fp64 instruction x clock


def wide_network(pkg):
    layers = [(3, 64)] + [(64, 64)] * 3 + [(64, 1)]
    rng = np.random.default_rng(64)
    blob = np.concatenate([np.concatenate([(rng.standard_normal((o, i)) / np.sqrt(i)).T.reshape(-1), rng.standard_normal(o) * 0.3]) for i, o in layers])
    return pkg.Network(layers, [-gmb.HALF] * 3, [gmb.HALF] * 3, blob)


def lattice(n):
    s = (n - 1) / (2 * gmb.HALF)
    return np.array([[s, 0, 0, gmb.HALF * s], [0, s, 0, gmb.HALF * s], [0, 0, s, gmb.HALF * s], [0, 0, 0, 1]], dtype=np.float32)


def bake_times(pkg, a, name, net):
    import torch
    import nn_mean_ref as nmr
    ref = nmr.NnMeanRef(threads=a.threads)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    macs = sum(i * o for i, o in net.layers)
    out = {"network": name, "layers": [list(l) for l in net.layers], "multiply_adds_per_voxel": macs, "sines_per_voxel": sum(o for _, o in net.layers[1:-1])}
    m = pkg.Medium(gmb.medium_params(pkg, "single-realization", "grid-64"))
    for n in SIZES:
        T = lattice(n)
        m.bake_mean_network(0, net, (n, n, n), T)                    # warm-up: code objects, allocator
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            m.bake_mean_network(0, net, (n, n, n), T)
            t1.record(stream)
            torch.cuda.synchronize(dev)
            times.append(t0.elapsed_time(t1) / 1e3)
        nz = n if n <= 64 else a.cpu_slab
        i2w = pkg.index_to_world(T)
        ref.bake(net, (n, n, 1), i2w)                                # warm-up: the thread pool
        c0 = time.perf_counter()
        ref.bake(net, (n, n, nz), i2w)
        cpu = (time.perf_counter() - c0) * (n / nz)
        best = min(times)
        roof = n ** 3 * macs * 2 / LANE_INSTRUCTIONS_PER_S
        out["%d^3" % n] = {"voxels": n ** 3, "seconds_best": best, "seconds_all": times, "voxels_per_s": n ** 3 / best,
                           "cpu_seconds_%d_threads" % a.threads: cpu, "cpu_timed_on_slices": nz, "cpu_over_device": cpu / best,
                           "issue_roof_seconds": roof, "fraction_of_issue_roof": roof / best}
    m.close()
    return out


def frames(pkg, a, net, variant):
    import torch
    scene = np.array(pkg.default_scene_s(a.width, a.height, a.spp), dtype=pkg.SCENE_S).reshape(())
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    npix = a.width * a.height
    alb = np.array(smb.ALBEDO, dtype=np.float32)
    names = ("grid-64", "baked-64", "handed-64")
    media = {"grid-64": gmb.make_medium(pkg, variant, "grid-64")}
    media["baked-64"] = pkg.Medium(gmb.medium_params(pkg, variant, "grid-64"))
    vox = media["baked-64"].bake_mean_network(0, net, (64, 64, 64), lattice(64), return_voxels=True)
    media["handed-64"] = pkg.Medium(gmb.medium_params(pkg, variant, "grid-64"))
    media["handed-64"].set_mean_grid(0, vox, lattice(64), "linear")
    d_mono = {m: torch.zeros(npix, dtype=torch.float32, device=dev) for m in names}
    d_rgb = {m: torch.zeros(3 * npix, dtype=torch.float32, device=dev) for m in names}

    def timed(kind, m):
        h = media[m]
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        if kind == "lambert":
            h.L.check(h.L.lib.gpis_render_scene_s(h.h, scene_p, ctypes.c_void_p(d_mono[m].data_ptr()), None, sp), "gpis_render_scene_s")
        else:
            h.L.check(h.L.lib.gpis_render_scene_s_paths_rgb(h.h, scene_p, a.bounces, alb.ctypes.data_as(ctypes.c_void_p),
                                                            ctypes.c_void_p(d_rgb[m].data_ptr()), None, sp), "gpis_render_scene_s_paths_rgb")
        t1.record(stream)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / 1e3

    out = {"variant": variant}
    for kind in ("lambert", "paths_rgb"):
        times, counters = {m: [] for m in names}, {}
        for m in names:
            timed(kind, m)
            media[m].reset_counters()
            timed(kind, m)
            counters[m] = media[m].counters()
        for _ in range(a.reps):
            for m in names:
                times[m].append(timed(kind, m))
        buf = d_mono if kind == "lambert" else d_rgb
        for m in names:
            buf[m].zero_()
            timed(kind, m)
        img = {m: buf[m].cpu().numpy() for m in names}
        assert img["baked-64"].any() and np.array_equal(img["baked-64"].view(np.uint32), img["handed-64"].view(np.uint32)), kind
        assert counters["baked-64"] == counters["handed-64"], kind
        best = {m: min(times[m]) for m in names}
        out[kind] = {m: {"seconds_per_frame_best": best[m], "seconds_per_frame_all": times[m], "n_eval": counters[m][0], "n_seg": counters[m][1]} for m in names}
        out[kind]["baked_over_handed"] = best["baked-64"] / best["handed-64"]
        out[kind]["baked_equals_handed_bit_for_bit"] = True
    for m in names:
        media[m].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-slab", type=int, default=8, help="z-slices of the 256^3 lattice the CPU restatement is timed on")
    ap.add_argument("--headline", action="append", default=None, help="a JSON line bench.py printed for this commit: stored, nothing is run")
    ap.add_argument("--headline-parent", action="append", default=None, help="a JSON line bench.py printed for the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.headline or a.headline_parent:
        doc = json.load(open(a.out))
        doc["bench_py_headline"] = {"order": "alternating in one session, same device: parent, this commit, parent, this commit, ...",
                                    "this_commit": [json.loads(l) for l in a.headline or []],
                                    "parent_commit": [json.loads(l) for l in a.headline_parent or []]}
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        return
    import _gpis_pkg
    import nn_mean_ref as nmr
    pkg = _gpis_pkg.load_package()
    blob = pkg.load_network(nmr.network_path("A"))
    doc = {"workload": "gpis_bake_mean_network on n^3 voxels over [-1.5, 1.5]^3; frames: scene S, %d x %d x %d spp, gpis_render_scene_s and "
                       "gpis_render_scene_s_paths_rgb (max_path_bounces %d), C0-like media of tools/grid_mean_bench.py" % (a.width, a.height, a.spp, a.bounces),
           "timing": "device events around the whole entry, best of %d after a warm-up call; the media of a frame comparison alternate in one process" % a.reps,
           "issue_roof": "2 unfused fp64 instructions per multiply-add, 4 issue cycles per wave64 fp64 instruction, 1024 SIMDs at 2.4 GHz: %.4g lane-instructions/s" % LANE_INSTRUCTIONS_PER_S,
           "bakes": [bake_times(pkg, a, "A (blob, 32 wide)", blob), bake_times(pkg, a, "64 wide, 3 hidden layers", wide_network(pkg))],
           "frames": [frames(pkg, a, blob, v) for v in smb.VARIANTS]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
