"""Rates of the weight-space GP medium (gpis_ws_*): one JSON document on stdout.

For a single-realization and a per-path (renewal) medium with N = 300 basis functions, on a fixed set of rays through a spherical
mean like C0's (tests/ws_oracle.py: make_rays), it measures the device's sampleDistance batch (device-pointer entry, timed with
CUDA events after a warm-up) and reports segments/s, field evaluations/s (the evaluations the reference performs: the march's
values, one per gradient, six per finite-difference gradient) and evaluations per segment, plus the 16-thread C restatement's rate
on a subset of the same rays.

    python tools/ws_bench.py [--rays 1048576] [--cpu-rays 2048] [--reps 3] [--out profiles/r04_ws_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _gpis_pkg  # noqa: E402
import ws_oracle  # noqa: E402

FP64_LANE_OPS_PER_TERM = 60          # estimate: one cos_glibc (reduction, table, polynomial) + the dot and the accumulation
FP64_ROOF_LANE_OPS = 256 * 4 * 16 * 2.4e9   # CUs x SIMDs x fp64 lanes per cycle x clock (MI355X_MICROARCH.md): ~39 T lane-ops/s


def run(pkg, form, rays, reps, cpu_rays, wso):
    import torch
    single = 1 if form == "single" else 0
    p, w = ws_oracle.ws_params(pkg, ctx="renewal", single=single, n_basis=300)
    m = pkg.WeightSpaceMedium(p, w)
    L = m.L.lib
    n = len(rays)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n * pkg.SEG_OUT.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def once():
        m.L.check(L.gpis_ws_sample_distance_batch(m.h, n, ctypes.c_void_p(d_rays.data_ptr()), ctypes.c_void_p(d_out.data_ptr()),
                                                  ctypes.c_void_p(stream.cuda_stream)), "gpis_ws_sample_distance_batch")

    once()                                           # warm-up (workspace allocation, code object load)
    torch.cuda.synchronize(dev)
    m.reset_counters()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        once()
        b.record(stream)
        torch.cuda.synchronize(dev)
        times.append(a.elapsed_time(b) / 1e3)
    c = m.counters()
    out = d_out.cpu().numpy().view(pkg.SEG_OUT)
    best = min(times)
    evals = c["n_eval"] / reps
    res = {
        "form": form, "basis_functions": 300, "rays": n, "reps": reps, "seconds_best": best, "seconds_all": times,
        "segments_per_s": n / best, "evals_per_s": evals / best, "evals_per_segment": evals / n,
        "speculative_evals_per_segment": c["n_spec"] / reps / n, "hit_fraction": float((out["exited"] == 0).mean()),
    }
    res["fp64_roof_fraction_estimate"] = res["evals_per_s"] * 300 * FP64_LANE_OPS_PER_TERM / FP64_ROOF_LANE_OPS
    if cpu_rays and wso is not None:
        sub = rays[:cpu_rays]
        t0 = time.perf_counter()
        want, n_eval = wso.sample_distance(p, w, sub, threads=16)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(want.view(np.uint8), out[:cpu_rays].view(np.uint8)))
        res["cpu_restatement"] = {"threads": 16, "rays": int(cpu_rays), "seconds": dt, "segments_per_s": cpu_rays / dt,
                                  "evals_per_s": n_eval / dt, "bit_identical_to_gpu": same}
        res["gpu_over_cpu_evals"] = res["evals_per_s"] / res["cpu_restatement"]["evals_per_s"]
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--cpu-rays", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forms", default="single,per_path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = _gpis_pkg.load_package()
    wso = ws_oracle.WsOracle() if a.cpu_rays and ws_oracle.available() else None
    rays = ws_oracle.make_rays(pkg, a.rays, seed=2024)
    doc = {"workload": "weight-space GP medium, N = 300, spherical mean r = 1 (C0-like: sigma 0.1, l 0.05), %d camera-like rays "
                       "from z = 4, near 0, far 6, step 0.01" % a.rays,
           "kernel": "k_ws_march<true> (one wave per segment, %d speculative points per batch, 18 KB LDS)" % 32,
           "fp64_roof_lane_ops_per_s": FP64_ROOF_LANE_OPS, "fp64_lane_ops_per_term_estimate": FP64_LANE_OPS_PER_TERM,
           "results": [run(pkg, f, rays, a.reps, a.cpu_rays, wso) for f in a.forms.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
