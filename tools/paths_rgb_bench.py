"""Frame time of the RGB path driver (gpis_render_scene_s_paths_rgb) against the mono driver (gpis_render_scene_s_paths): one JSON
document on stdout.

Both drivers march the same rays (the tool asserts equal n_eval and n_seg), so the difference is the shade / NEE-add / accumulate
kernels and 24 B per sample per bounce of extra path state.  The two are timed in ONE process in alternating runs (device events
around the whole call, after a warm-up, best and all of --reps): a C1 frame with a guide, emission off, and the `rust` medium of
tests/paths_rgb_ref.py (emission on: the fp64 fbm at every hit; the mono driver renders the same medium without it).

    python tools/paths_rgb_bench.py [--width 256 --height 256 --spp 8 --bounces 4] [--reps 5] [--mono-lib <libgpis_hip.so of the
                                    parent commit>] [--out profiles/r09_paths_rgb_bench.json]
    python tools/paths_rgb_bench.py --only rgb|mono [--case c1|rust]      # the frames alone, for rocprofv3 --kernel-trace --stats
    python tools/paths_rgb_bench.py --merge <out.json> c1|rust <mono_kernel_stats.csv> <rgb_kernel_stats.csv>   # adds a kernel table (no GPU)
"""
import argparse
import csv
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ALBEDO = (0.8, 0.6, 0.4)


def case_params(pkg, case):
    import paths_rgb_ref as prr
    if case == "rust":
        return prr.CASES["rust"](pkg)[0], False
    return pkg.params_for_config("C1"), True


class OtherBuild:
    """The few entries the mono frame needs, from another build of the library (one that may lack the RGB entry, which
    pkg.GpisLib would refuse to load)."""

    class _Lib:
        def __init__(self, path):
            vp, i32 = ctypes.c_void_p, ctypes.c_int
            self.lib = ctypes.CDLL(path)
            self.lib.gpis_last_error.restype = ctypes.c_char_p
            self.lib.gpis_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
            self.lib.gpis_destroy.argtypes = [vp]
            self.lib.gpis_build_guide.argtypes = [vp, i32, i32]
            self.lib.gpis_get_counters.argtypes = [vp, vp, vp]
            self.lib.gpis_reset_counters.argtypes = [vp]
            self.lib.gpis_render_scene_s_paths.argtypes = [vp, vp, i32, ctypes.c_float, vp, vp]

        def check(self, status, what):
            if status != 0:
                raise RuntimeError("%s failed (%d): %s" % (what, status, self.lib.gpis_last_error().decode()))

    def __init__(self, pkg, path, params):
        self.L = self._Lib(path)
        self.params = pkg.as_params(params)
        self.h = ctypes.c_void_p()
        self.L.check(self.L.lib.gpis_create(self.params.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(self.h)), "gpis_create")

    def build_guide(self, half, ppc):
        self.L.check(self.L.lib.gpis_build_guide(self.h, half, ppc), "gpis_build_guide")

    def reset_counters(self):
        self.L.check(self.L.lib.gpis_reset_counters(self.h), "gpis_reset_counters")

    def counters(self):
        e, s = ctypes.c_uint64(), ctypes.c_uint64()
        self.L.check(self.L.lib.gpis_get_counters(self.h, ctypes.byref(e), ctypes.byref(s)), "gpis_get_counters")
        return e.value, s.value

    def close(self):
        self.L.lib.gpis_destroy(self.h)


def run_case(pkg, a, case, mono_lib):
    import torch
    import oracle_bindings as ob
    params, guide = case_params(pkg, case)
    scene = np.array(ob.default_scene_s(a.width, a.height, a.spp), dtype=pkg.SCENE_S).reshape(())
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    npix = a.width * a.height
    alb = np.array(ALBEDO, dtype=np.float32)
    media = {}
    for which in ("mono", "rgb"):
        if a.only and which != a.only:
            continue
        m = OtherBuild(pkg, mono_lib, params) if which == "mono" and mono_lib else pkg.Medium(params)
        if guide:
            m.build_guide(16, 8)
        media[which] = m
    d_mono = torch.zeros(npix, dtype=torch.float32, device=dev)
    d_rgb = torch.zeros(3 * npix, dtype=torch.float32, device=dev)
    scene_p = scene.ctypes.data_as(ctypes.c_void_p)

    def frame(which):
        m = media[which]
        if which == "mono":
            m.L.check(m.L.lib.gpis_render_scene_s_paths(m.h, scene_p, a.bounces, ctypes.c_float(ALBEDO[0]), ctypes.c_void_p(d_mono.data_ptr()), sp),
                      "gpis_render_scene_s_paths")
        else:
            m.L.check(m.L.lib.gpis_render_scene_s_paths_rgb(m.h, scene_p, a.bounces, alb.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_rgb.data_ptr()),
                                                            None, sp), "gpis_render_scene_s_paths_rgb")

    def timed(which):
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        frame(which)
        t1.record(stream)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) / 1e3

    times = {w: [] for w in media}
    counters = {}
    for w in media:                                  # warm-up: workspaces, code objects; and the work counters of one frame
        timed(w)
        media[w].reset_counters()
        timed(w)
        counters[w] = media[w].counters()
    for _ in range(a.reps):
        for w in media:
            times[w].append(timed(w))
    d_mono.zero_()                                   # one frame of each into zeroed buffers, for the comparison of the images
    d_rgb.zero_()
    for w in media:
        timed(w)
    out = {"case": case, "emission": bool(int(params["mean_emission"]["enabled"])), "guide": guide, "reps": a.reps}
    for w in media:
        out[w] = {"seconds_per_frame_best": min(times[w]), "seconds_per_frame_all": times[w], "n_eval": counters[w][0], "n_seg": counters[w][1]}
        media[w].close()
    if len(media) == 2:
        emissive = out["emission"]
        if not emissive:
            # the same rays: channel 0 is the mono image bit for bit, and the work counters agree
            assert counters["mono"] == counters["rgb"], counters
            mono = d_mono.cpu().numpy()
            rgb0 = d_rgb.cpu().numpy().reshape(-1, 3)[:, 0]
            assert np.array_equal(mono.view(np.uint32), np.ascontiguousarray(rgb0).view(np.uint32)), "channel 0 differs from the mono driver's image"
        else:
            assert counters["rgb"][1] > counters["mono"][1]      # the extra last segment of an emissive medium
        out["rgb_over_mono"] = out["rgb"]["seconds_per_frame_best"] / out["mono"]["seconds_per_frame_best"]
        out["paths_per_s_rgb"] = a.width * a.height * a.spp / out["rgb"]["seconds_per_frame_best"]
    return out


def merge(path, case, mono_csv, rgb_csv):
    """the per-kernel tables tools/rocpd_summary.py writes for `--only mono` and `--only rgb` of one case, into the document"""
    doc = json.load(open(path))
    table = {}
    for which, f in (("mono", mono_csv), ("rgb", rgb_csv)):
        rows = list(csv.DictReader(open(f)))
        table[which] = [{"kernel": r["Name"], "calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"]), "percent": float(r["Percentage"])} for r in rows]
    doc.setdefault("kernel_table", {})[case] = table
    doc["kernel_table_source"] = "rocprofv3 --kernel-trace --stats of `--only mono` and `--only rgb` (warm-up frames included), each a run of its own"
    with open(path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        return merge(*sys.argv[2:6])
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("mono", "rgb"), default=None)
    ap.add_argument("--case", choices=("c1", "rust"), default=None)
    ap.add_argument("--mono-lib", default=None, help="time the mono driver of another build of the library (the parent commit's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _gpis_pkg
    pkg = _gpis_pkg.load_package()
    doc = {"workload": "scene S, %d x %d x %d spp = %d samples, max_path_bounces %d, albedo %s (mono: %g)"
                       % (a.width, a.height, a.spp, a.width * a.height * a.spp, a.bounces, ALBEDO, ALBEDO[0]),
           "timing": "device events around the whole driver call, alternating mono / rgb in one process after a warm-up frame of each",
           "mono_library": a.mono_lib or "the same build",
           "results": [run_case(pkg, a, c, a.mono_lib) for c in ([a.case] if a.case else ["c1", "rust"])]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
