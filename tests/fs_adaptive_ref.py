"""TEST INFRASTRUCTURE: the cases and the CPU composite of the function-space adaptive drivers (gpis_fs_render_scene_s_adaptive,
gpis_fs_render_scene_s_paths_adaptive).  A sample is a pure function of (x, y, k, scene_seed), so a frame is the schedule of
tests/adaptive_ref.py over per-sample values that one uniform-driver call with spp_count = 1 gives: here the CPU composites
fs_scene_ref.FsSceneRef.compose and fs_paths_ref.FsPathsRef.compose, in tests/test_gpu_fs_adaptive.py the uniform GPU entries.
Neither uses the code under test.

The frame is adaptive_ref's small one (22 x 14, camera at (0, 0, 8): 6 x 4 records, clipped tiles on two edges); the media are
fs_scene_ref.fs_params with few sample points, so a case is some ten thousand segments.  What the schedule's `hits` slot carries
is the driver's per-pixel count: the primary segment's hit for the frame driver, the segments marched (path plus shadow, at most
2 * bounces - 1 per sample) for the path driver."""
import os

import numpy as np

import adaptive_ref as ar
import fs_paths_ref
import fs_scene_ref
import ws_adaptive_ref as wa
import ws_oracle

W, H = ar.SMALL_W, ar.SMALL_H
W64, H64, S64 = 12, 8, 32                 # the frame of the 64-point case: 3 x 2 records, two passes
GOLDEN = os.path.join(ws_oracle.ROOT, "tests", "golden", "fs_adaptive_small.npz")
BOUNCES, ALBEDO = 3, 0.8

# name -> (driver, (context, fs_sample_points, fs_step_size), scene fields, (width, height))
CASES = {
    "lambert_renewal": ("lambert", ("RENEWAL", 16, 0.04), {}, (W, H)),
    "lambert_none": ("lambert", ("NONE", 12, 0.0), {}, (W, H)),
    "lambert_global_short": ("lambert", ("GLOBAL", 14, 0.05), {"spp_count": 40}, (W, H)),
    "lambert_renewal_plus": ("lambert", ("RENEWAL_PLUS", 16, 0.04), {}, (W, H)),
    "paths_renewal": ("paths", ("RENEWAL", 12, 0.04), {}, (W, H)),
    "paths_none": ("paths", ("NONE", 12, 0.0), {}, (W, H)),
    "paths_global_short": ("paths", ("GLOBAL", 8, 0.05), {"spp_count": 40}, (W, H)),
    "paths_renewal_plus": ("paths", ("RENEWAL_PLUS", 16, 0.04), {}, (W, H)),
}
# The largest state, n_points at the LDS bound: two passes.  The plan step dilates the weights over the neighbouring records, so of
# 3 x 2 records one gets a count of 1 only when the object stays out of two columns: the camera stands to the side and looks past
# it under a wider angle (tried on the CPU composite: centred, every record of the second pass got 8 .. 19 samples).
SIDE_VIEW = {"spp_count": S64, "cam_pos": (3.0, 0.0, 8.0), "cam_fov_deg": 65.0}
CASES_64 = {
    "lambert_global64": ("lambert", ("GLOBAL", 64, 0.01), SIDE_VIEW, (W64, H64)),
    "paths_global64": ("paths", ("GLOBAL", 64, 0.01), SIDE_VIEW, (W64, H64)),
}
# a light bright enough for renderTile's clamp (values above 65536 count as 0), as ws_adaptive_ref.CLAMP_CASES
CLAMP_CASES = {
    "lambert_clamp": ("lambert", ("RENEWAL", 16, 0.04), {"light_radiance": 1e5}, (W, H)),
    "paths_clamp": ("paths", ("RENEWAL", 12, 0.04), {"light_radiance": 1e6}, (W, H)),
}
# the early stop of the frame driver: a light behind the object, which no normal the camera sees faces (hits, but no lit sample)
DARK = {"light_dir": (0.0, 0.0, -1.0)}
ALL_CASES = dict(CASES, **CASES_64, **CLAMP_CASES)


def medium(pkg, ctx="RENEWAL", n=16, step=0.04):
    return fs_scene_ref.fs_params(pkg, ctx, n, step)


def scene(ob, spp=ar.SMALL_SPP, size=(W, H), **fields):
    s = ob.default_scene_s(size[0], size[1], spp)
    s["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        s[k] = v
    return s


def case_inputs(pkg, ob, name):
    """(driver, params, scene) of a case"""
    driver, (ctx, n, step), fields, size = ALL_CASES[name]
    return driver, medium(pkg, ctx, n, step), scene(ob, size=size, **fields)


frame = wa.frame                 # adaptive_ref.frame over render_one(scene with spp_count = 1) -> (image, count); adds largest_value
check_schedule = wa.check_schedule


def check_schedule_two_passes(ref):
    """the analogue of check_schedule for a frame of two passes: the first uniform at 16, the second mixing 1 with more than 16"""
    counts = ref["counts"]
    assert len(counts) == 2 and (counts[0] == 16).all() and (counts[1] == 1).any() and counts[1].max() > 16, [(int(c.min()), int(c.max())) for c in counts]


def check_case_schedule(name, ref):
    (check_schedule_two_passes if name in CASES_64 else check_schedule)(ref)


class CpuRenderer:
    """the two uniform drivers on the CPU, one call at a time; `seen` accumulates what fs_scene_ref.assert_non_vacuous asks of a
    frame (the frame driver's Composite) over the calls of one frame"""

    def __init__(self, pkg, ob, threads=ar.THREADS):
        self.pkg, self.ob = pkg, ob
        self.paths_ref = fs_paths_ref.FsPathsRef(pkg, ob, threads=threads)
        self.scene_ref = self.paths_ref.scene_ref

    def render_one(self, driver, p, bounces=BOUNCES, tally=None):
        if driver == "lambert":
            def one(s):
                c = self.scene_ref.compose(p, s)
                if tally is not None:
                    for k in ("n_miss", "n_exit", "n_hit", "n_visible", "n_occluded"):
                        tally[k] = tally.get(k, 0) + getattr(c, k)
                return c.image, c.hits
        else:
            def one(s):
                c = self.paths_ref.compose(p, s, bounces, ALBEDO)
                assert c.segs.max() <= 255
                if tally is not None:
                    tally["n_miss"] = tally.get("n_miss", 0) + c.n_miss
                    tally["n_exit"] = tally.get("n_exit", 0) + c.n_exit_after_hit
                    tally["n_hit"] = tally.get("n_hit", 0) + c.n_two_hits
                    tally["n_visible"] = tally.get("n_visible", 0) + c.n_visible
                    tally["n_occluded"] = tally.get("n_occluded", 0) + c.n_occluded
                return c.image, c.segs
        return one

    def frame(self, driver, p, sc, adaptive=None, bounces=BOUNCES):
        """the composite frame; ref["classes"] holds the frame's class counts for assert_non_vacuous"""
        tally = {}
        ref = frame(self.render_one(driver, p, bounces, tally), sc, adaptive)
        ref["classes"] = Classes(tally)
        return ref


class Classes:
    """what fs_scene_ref.assert_non_vacuous reads: a miss, an exit, a hit, a visible and an occluded shadow segment (for the path
    driver: an exit after a hit, and a path with two hits)"""

    def __init__(self, tally):
        for k in ("n_miss", "n_exit", "n_hit", "n_visible", "n_occluded"):
            setattr(self, k, tally.get(k, 0))


def golden_arrays(pkg, ob, cpu=None):
    """the contents of tests/golden/fs_adaptive_small.npz, from the CPU composites alone"""
    cpu = cpu or CpuRenderer(pkg, ob)
    out = {"adaptive": ar.default_adaptive(), "max_bounces": np.int32(BOUNCES), "albedo": np.float32(ALBEDO)}
    for tag, name in (("lambert", "lambert_renewal"), ("paths", "paths_global_short")):
        driver, p, sc = case_inputs(pkg, ob, name)
        ref = cpu.frame(driver, p, sc)
        check_schedule(ref)
        fs_scene_ref.assert_non_vacuous(ref["classes"])
        out[tag + "_params"] = np.frombuffer(p.tobytes(), dtype=np.uint8)
        out[tag + "_scene"] = np.frombuffer(np.array(sc, dtype=pkg.SCENE_S).tobytes(), dtype=np.uint8)
        for k in ("radiance_sum", "sample_count", "hit_count", "records", "info", "counts"):
            out[tag + "_" + k] = ref[k]
    return out
