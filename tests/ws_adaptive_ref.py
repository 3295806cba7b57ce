"""TEST INFRASTRUCTURE: the cases and the CPU composite of the weight-space adaptive drivers (gpis_ws_render_scene_s_adaptive,
gpis_ws_render_scene_s_paths_adaptive).  A sample is a pure function of (x, y, k, scene_seed), so a frame is the schedule of
tests/adaptive_ref.py over per-sample values that one uniform-driver call with spp_count = 1 gives: here the CPU composites
ws_scene_ref.SceneRef.compose and ws_paths_ref.PathsRef.compose, in tests/test_gpu_ws_adaptive.py the uniform GPU entries.  Neither
uses the code under test.

The frame is adaptive_ref's small one (22 x 14, camera at (0, 0, 8): 6 x 4 records, clipped tiles on two edges, a 16-pixel tile
boundary inside); the media are ws_oracle.ws_params with step_size 0.05 and small bases, so a case is a few thousand samples."""
import os

import numpy as np

import adaptive_ref as ar
import ws_oracle
import ws_paths_ref
import ws_scene_ref

W, H = ar.SMALL_W, ar.SMALL_H
GOLDEN = os.path.join(ws_oracle.ROOT, "tests", "golden", "ws_adaptive_small.npz")
BOUNCES, ALBEDO = 3, 0.8

# name -> (driver, ws_params keywords, scene fields)
CASES = {
    "lambert_renewal": ("lambert", dict(ctx="renewal", n_basis=32), {}),
    "lambert_single": ("lambert", dict(ctx="renewal", single=1, n_basis=32), {}),
    "lambert_global_short": ("lambert", dict(ctx="global", n_basis=8), {"spp_count": 40}),
    "lambert_finite_differences": ("lambert", dict(ctx="renewal", normal=1, n_basis=32), {}),
    "paths_renewal": ("paths", dict(ctx="renewal", n_basis=32), {}),
    "paths_global": ("paths", dict(ctx="global", n_basis=8), {}),
    "paths_single_short": ("paths", dict(ctx="renewal", single=1, n_basis=32), {"spp_count": 40}),
}
# a light bright enough for renderTile's clamp (values above 65536 count as 0)
CLAMP_CASES = {
    "lambert_clamp": ("lambert", dict(ctx="renewal", n_basis=32), {"light_radiance": 1e5}),
    "paths_clamp": ("paths", dict(ctx="renewal", n_basis=8), {"light_radiance": 1e6}),
}


def medium(pkg, **kw):
    p, w = ws_oracle.ws_params(pkg, **kw)
    p["step_size"] = 0.05
    return p, w


def scene(ob, spp=ar.SMALL_SPP, **fields):
    s = ob.default_scene_s(W, H, spp)
    s["cam_pos"] = (0.0, 0.0, 8.0)
    for k, v in fields.items():
        s[k] = v
    return s


def case_inputs(pkg, ob, name):
    """(driver, params, ws params, scene) of a case"""
    driver, kw, fields = dict(CASES, **CLAMP_CASES)[name]
    p, w = medium(pkg, **kw)
    return driver, p, w, scene(ob, **fields)


def frame(render_one, sc, adaptive=None):
    """adaptive_ref.frame over render_one(scene with spp_count = 1) -> (image, hits); adds the largest sample value seen"""
    seen = []

    def one(s):
        img, hits = render_one(s)
        seen.append(float(np.max(img)))
        return img, hits
    ref = ar.frame(ar.default_adaptive() if adaptive is None else adaptive, int(sc["width"]), int(sc["height"]), int(sc["spp_count"]),
                   ar.per_sample_values(one, sc))
    ref["largest_value"] = max(seen)
    return ref


def check_schedule(ref):
    """what keeps a degenerate schedule from passing: three passes, the first uniform at 16, later ones mixing 1 with more than 16"""
    counts = ref["counts"]
    assert len(counts) == 3 and (counts[0] == 16).all() and (counts[1:] == 1).any() and counts[1].max() > 16, [(int(c.min()), int(c.max())) for c in counts]


class CpuRenderer:
    """the two uniform drivers on the CPU, one call at a time"""

    def __init__(self, pkg, ob):
        self.pkg, self.ob = pkg, ob
        self.wso = ws_oracle.WsOracle()
        self.scene_ref = ws_scene_ref.SceneRef(pkg, ob, self.wso)
        self.paths_ref = ws_paths_ref.PathsRef(pkg)

    def render_one(self, driver, p, w):
        if driver == "lambert":
            def one(s):
                c = self.scene_ref.compose(p, w, s)
                return c.image, c.hits
        else:
            march = ws_paths_ref.WsMarch(p, w, self.wso)

            def one(s):
                c = self.paths_ref.compose(march, s, BOUNCES, ALBEDO)
                return c.image, np.zeros(c.image.shape, dtype=np.uint8)
        return one

    def frame(self, driver, p, w, sc, adaptive=None):
        return frame(self.render_one(driver, p, w), sc, adaptive)

    def costs(self, driver, p, w, sc, per_pixel, march=None):
        """(n_eval, n_seg) the reference spends on the samples k < per_pixel[y, x] of every pixel: the composite of the uniform
        driver over exactly the samples a schedule used.  `march`: what marches the segments instead of the C restatement (a
        BatchMarch, whose medium then holds the device's counters of the same segments; n_eval is 0 then)."""
        per_pixel = np.asarray(per_pixel)
        n_eval = n_seg = 0
        for k in range(int(per_pixel.max())):
            one = np.array(sc).copy()
            one["spp_begin"], one["spp_count"] = int(sc["spp_begin"]) + k, 1
            keep = (per_pixel > k).reshape(-1)
            if driver == "lambert":
                c = _MaskedScene(self.scene_ref, keep, march or self.wso).compose(p, w, one)
            else:
                c = _MaskedPaths(self.paths_ref, keep).compose(march or ws_paths_ref.WsMarch(p, w, self.wso), one, BOUNCES, ALBEDO)
            n_eval, n_seg = n_eval + c.n_eval, n_seg + c.n_seg
        return n_eval, n_seg


class BatchMarch:
    """The batch entries of a WeightSpaceMedium on the GPU as the march of either composite (ws_oracle.WsOracle's and
    ws_paths_ref.WsMarch's signatures).  A segment costs the same evaluations there as inside the fused frame kernels (one
    ws_sample_distance / ws_transmittance_one per segment either way), so after a composite the medium's counters hold what
    exactly those segments cost on the device."""

    def __init__(self, pkg, med):
        self.pkg, self.med = pkg, med

    def sample_distance(self, *args):
        rays = args[-1]
        return (self.med.sample_distance_batch(rays) if len(rays) else np.zeros(0, dtype=self.pkg.SEG_OUT)), 0

    def transmittance(self, *args):
        rays = args[-1]
        return (self.med.transmittance_batch(rays) if len(rays) else np.zeros(0, dtype=np.uint8)), 0


class _MaskedScene(ws_scene_ref.SceneRef):
    """SceneRef over the pixels of a mask only"""

    def __init__(self, base, keep, wso):
        self.__dict__.update(base.__dict__)
        self.keep, self.wso = keep, wso

    def primary_rays(self, sc):
        rays, us, pix, miss = super().primary_rays(sc)
        k = self.keep[pix]
        return rays[k], us[k], pix[k], miss


class _MaskedPaths(ws_paths_ref.PathsRef):
    """PathsRef over the pixels of a mask only: the other samples start dead"""

    def __init__(self, base, keep):
        self.__dict__.update(base.__dict__)
        self.keep = keep

    def begin(self, sc):
        rays, rng, alive, pix = super().begin(sc)
        alive[~self.keep[pix]] = 0
        return rays, rng, alive, pix


def golden_arrays(pkg, ob, cpu=None):
    """the contents of tests/golden/ws_adaptive_small.npz, from the CPU composites alone"""
    cpu = cpu or CpuRenderer(pkg, ob)
    out = {"adaptive": ar.default_adaptive(), "max_bounces": np.int32(BOUNCES), "albedo": np.float32(ALBEDO)}
    for tag, name in (("lambert", "lambert_renewal"), ("paths", "paths_global")):
        driver, p, w, sc = case_inputs(pkg, ob, name)
        ref = cpu.frame(driver, p, w, sc)
        check_schedule(ref)
        out[tag + "_params"] = np.frombuffer(p.tobytes(), dtype=np.uint8)
        out[tag + "_ws"] = np.frombuffer(w.tobytes(), dtype=np.uint8)
        out[tag + "_scene"] = np.frombuffer(np.array(sc, dtype=pkg.SCENE_S).tobytes(), dtype=np.uint8)
        for k in ("radiance_sum", "sample_count", "hit_count", "records", "info", "counts"):
            out[tag + "_" + k] = ref[k]
    return out
