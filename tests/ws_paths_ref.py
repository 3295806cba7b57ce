"""TEST INFRASTRUCTURE: the reference image of the multi-bounce estimator on scene S through the weight-space GP medium, composed on
the CPU bounce level by bounce level from pieces that exist on their own: a plain-C camera step, shade step and sums
(tests/native/ws_paths_shade.c, compiled like ws_oracle.c with the restatement flags) and a medium's sampleDistance /
transmittance over the live paths and the NEE rays (tests/native/ws_oracle.c for the weight-space medium).  It is the naive form:
every segment's realization is rebuilt, whatever the context.

The medium is a parameter (`WsMarch`, `ScMarch`): composing the same C through the sparse-convolution oracle's batch entries
must give Oracle.render_scene_s_paths bit for bit, which ties ws_paths_shade.c to the oracle the existing path driver is
checked against (tests/test_ws_paths_cpu.py)."""
import ctypes
import os
import subprocess

import numpy as np

import ws_oracle
from ws_scene_ref import scene_pixels, small_scene  # noqa: F401  (small_scene: the frame the tests start from)

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "ws_paths_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libws_paths_shade.so")
END_LIVES, END_NOT_OK, END_EXITED, END_BELOW, END_NO_CHORD = range(5)


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the path shade step")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class WsMarch:
    """the weight-space medium of (params, ws) through the C restatement"""

    def __init__(self, params, ws, wso=None):
        self.params, self.ws = params, ws
        self.wso = wso or ws_oracle.WsOracle()

    def sample_distance(self, rays):
        return self.wso.sample_distance(self.params, self.ws, rays)

    def transmittance(self, rays):
        return self.wso.transmittance(self.params, self.ws, rays)


class ScMarch:
    """a sparse-convolution medium through the oracle's batch entries (no evaluation count)"""

    def __init__(self, oracle):
        self.oracle = oracle

    def sample_distance(self, rays):
        return self.oracle.sample_distance(rays), 0

    def transmittance(self, rays):
        return self.oracle.transmittance(rays), 0


class Composite:
    """Result of compose(): image (the accumulated buffer), n_eval (the medium's evaluations), n_seg (path plus shadow segments
    marched) and the per-class counts the tests assert on."""

    def __init__(self):
        self.image = None
        self.n_eval = self.n_seg = self.n_path_seg = self.n_shadow_seg = 0
        self.n_samples = self.n_miss = 0
        self.max_hits = 0                  # most medium hits of one path
        self.n_three_hits = 0              # paths with at least 3 medium hits
        self.n_exit_after_hit = 0          # paths ended by `exited` after at least one hit
        self.n_below = self.n_no_chord = 0  # paths ended by wi.z <= 0 / by a bounce direction without a chord (before the last bounce)
        self.n_not_ok = 0
        self.n_visible = self.n_occluded = 0
        self.hit_gp_ids = set()

    def non_vacuous(self):
        """every class of sample a frame must hold (tests/test_ws_paths_cpu.py)"""
        return {"miss": self.n_miss > 0, "three_hits": self.n_three_hits > 0, "exit_after_hit": self.n_exit_after_hit > 0,
                "below_or_no_chord": self.n_below + self.n_no_chord > 0, "visible": self.n_visible > 0, "occluded": self.n_occluded > 0}


class PathsRef:
    def __init__(self, pkg):
        self.pkg = pkg
        self.lib = ctypes.CDLL(build())
        vp, sz, u32, i32, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
        self.lib.ws_paths_begin.argtypes = [vp, u32, u32, u32, vp, vp]
        self.lib.ws_paths_shade.argtypes = [vp, sz, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        self.lib.ws_paths_shade.restype = None
        self.lib.ws_paths_nee_add.argtypes = [sz, vp, vp, vp, vp]
        self.lib.ws_paths_nee_add.restype = None
        self.lib.ws_paths_sum.argtypes = [sz, vp, vp, vp]
        self.lib.ws_paths_sum.restype = None

    def begin(self, scene):
        """Every sample of the call `scene` selects, in (pixel, sample) order: segment-0 rays, stream states, alive (the ray
        meets the bound) and pixel index."""
        pkg = self.pkg
        w, s0, sn = int(scene["width"]), int(scene["spp_begin"]), int(scene["spp_count"])
        px = scene_pixels(scene)
        n = len(px) * sn
        rays = np.zeros(n, dtype=pkg.RAY_IN)
        rng = np.zeros(n, dtype=np.uint64)
        alive = np.zeros(n, dtype=np.uint8)
        pix = np.zeros(n, dtype=np.uint32)
        ray = np.zeros((), dtype=pkg.RAY_IN)
        g = ctypes.c_uint64()
        i = 0
        for x, y in px:
            for k in range(s0, s0 + sn):
                alive[i] = self.lib.ws_paths_begin(_p(scene), x, y, k, _p(ray), ctypes.byref(g))
                rays[i] = ray
                rng[i] = g.value
                pix[i] = y * w + x
                i += 1
        return rays, rng, alive, pix

    def compose(self, march, scene, max_bounces, albedo, into=None):
        """One driver call on the CPU.  `into`: a Composite of earlier calls to accumulate into (image and counts)."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        h, w = int(scene["height"]), int(scene["width"])
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w), dtype=np.float32)
        rays, rng, alive, pix = self.begin(scene)
        n = len(rays)
        c.n_samples += n
        c.n_miss += int(n - alive.sum())
        thr = np.ones(n, dtype=np.float32)
        emission = np.zeros(n, dtype=np.float32)
        hits = np.zeros(n, dtype=np.int32)
        seg = np.zeros(n, dtype=pkg.SEG_OUT)
        shadow = np.zeros(n, dtype=pkg.RAY_IN)
        contrib = np.zeros(n, dtype=np.float32)
        nee, end = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for bounce in range(int(max_bounces)):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            assert (rays["segment"][idx] == bounce).all()
            out, e = march.sample_distance(rays[idx])
            seg[idx] = out
            c.n_eval += e
            c.n_seg += len(idx)
            c.n_path_seg += len(idx)
            hit = idx[(out["ok"] != 0) & (out["exited"] == 0)]
            hits[hit] += 1
            c.hit_gp_ids |= set(int(g) for g in seg["gp_id"][hit])
            self.lib.ws_paths_shade(_p(scene), n, bounce, int(max_bounces), ctypes.c_float(albedo), _p(rays), _p(seg), _p(rng), _p(thr), _p(alive),
                                    _p(shadow), _p(contrib), _p(nee), _p(end))
            c.n_not_ok += int((end[idx] == END_NOT_OK).sum())
            c.n_exit_after_hit += int(((end[idx] == END_EXITED) & (hits[idx] > 0)).sum())
            if bounce < max_bounces - 1:                     # at the last bounce nothing after the march can be observed
                c.n_below += int((end[idx] == END_BELOW).sum())
                c.n_no_chord += int((end[idx] == END_NO_CHORD).sum())
            sidx = np.nonzero(nee)[0]
            vis = np.zeros(n, dtype=np.uint8)
            if len(sidx):
                assert (shadow["segment"][sidx] == bounce + 1).all() and (shadow["first_scatter"][sidx] == 0).all()
                v, e = march.transmittance(shadow[sidx])
                vis[sidx] = v
                c.n_eval += e
                c.n_seg += len(sidx)
                c.n_shadow_seg += len(sidx)
                c.n_visible += int((v != 0).sum())
                c.n_occluded += int((v == 0).sum())
            self.lib.ws_paths_nee_add(n, _p(nee), _p(vis), _p(contrib), _p(emission))
        self.lib.ws_paths_sum(n, _p(pix), _p(emission), _p(c.image))
        c.max_hits = max(c.max_hits, int(hits.max()) if n else 0)
        c.n_three_hits += int((hits >= 3).sum())
        return c


# ---- the frames the tests and the fixture share ---------------------------------------------------------------------------------
CTXS = ["global", "renewal_plus", "renewal", "none"]
CLASSES = ("miss", "three_hits", "exit_after_hit", "below_or_no_chord", "visible", "occluded")

# name -> (ws_params keywords, max_bounces, albedo, centre / radius of the second sphere or None, classes the frame cannot hold)
# Frame: small_scene (24 x 16 x 4, fov 60 degrees, default camera, light and seed).  N = 65 (two rounds of basis functions, the
# second with one lane) except where N is the case; N = 300 in one case only.
# Classes a case cannot hold BY CONSTRUCTION, whatever camera, fov or seed:
#   max_bounces 1 — one segment per sample: no second hit, no NEE (bounce < max_bounces - 1 never holds), and nothing after
#       the march is observed; the image is all zero and the case checks the counters;
#   max_bounces 2 — at most two segments per path, so at most two hits;
#   absorption_only — sampleDistance reports exited = 1 for every segment (GPM.cpp:304-312): no hit at all.
# N = 0 is the mean alone.  One sphere is convex and a path leaves it after one hit, and the CSG pair of ws_oracle.ws_params (a
# small sphere on the flank of the unit sphere) gives two hits at most from this camera; the second sphere of this case, radius
# 0.8 at (0, 0.9, 0.9), makes a crease that faces the camera, in which paths hit three times and shadow rays are occluded.
CASES = {}
for _c in CTXS:
    for _s in (0, 1):
        CASES["%s-single%d" % (_c, _s)] = (dict(ctx=_c, single=_s, n_basis=65), 3, 0.8, None, ())
CASES["bounces1"] = (dict(ctx="renewal", n_basis=65), 1, 0.8, None, ("three_hits", "exit_after_hit", "below_or_no_chord", "visible", "occluded"))
CASES["bounces2"] = (dict(ctx="renewal", n_basis=65), 2, 0.8, None, ("three_hits",))
CASES["bounces4"] = (dict(ctx="renewal", n_basis=65), 4, 0.8, None, ())
CASES["bounces4-global"] = (dict(ctx="global", n_basis=65), 4, 0.8, None, ())
CASES["finite_differences"] = (dict(ctx="renewal", normal=1, n_basis=65), 3, 0.8, None, ())
CASES["finite_differences-single"] = (dict(ctx="none", single=1, normal=1, n_basis=65), 3, 0.8, None, ())
CASES["n0"] = (dict(ctx="renewal", n_basis=0, mean_additional=True), 3, 0.8, ((0.0, 0.9, 0.9), 0.8), ())
CASES["n300"] = (dict(ctx="renewal_plus", n_basis=300), 3, 0.8, None, ())
CASES["two_ids"] = (dict(ctx="renewal", n_basis=65, mean_additional=True), 3, 0.8, None, ())
CASES["absorption_only"] = (dict(ctx="renewal_plus", n_basis=65, absorption_only=True), 3, 0.8, None,
                            ("three_hits", "exit_after_hit", "below_or_no_chord", "visible", "occluded"))
CASES["albedo1"] = (dict(ctx="global", n_basis=65), 3, 1.0, None, ())


def case_inputs(pkg, ob, name):
    """(params, ws params, scene, max_bounces, albedo, impossible classes) of a case"""
    kw, max_bounces, albedo, second, impossible = CASES[name]
    p, w = ws_oracle.ws_params(pkg, **kw)
    if second is not None:
        p["mean_additional"]["center"], p["mean_additional"]["radius"] = second
    return p, w, small_scene(ob), max_bounces, albedo, impossible


def check_non_vacuous(c, impossible=()):
    """Every class the frame can hold is there, and the ones it cannot hold by construction are indeed absent."""
    nv = c.non_vacuous()
    for k in CLASSES:
        assert nv[k] == (k not in impossible), (k, nv, impossible)


def parts(ob, kind):
    """scenes of the calls that together cover one frame (40 rows, so that three shards of 8-pixel tiles all get rows)"""
    def base():
        s = small_scene(ob, width=12, height=40, spp=5)
        s["tile_size"] = 8
        return s
    out = []
    if kind == "shards":
        for k in range(3):
            s = base()
            s["shard_index"], s["shard_count"] = k, 3
            out.append(s)
    elif kind == "rows":
        for y0, yc in ((0, 17), (17, 23)):
            s = base()
            s["y_begin"], s["y_count"] = y0, yc
            out.append(s)
    else:
        # "spp": the second call adds ONE sample per pixel, so ((((a0 + a1) + a2) + a3) + a4 is the whole frame's own order;
        # "spp_assoc": (a0 + a1) + ((a2 + a3) + a4), another float32 association than the whole frame's
        for s0, sn in (((0, 4), (4, 1)) if kind == "spp" else ((0, 2), (2, 3))):
            s = base()
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    return base(), out
