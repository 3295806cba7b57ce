"""TEST INFRASTRUCTURE: the reference image of the multi-bounce estimator on scene S through the function-space GP medium,
composed on the CPU bounce level by bounce level (in the style of ws_paths_ref.PathsRef.compose) from pieces that exist on their
own: the camera step of the function-space scene composite (fs_scene_ref: the oracle's primary rays, the stream state after jx,
jy), the CPU restatement of the medium (Oracle.fs_sample_distance / fs_transmittance, which take and return gpis_fs_state records
as VALUES) and the plain-C shade step cut in two around the shadow segment (tests/native/fs_paths_shade.c).

Per bounce level, for the live paths:
    seg, state      = fs_sample_distance(ray, state)          the path's context and sampler advance
    nee, shadow ray = fs_paths_nee(ray, seg)                  draws nothing
    vis, copy       = fs_transmittance(shadow ray, state)     on a copy; ONLY the sampler state comes back into the path's state
    next ray        = fs_paths_bounce(ray, seg, sampler)      disk pairs from the path's stream
so segment b + 1 is conditioned on the context segment b left, and the stream is never forked.

Two deliberate MIS-compositions exist for the sensitivity checks of tests/test_fs_paths_cpu.py:
    shadow_in_place  the path continues from the context the shadow segment left (what k_fs_scene may do, nothing following it);
    fork_sampler     the path does not take over the shadow segment's sampler state (the stream is forked at the hit)."""
import ctypes
import os
import subprocess

import numpy as np

import fs_scene_ref
import ws_oracle
import ws_paths_ref
import ws_scene_ref
from ws_paths_ref import END_BELOW, END_EXITED, END_NO_CHORD, END_NOT_OK  # noqa: F401

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "fs_paths_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libfs_paths_shade.so")
_p = ws_scene_ref._p


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, ws_paths_ref.SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
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


CLASSES = ("miss", "two_hits", "exit_after_hit", "below_or_no_chord", "visible", "occluded", "nee_then_segment")


class Composite:
    """Result of compose(): image and segs (the accumulated buffers: radiance sums, segments marched per pixel), the per-class
    counts the tests assert on and, of the LAST compose() call, the per-bounce records (`levels`: dicts of idx, rays, states,
    seg, states_after, rng_after_shadow, throughput after the weight, alive after the NEE step)."""

    def __init__(self):
        self.image = self.segs = None
        self.n_seg = self.n_path_seg = self.n_shadow_seg = 0
        self.n_samples = self.n_miss = 0
        self.max_hits = 0                   # most medium hits of one path
        self.n_two_hits = self.n_three_hits = 0
        self.n_exit_after_hit = 0           # paths ended by `exited` after at least one hit
        self.n_below = self.n_no_chord = 0  # paths ended by wi.z <= 0 / by a bounce direction without a chord (before the last bounce)
        self.n_not_ok = 0
        self.n_visible = self.n_occluded = 0
        self.n_nee_then_segment = 0         # shadow segments after which the path marched a further segment
        self.levels = None

    def non_vacuous(self):
        return {"miss": self.n_miss > 0, "two_hits": self.n_two_hits > 0, "exit_after_hit": self.n_exit_after_hit > 0,
                "below_or_no_chord": self.n_below + self.n_no_chord > 0, "visible": self.n_visible > 0, "occluded": self.n_occluded > 0,
                "nee_then_segment": self.n_nee_then_segment > 0}

    def class_counts(self):
        return np.array([self.n_samples, self.n_miss, self.n_path_seg, self.n_shadow_seg, self.n_two_hits, self.n_three_hits, self.n_exit_after_hit,
                         self.n_below, self.n_no_chord, self.n_not_ok, self.n_visible, self.n_occluded, self.n_nee_then_segment], dtype=np.int64)


class FsPathsRef:
    def __init__(self, pkg, ob, threads=8):
        self.pkg, self.ob = pkg, ob
        self.scene_ref = fs_scene_ref.FsSceneRef(pkg, ob, threads=threads)
        self.lib = ctypes.CDLL(build())
        vp, sz, i32, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
        self.lib.fs_paths_nee.argtypes = [vp, sz, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp]
        self.lib.fs_paths_nee.restype = None
        self.lib.fs_paths_bounce.argtypes = [vp, sz, i32, f32, vp, vp, vp, vp, vp, vp]
        self.lib.fs_paths_bounce.restype = None
        self.lib.ws_paths_shade.argtypes = [vp, sz, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        self.lib.ws_paths_shade.restype = None
        self.lib.ws_paths_nee_add.argtypes = [sz, vp, vp, vp, vp]
        self.lib.ws_paths_nee_add.restype = None
        self.lib.ws_paths_sum.argtypes = [sz, vp, vp, vp]
        self.lib.ws_paths_sum.restype = None

    def compose(self, params, scene, max_bounces, albedo, into=None, shadow_in_place=False, fork_sampler=False):
        """One driver call on the CPU.  `into`: a Composite of earlier calls to accumulate into (image, segs and counts)."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        h, w = int(scene["height"]), int(scene["width"])
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w), dtype=np.float32)
            c.segs = np.zeros((h, w), dtype=np.uint32)
        orc = self.scene_ref.oracle(params)
        # the camera step of fs_scene_ref: the samples that meet the bound, in (pixel, sample) order, and their empty states
        rays, _, pix, miss = self.scene_ref.base.primary_rays(scene)
        st = self.scene_ref.primary_states(scene, rays)
        n = len(rays)
        c.n_samples += n + miss
        c.n_miss += miss
        alive = np.ones(n, dtype=np.uint8)
        thr = np.ones(n, dtype=np.float32)
        emission = np.zeros(n, dtype=np.float32)
        hits = np.zeros(n, dtype=np.int32)
        segs = np.zeros(n, dtype=np.uint32)
        seg = np.zeros(n, dtype=pkg.SEG_OUT)
        shadow = np.zeros(n, dtype=pkg.RAY_IN)
        contrib = np.zeros(n, dtype=np.float32)
        nee, end = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        c.levels = []
        for bounce in range(int(max_bounces)):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            assert (rays["segment"][idx] == bounce).all()
            level = dict(idx=idx, rays=rays[idx].copy(), states=st[idx].copy())
            out, st_after = orc.fs_sample_distance(rays[idx], st[idx])
            seg[idx] = out
            st[idx] = st_after
            segs[idx] += 1
            c.n_seg += len(idx)
            c.n_path_seg += len(idx)
            hits[idx[(out["ok"] != 0) & (out["exited"] == 0)]] += 1
            self.lib.fs_paths_nee(_p(scene), n, bounce, int(max_bounces), ctypes.c_float(albedo), _p(rays), _p(seg), _p(thr), _p(alive),
                                  _p(shadow), _p(contrib), _p(nee), _p(end))
            c.n_not_ok += int((end[idx] == END_NOT_OK).sum())
            c.n_exit_after_hit += int(((end[idx] == END_EXITED) & (hits[idx] > 0)).sum())
            sidx = np.nonzero(nee)[0]
            vis = np.zeros(n, dtype=np.uint8)
            if len(sidx):
                assert (shadow["segment"][sidx] == bounce + 1).all() and (shadow["first_scatter"][sidx] == 0).all()
                v, st_shadow = orc.fs_transmittance(shadow[sidx], st[sidx])       # works on a copy
                vis[sidx] = v
                if shadow_in_place:                  # MIS-composition: the shadow segment's context becomes the path's
                    keep = st["sampler_state"][sidx].copy()
                    st[sidx] = st_shadow
                    st["sampler_state"][sidx] = keep
                if not fork_sampler:                 # the path goes on from where the shadow segment's draws stopped
                    st["sampler_state"][sidx] = st_shadow["sampler_state"]
                segs[sidx] += 1
                c.n_seg += len(sidx)
                c.n_shadow_seg += len(sidx)
                c.n_visible += int((v != 0).sum())
                c.n_occluded += int((v == 0).sum())
            self.lib.ws_paths_nee_add(n, _p(nee), _p(vis), _p(contrib), _p(emission))
            level.update(seg=out, states_after=st_after, rng_after_shadow=st["sampler_state"][idx].copy(), throughput=thr[idx].copy(),
                         alive=alive[idx].copy(), nee=nee[idx].copy(), shadow=shadow[idx].copy(), contrib=contrib[idx].copy())
            c.levels.append(level)
            if bounce + 1 >= max_bounces:            # nothing after the last segment is observable: the driver stops here
                break
            rng = np.ascontiguousarray(st["sampler_state"])
            self.lib.fs_paths_bounce(_p(scene), n, bounce, ctypes.c_float(albedo), _p(rays), _p(seg), _p(rng), _p(thr), _p(alive), _p(end))
            st["sampler_state"] = rng
            c.n_below += int((end[idx] == END_BELOW).sum())
            c.n_no_chord += int((end[idx] == END_NO_CHORD).sum())
            c.n_nee_then_segment += int(((nee != 0) & (alive != 0)).sum())
        self.lib.ws_paths_sum(n, _p(pix), _p(emission), _p(c.image))
        np.add.at(c.segs.reshape(-1), pix, segs)
        c.max_hits = max(c.max_hits, int(hits.max()) if n else 0)
        c.n_two_hits += int((hits >= 2).sum())
        c.n_three_hits += int((hits >= 3).sum())
        return c


# ---- the media and frames the tests, the fixture and the bench share ------------------------------------------------------------
def absorption_only(p):
    p = p.copy()
    p["sigma_a"], p["sigma_s"] = 1.0, 0.0
    return p


# name -> (context, fs_sample_points, fs_step_size, fs_params keywords, (width, height, spp), max_bounces, albedo, absorption_only,
#          classes the frame cannot hold)
# Frames: ws_scene_ref.small_scene (fov 60 degrees, default camera, light and seed), media: fs_scene_ref.fs_params (sigma 0.1,
# length scale 0.05, spherical mean of radius 1) with the points / step of fs_scene_ref.CASES.  These were tried first, on the
# CPU, and every one of them holds every class it can hold (tests/test_fs_paths_cpu.py: EXPECTED records the counts), so sigma,
# length scale, mean radius, fov and seed stayed at the values of fs_scene_ref: the field is rough enough at sigma 0.1 / length
# scale 0.05 for paths to hit the surface again after a bounce.
# Classes a case cannot hold BY CONSTRUCTION:
#   max_bounces 1 — one segment per sample: no second hit, no NEE, nothing after the march is observed (the image is all zero);
#   max_bounces 2 — two segments per path at most: two hits at most (three_hits is asked of no such case), but one NEE and a
#       further segment, so every class of CLASSES is possible;
#   absorption_only — sampleDistance reports exited = 1 for every segment (GPM.cpp:304-312): no hit at all.
#
# One class of the weight-space composite (ws_paths_ref.CLASSES) this medium excludes in EVERY frame of scene S, whatever sigma,
# length scale, mean, fov or seed — a path ended by wi.z <= 0 or by a bounce direction without a chord:
#   wi.z <= 0 — sampleDistance itself refuses a hit whose gradient points along the ray (aniso . dir > 0 in double gives !ok:
#       gpis_fs.hpp, fs_sample_distance_one), so a hit the path driver sees has n . (-dir) >= 0, and wi.z could be
#       <= 0 only through the float32 rounding of an exactly grazing hit;
#   no chord — a hit lies at t < far_t on a chord of the bounding sphere, strictly inside it, and every direction from an inside
#       point has a chord.
# A sweep over sigma 0.05 / 0.1 / 0.5, length scale 0.02 / 0.05 / 0.3, mean radius 0.6 .. 1.6 and a homogeneous mean, fov 35 / 60
# and two seeds at 4 bounces marched 426 332 path segments on the CPU without one such end.  The branches are in the kernel and in
# fs_paths_shade.c all the same (the pin against ws_paths_shade.c covers their arithmetic on records altered so that paths do end so); every case
# asserts that the class is absent, so a frame that does reach it will be noticed.
EXCLUDED_BY_THE_MEDIUM = ("below_or_no_chord",)
NO_HIT = ("two_hits", "exit_after_hit", "below_or_no_chord", "visible", "occluded", "nee_then_segment")
CASES = {
    "renewal-16": ("RENEWAL", 16, 0.04, {}, (24, 16, 4), 3, 0.8, False, ()),
    "none-12": ("NONE", 12, 0.0, {}, (24, 16, 4), 3, 0.8, False, ()),
    "global-14": ("GLOBAL", 14, 0.05, {}, (24, 16, 4), 3, 0.8, False, ()),
    "renewal_plus-32": ("RENEWAL_PLUS", 32, 0.02, {}, (24, 16, 4), 3, 0.8, False, ()),
    "global-64": ("GLOBAL", 64, 0.01, {}, (12, 8, 2), 3, 0.8, False, ()),
    "bounces1": ("RENEWAL", 16, 0.04, {}, (24, 16, 4), 1, 0.8, False, NO_HIT),
    "bounces2": ("RENEWAL", 16, 0.04, {}, (24, 16, 4), 2, 0.8, False, ()),
    "bounces4": ("RENEWAL_PLUS", 16, 0.04, {}, (24, 16, 4), 4, 0.8, False, ()),
    "albedo1": ("GLOBAL", 14, 0.05, {}, (24, 16, 4), 3, 1.0, False, ()),
    "aniso": ("RENEWAL", 16, 0.04, dict(aniso=(1.0, 0.7, 1.4)), (24, 16, 4), 3, 0.8, False, ()),
    "homogeneous": ("RENEWAL", 16, 0.04, dict(mean="HOMOGENEOUS", offset=0.05), (24, 16, 4), 3, 0.8, False, ()),
    "absorption_only": ("RENEWAL_PLUS", 16, 0.04, {}, (24, 16, 4), 3, 0.8, True, NO_HIT),
}
THREE_HITS = ("bounces4",)          # cases that must hold a path with at least three hits


def case(pkg, ob, name):
    """(params, scene, max_bounces, albedo, impossible classes) of a case"""
    ctx, n, step, kw, (w, h, spp), max_bounces, albedo, absorb, impossible = CASES[name]
    p = fs_scene_ref.fs_params(pkg, ctx, n, step, **kw)
    if absorb:
        p = absorption_only(p)
    return p, ws_scene_ref.small_scene(ob, w, h, spp, fov=60.0), max_bounces, albedo, impossible


def check_non_vacuous(c, impossible=()):
    """Every class the frame can hold is there, and the ones it cannot hold by construction are indeed absent."""
    nv = c.non_vacuous()
    impossible = tuple(impossible) + EXCLUDED_BY_THE_MEDIUM
    for k in CLASSES:
        assert nv[k] == (k not in impossible), (k, nv, impossible)
