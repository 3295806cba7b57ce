"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_nee_paths_rgb, the conductor NEE / MIS path estimator on scene S in RGB
with the medium's emission, composed on the CPU bounce level by bounce level — one call per bounce over all live samples — from the
oracle's batch entries (oracle_scene_s_primary, oracle_sample_distance_batch with its coefficients, oracle_nee_pdf_batch,
oracle_nee_grad_batch, oracle_transmittance_batch, oracle_mean_color_emission) and a plain-C restatement in float of the set-up,
shade, bounce and gather step (tests/native/nee_paths_rgb_shade.c, compiled with the flags of oracle/Makefile).

tests/test_nee_paths_rgb_cpu.py ties the C file to tests/nee_paths_ref.py's mono composite, which is itself pinned to
oracle_render_scene_s_nee."""
import ctypes
import os
import subprocess

import numpy as np

import nee_paths_ref as npr
import ws_oracle
from ws_scene_ref import scene_pixels

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "nee_paths_rgb_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libnee_paths_rgb_shade.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "nee_paths_rgb_small.npz")

# numpy mirror of nee_paths_rgb_shade.c's nee_paths_rgb_hit
HIT = np.dtype([
    ("d", "<f4", 3), ("w", "<f4", 3), ("F", "<f4", 3), ("thr", "<f4", 3), ("scheme", "<i4"),
    ("hit", "u1"), ("want_light", "u1"), ("want_phase", "u1"), ("want_pdf_normal", "u1"),
    ("pdf_half", "<f4"), ("grad_half", "<f4", 3), ("pdf_normal", "<f4"),
    ("go_light", "u1"), ("go_phase", "u1"), ("vis_light", "u1"), ("vis_phase", "u1"),
    ("contrib_light", "<f4", 3), ("contrib_phase", "<f4", 3),
], align=True)


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the RGB NEE path shade step")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def shade_lib():
    lib = ctypes.CDLL(build())
    vp, sz, u32, i32, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
    lib.nee_paths_rgb_hit_size.restype = sz
    assert lib.nee_paths_rgb_hit_size() == HIT.itemsize
    lib.nee_paths_rgb_stream.argtypes = [vp, u32, u32, u32]
    lib.nee_paths_rgb_stream.restype = ctypes.c_uint64
    lib.nee_paths_rgb_fresnel.argtypes = [vp, f32, vp]
    lib.nee_paths_rgb_fresnel.restype = None
    lib.nee_paths_rgb_points.argtypes = [sz] + [vp] * 5
    lib.nee_paths_rgb_points.restype = None
    lib.nee_paths_rgb_setup.argtypes = [vp, vp, sz, i32, i32, i32] + [vp] * 12
    lib.nee_paths_rgb_setup.restype = None
    lib.nee_paths_rgb_shade.argtypes = [vp, vp, sz, i32, i32] + [vp] * 9
    lib.nee_paths_rgb_shade.restype = None
    lib.nee_paths_rgb_gather.argtypes = [vp, sz, vp, vp]
    lib.nee_paths_rgb_gather.restype = None
    lib.nee_paths_rgb_sum.argtypes = [sz, vp, vp, vp, vp, vp]
    lib.nee_paths_rgb_sum.restype = None
    return lib


def emissive(params):
    return int(params["mean_emission"]["enabled"]) != 0


def without_emission(params):
    p = np.array(params).copy()
    p["mean_emission"]["enabled"] = 0
    return p


def channel_surface(pkg, surface, c):
    """the mono surface that carries channel c of an RGB surface"""
    surface = np.array(surface, dtype=pkg.SURFACE_RGB_S).reshape(())
    s = np.zeros((), dtype=pkg.SURFACE_S)
    for key in ("eta", "k", "albedo", "cap_radiance"):
        s[key] = surface[key][c]
    s["cap_cos"] = surface["cap_cos"]
    return s


def grey_surface(pkg, surface):
    """the RGB surface whose three channels are a mono surface"""
    surface = np.array(surface, dtype=pkg.SURFACE_S).reshape(())
    s = np.zeros((), dtype=pkg.SURFACE_RGB_S)
    for key in ("eta", "k", "albedo", "cap_radiance"):
        s[key] = surface[key]
    s["cap_cos"] = surface["cap_cos"]
    return s


class Composite:
    """Result of compose(): image (H, W, 3) and seg_count (H, W) (the accumulated buffers), n_seg (= seg_count.sum()), and per bounce
    the segments marched (`marched`), the hits the estimators follow (`hits`), the segments that left the medium (`exits`), the
    light / phase shadow segments marched (`light`, `phase`) and those of the light's that were visible (`light_visible`); of the
    LAST call composed the per-sample emission sums (`sample_em`) and pixel indices (`pix`)."""

    def __init__(self):
        self.image = self.seg_count = None
        self.n_samples = self.n_miss = 0
        self.marched, self.hits, self.exits, self.light, self.phase, self.light_visible = [], [], [], [], [], []
        self.sample_em = self.pix = None

    @property
    def n_seg(self):
        return int(self.seg_count.sum())

    def _count(self, lst, bounce, k):
        while len(lst) <= bounce:
            lst.append(0)
        lst[bounce] += int(k)


class NeePathsRgbRef:
    def __init__(self, pkg, ob):
        self.pkg, self.ob = pkg, ob
        self.lib = shade_lib()

    def fresnel(self, surface, cos_theta):
        surface = np.array(surface, dtype=self.pkg.SURFACE_RGB_S).reshape(())
        out = np.zeros(3, dtype=np.float32)
        self.lib.nee_paths_rgb_fresnel(_p(surface), ctypes.c_float(cos_theta), _p(out))
        return out

    def begin(self, orc, scene):
        """Every sample of the call `scene` selects, in (pixel, sample) order: the segment-0 ray of oracle_scene_s_primary, the
        stream's state after jx, jy and the march jitter, alive (the ray meets the bound) and the pixel index."""
        pkg = self.pkg
        w, s0, sn = int(scene["width"]), int(scene["spp_begin"]), int(scene["spp_count"])
        px = scene_pixels(scene)
        n = len(px) * sn
        rays = np.zeros(n, dtype=pkg.RAY_IN)
        rng = np.zeros(n, dtype=np.uint64)
        alive = np.zeros(n, dtype=np.uint8)
        pix = np.zeros(n, dtype=np.uint32)
        i = 0
        for x, y in px:
            for k in range(s0, s0 + sn):
                hit, ray, _ = orc.scene_s_primary(scene, x, y, k)
                rays[i] = ray
                alive[i] = 1 if hit else 0
                rng[i] = self.lib.nee_paths_rgb_stream(_p(scene), x, y, k)
                pix[i] = y * w + x
                i += 1
        return rays, rng, alive, pix

    def compose(self, orc, scene, surface, max_bounces, into=None):
        """One driver call on the CPU through the oracle `orc`.  `into`: a Composite of earlier calls to accumulate into."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        surface = np.array(surface, dtype=pkg.SURFACE_RGB_S).reshape(())
        max_bounces = int(max_bounces)
        assert max_bounces >= 1 and -1.0 < float(surface["cap_cos"]) < 1.0
        h, w = int(scene["height"]), int(scene["width"])
        E = emissive(orc.params)
        n_marched = max_bounces if E else max_bounces - 1
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w, 3), dtype=np.float32)
            c.seg_count = np.zeros((h, w), dtype=np.uint32)
        rays, rng, alive, pix = self.begin(orc, scene)
        n = len(rays)
        c.n_samples += n
        c.n_miss += int(n - alive.sum())
        thr = np.ones((n, 3), dtype=np.float32)
        em = np.zeros((n, 3), dtype=np.float32)
        segs = np.zeros(n, dtype=np.uint32)
        seg = np.zeros(n, dtype=pkg.SEG_OUT)
        coeff = np.zeros(n, dtype=pkg.COND_COEFF)
        hits = np.zeros(n, dtype=HIT)
        q_half, q_normal = np.zeros(n, dtype=pkg.NEE_QUERY), np.zeros(n, dtype=pkg.NEE_QUERY)
        sh_light, sh_phase = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=pkg.RAY_IN)
        for bounce in range(n_marched):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            assert (rays["segment"][idx] == bounce).all() and (rays["first_scatter"][idx] == (1 if bounce == 0 else 0)).all()
            seg[idx], coeff[idx] = orc.sample_distance(rays[idx], want_coeff=True)
            c._count(c.marched, bounce, len(idx))
            c._count(c.exits, bounce, (seg["exited"][idx] != 0).sum())
            surf, points = np.zeros(n, dtype=np.uint8), np.zeros((n, 3), dtype=np.float64)
            e = np.zeros((n, 3), dtype=np.float32)
            if E:
                self.lib.nee_paths_rgb_points(n, _p(alive), _p(rays), _p(seg), _p(surf), _p(points))
                k = np.nonzero(surf)[0]
                if len(k):
                    e[k] = orc.mean_color_emission(points[k])[1]
            self.lib.nee_paths_rgb_setup(_p(scene), _p(surface), n, bounce, max_bounces, 1 if E else 0, _p(alive), _p(rays), _p(seg), _p(coeff), _p(e),
                                         _p(rng), _p(thr), _p(em), _p(segs), _p(hits), _p(q_half), _p(q_normal))
            c._count(c.hits, bounce, hits["hit"].sum())
            if bounce + 1 >= max_bounces:
                assert not hits["hit"].any() and not alive.any()
                break
            k = np.nonzero(hits["want_light"])[0]
            if len(k):
                hits["pdf_half"][k] = orc.nee_pdf(q_half[k])
                hits["grad_half"][k] = orc.nee_grad(q_half[k])
            k = np.nonzero(hits["want_pdf_normal"])[0]
            if len(k):
                hits["pdf_normal"][k] = orc.nee_pdf(q_normal[k])
            self.lib.nee_paths_rgb_shade(_p(scene), _p(surface), n, bounce, n_marched, _p(alive), _p(rays), _p(seg), _p(rng), _p(thr), _p(segs),
                                         _p(hits), _p(sh_light), _p(sh_phase))
            for go, vis, sh, lst in (("go_light", "vis_light", sh_light, c.light), ("go_phase", "vis_phase", sh_phase, c.phase)):
                k = np.nonzero(hits[go])[0]
                c._count(lst, bounce, len(k))
                if len(k):
                    assert (sh["segment"][k] == bounce + 1).all() and (sh["first_scatter"][k] == 0).all()
                    hits[vis][k] = orc.transmittance(sh[k])
            c._count(c.light_visible, bounce, (hits["go_light"] & hits["vis_light"]).sum())
            self.lib.nee_paths_rgb_gather(_p(surface), n, _p(hits), _p(em))
        self.lib.nee_paths_rgb_sum(n, _p(pix), _p(em), _p(segs), _p(c.image), _p(c.seg_count))
        c.sample_em, c.pix = em, pix
        return c


# ---- the frame, the media and the surfaces the tests and the fixture share -------------------------------------------------------
W, H, SPP = 22, 15, 3              # 990 samples: four workgroups, a multiple of neither 64 nor 256; clipped 4x4 and 16x16 tiles
BOUNCES = (1, 2, 4)
GOLDEN_BOUNCES = 4


def frame(ob):
    return ob.default_scene_s(W, H, SPP)


def copper(pkg, **kw):
    """the default surface under a coloured light bright enough that float rounding differs per channel"""
    s = pkg.default_surface_rgb()
    s["cap_radiance"] = (20.0, 15.0, 10.0)
    for k, v in kw.items():
        s[k] = v
    return s


def _emissive(pkg):
    # nee_paths_ref's colour medium (a mean-colour ramp and absorption: three different weights) with a left-right emission ramp
    p = npr._colour(pkg)
    e = p["mean_emission"]
    e["enabled"], e["type"] = 1, 1
    e["min"], e["max"], e["start"], e["end"] = 0.05, 0.5, -1.0, 1.0
    return p


# name -> (params, surface): the three schemes on C2 (UNI with the wide cap of nee_paths_ref) and the emissive colour medium
CASES = {
    "uni": lambda pkg: (npr._c2(pkg, "uni"), copper(pkg, cap_cos=0.9)),
    "nee": lambda pkg: (npr._c2(pkg, "nee"), copper(pkg)),
    "mis": lambda pkg: (npr._c2(pkg, "mis"), copper(pkg)),
    "mis-emission": lambda pkg: (_emissive(pkg), copper(pkg)),
}
GREY_CASES = ("uni", "nee", "mis")         # media without emission whose three weights are equal
EMISSIVE_CASE = "mis-emission"


def parts(ob, kind):
    """scenes of the calls that together cover the frame: two row ranges, the spp ranges {0}, {1, 2}, or 2 shards of 4-pixel tile
    rows (4 tile rows: 2 and 2)"""
    out = []
    if kind == "rows":
        for y0, yc in ((0, 7), (7, H - 7)):
            s = frame(ob)
            s["y_begin"], s["y_count"] = y0, yc
            out.append(s)
    elif kind == "spp":
        # (a0) + (a1 + a2) is another float32 association than the whole frame's (a0 + a1) + a2: compare with the sum of the parts'
        # own composites
        for s0, sn in ((0, 1), (1, 2)):
            s = frame(ob)
            s["spp_begin"], s["spp_count"] = s0, sn
            out.append(s)
    else:
        for k in range(2):
            s = frame(ob)
            s["tile_size"], s["shard_index"], s["shard_count"] = 4, k, 2
            out.append(s)
    return out


_memo = {}


def reference(pkg, ob, name, max_bounces, surface=None, emission=True, threads=16):
    """the composite of case `name` on the whole frame (computed once per process, never modified by its users); `surface`: another
    RGB surface than the case's own; emission=False: the same medium with mean_emission switched off"""
    params, own = CASES[name](pkg)
    surface = np.array(own if surface is None else surface, dtype=pkg.SURFACE_RGB_S).reshape(())
    key = (name, int(max_bounces), surface.tobytes(), bool(emission))
    if key not in _memo:
        if not emission:
            params = without_emission(params)
        orc = ob.Oracle(params, threads=threads)
        c = NeePathsRgbRef(pkg, ob).compose(orc, frame(ob), surface, max_bounces)
        c.image.setflags(write=False)
        c.seg_count.setflags(write=False)
        _memo[key] = c
    return _memo[key]


_mono_memo = {}


def mono_reference(pkg, ob, name, max_bounces, surface, threads=16):
    """nee_paths_ref's mono composite on this module's frame and case `name`'s medium (without emission) for a mono surface"""
    surface = np.array(surface, dtype=pkg.SURFACE_S).reshape(())
    key = (name, int(max_bounces), surface.tobytes())
    if key not in _mono_memo:
        params, _ = CASES[name](pkg)
        orc = ob.Oracle(without_emission(params), threads=threads)
        _mono_memo[key] = npr.NeePathsRef(pkg, ob).compose(orc, frame(ob), surface, max_bounces)
    return _mono_memo[key]
