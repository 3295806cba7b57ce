"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_paths_rgb, the Lambert multi-bounce estimator on scene S in RGB with the
medium's emission, composed on the CPU bounce level by bounce level — one call per bounce over all live samples — from the
oracle's batch entries (oracle_scene_s_primary, oracle_sample_distance_batch, oracle_transmittance_batch,
oracle_mean_color_emission) and a plain-C restatement in float of the set-up, shade, emission add, NEE add and pixel sum
(tests/native/paths_rgb_shade.c, compiled with the flags of oracle/Makefile).

tests/test_paths_rgb_cpu.py ties the C file to the oracle: without emission every channel of a composite must equal
oracle_render_scene_s_paths, bit for bit, for the medium and albedo with that channel rolled to the front."""
import ctypes
import os
import subprocess

import numpy as np

import ws_oracle
from ws_scene_ref import scene_pixels

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "paths_rgb_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libpaths_rgb_shade.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "paths_rgb_small.npz")


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the RGB path shade step")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def shade_lib():
    lib = ctypes.CDLL(build())
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    lib.paths_rgb_stream.argtypes = [vp, u32, u32, u32]
    lib.paths_rgb_stream.restype = ctypes.c_uint64
    lib.paths_rgb_begin.argtypes = [sz, vp, vp, vp]
    lib.paths_rgb_begin.restype = None
    lib.paths_rgb_setup.argtypes = [sz] + [vp] * 6
    lib.paths_rgb_setup.restype = None
    lib.paths_rgb_shade.argtypes = [vp, sz, i32, i32, i32] + [vp] * 14
    lib.paths_rgb_shade.restype = None
    lib.paths_rgb_nee_add.argtypes = [sz, vp, vp, vp, vp]
    lib.paths_rgb_nee_add.restype = None
    lib.paths_rgb_sum.argtypes = [sz, vp, vp, vp, vp, vp]
    lib.paths_rgb_sum.restype = None
    return lib


def emissive(params):
    return int(params["mean_emission"]["enabled"]) != 0


def without_emission(params):
    p = np.array(params).copy()
    p["mean_emission"]["enabled"] = 0
    return p


class Level:
    """What one bounce level of the last compose() call did, per sample of that call (arrays of n or (n, 3)): `marched` (a path
    segment), `hit`, `points` (where the emission was evaluated), `thr_before` and `e` of the emission term (zeros unless the
    medium emits and the sample hit), `nee` (a shadow segment was marched), `vis` and `contrib` of the NEE term."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Composite:
    """Result of compose(): image (H, W, 3) and seg_count (H, W) (the accumulated buffers), n_seg (= seg_count.sum()), per bounce
    the segments marched (`marched`), the hits (`hits`) and the shadow segments marched (`shadow`), and of the LAST call composed
    its bounce levels (`levels`), per-sample emission sums (`sample_em`) and pixel indices (`pix`)."""

    def __init__(self):
        self.image = self.seg_count = None
        self.n_samples = self.n_miss = 0
        self.marched, self.hits, self.shadow = [], [], []
        self.levels, self.sample_em, self.pix = [], None, None

    @property
    def n_seg(self):
        return int(self.seg_count.sum())

    def _count(self, lst, bounce, k):
        while len(lst) <= bounce:
            lst.append(0)
        lst[bounce] += int(k)


class PathsRgbRef:
    def __init__(self, pkg, ob):
        self.pkg, self.ob = pkg, ob
        self.lib = shade_lib()

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
                rng[i] = self.lib.paths_rgb_stream(_p(scene), x, y, k)
                pix[i] = y * w + x
                i += 1
        return rays, rng, alive, pix

    def compose(self, orc, scene, max_bounces, albedo, into=None):
        """One driver call on the CPU through the oracle `orc`.  `into`: a Composite of earlier calls to accumulate into."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        albedo = np.ascontiguousarray(np.broadcast_to(np.asarray(albedo, dtype=np.float32), (3,)))
        max_bounces = int(max_bounces)
        assert max_bounces >= 1
        h, w = int(scene["height"]), int(scene["width"])
        E = emissive(orc.params)
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w, 3), dtype=np.float32)
            c.seg_count = np.zeros((h, w), dtype=np.uint32)
        rays, rng, alive, pix = self.begin(orc, scene)
        n = len(rays)
        c.n_samples += n
        c.n_miss += int(n - alive.sum())
        thr, em = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
        segs = np.zeros(n, dtype=np.uint32)
        self.lib.paths_rgb_begin(n, _p(thr), _p(em), _p(segs))
        seg = np.zeros(n, dtype=pkg.SEG_OUT)
        shadow = np.zeros(n, dtype=pkg.RAY_IN)
        c.levels = []
        # the segment max_bounces - 1 is marched only by an emissive medium: its hit emits, and nothing follows it
        for bounce in range(max_bounces if E else max_bounces - 1):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            assert (rays["segment"][idx] == bounce).all() and (rays["first_scatter"][idx] == (1 if bounce == 0 else 0)).all()
            marched = alive.copy()
            seg[idx] = orc.sample_distance(rays[idx])
            c._count(c.marched, bounce, len(idx))
            hit, points = np.zeros(n, dtype=np.uint8), np.zeros((n, 3), dtype=np.float64)
            self.lib.paths_rgb_setup(n, _p(alive), _p(rays), _p(seg), _p(segs), _p(hit), _p(points))
            c._count(c.hits, bounce, hit.sum())
            e = np.zeros((n, 3), dtype=np.float32)
            k = np.nonzero(hit)[0]
            if E and len(k):
                e[k] = orc.mean_color_emission(points[k])[1]
            thr_before, contrib = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
            nee, vis = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            self.lib.paths_rgb_shade(_p(scene), n, bounce, max_bounces, 1 if E else 0, _p(albedo), _p(rays), _p(seg), _p(hit), _p(e), _p(rng),
                                     _p(thr), _p(em), _p(segs), _p(alive), _p(thr_before), _p(shadow), _p(contrib), _p(nee))
            k = np.nonzero(nee)[0]
            c._count(c.shadow, bounce, len(k))
            if len(k):
                assert bounce < max_bounces - 1
                assert (shadow["segment"][k] == bounce + 1).all() and (shadow["first_scatter"][k] == 0).all()
                vis[k] = orc.transmittance(shadow[k])
            self.lib.paths_rgb_nee_add(n, _p(nee), _p(vis), _p(contrib), _p(em))
            c.levels.append(Level(marched=marched, hit=hit, points=points, thr_before=thr_before, e=e, nee=nee, vis=vis, contrib=contrib))
        self.lib.paths_rgb_sum(n, _p(pix), _p(em), _p(segs), _p(c.image), _p(c.seg_count))
        c.sample_em, c.pix = em, pix
        return c


# ---- the frame and the media the tests and the fixture share --------------------------------------------------------------------
W, H, SPP = 24, 20, 3              # 1440 samples: a multiple of neither 64 nor 256
BOUNCES = (1, 2, 4)
GOLDEN_BOUNCES = 4
ALBEDO = (0.8, 0.6, 0.4)
GUIDE = (16, 8)


def frame(ob):
    return ob.default_scene_s(W, H, SPP)


def _ramp(r, typ, lo, hi, start=-1.0, end=1.0):
    r["enabled"], r["type"] = 1, typ
    r["min"], r["max"], r["start"], r["end"] = lo, hi, start, end


def _emission_ramp(p):
    _ramp(p["mean_emission"], 1, 0.05, 0.5)        # left-right, at most 0.5


def _grey(pkg):
    return pkg.params_for_config("C1")


def _sigma(pkg):
    p = pkg.params_for_config("C1")
    p["sigma_a"] = (0.25, 0.5, 1.0)
    return p


def _ramp_case(pkg):
    # the mean-colour bounds of nee_paths_ref._colour, as the two-ramp product (type 3); ramp noises have three equal components
    p = pkg.params_for_config("C0")
    c = p["mean_color"]
    _ramp(c, 3, 0.2, 0.9)
    c["min2"], c["max2"], c["start2"], c["end2"] = 0.5, 1.5, -0.5, 0.5
    _emission_ramp(p)
    return p


def _c1_emission(pkg):
    p = pkg.params_for_config("C1")
    _emission_ramp(p)
    return p


def _rust(pkg):
    # the medium of test_gpu_parity.test_sandstone_and_rust_noises: three different colour and emission components, per-path
    # realizations, the persistent march
    p = pkg.params_for_config("C3")
    p["impulse_density"] = 12
    p["multi_resolution_grid"] = 1
    p["isotropic_3d_sampling"] = 1
    p["correlation_context"] = pkg.CTX.RENEWAL
    p["ls_ramp_type"] = 5
    for key, lo, hi in (("var", 0.5, 1.6), ("mean_color", 0.0, 0.0), ("mean_emission", 0.0, 0.0)):
        p[key]["enabled"], p[key]["type"] = 1, 5
        p[key]["min"], p[key]["max"] = lo, hi
    return p


# name -> (params, albedo, guide)
CASES = {
    "grey": lambda pkg: (_grey(pkg), (0.8, 0.8, 0.8), True),
    "sigma": lambda pkg: (_sigma(pkg), ALBEDO, True),
    "ramp": lambda pkg: (_ramp_case(pkg), ALBEDO, False),
    "c1-emission": lambda pkg: (_c1_emission(pkg), ALBEDO, True),
    "rust": lambda pkg: (_rust(pkg), ALBEDO, False),
}
PIN_CASES = ("grey", "sigma", "ramp")              # with emission switched off: every channel against oracle_render_scene_s_paths
EMISSIVE_CASES = ("ramp", "c1-emission", "rust")


def parts(ob, kind):
    """scenes of the calls that together cover the frame: two row ranges, the spp ranges {0}, {1, 2}, or 3 shards of 4-pixel
    tile rows (5 tile rows: the shards get 2, 2 and 1)"""
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
        for k in range(3):
            s = frame(ob)
            s["tile_size"], s["shard_index"], s["shard_count"] = 4, k, 3
            out.append(s)
    return out


_memo = {}


def reference(pkg, ob, name, max_bounces, emission=True, threads=16):
    """the composite of case `name` on the whole frame (computed once per process, never modified by its users); emission=False:
    the same medium with mean_emission switched off"""
    key = (name, int(max_bounces), bool(emission))
    if key not in _memo:
        params, albedo, _ = CASES[name](pkg)
        if not emission:
            params = without_emission(params)
        orc = ob.Oracle(params, threads=threads)
        c = PathsRgbRef(pkg, ob).compose(orc, frame(ob), max_bounces, albedo)
        c.image.setflags(write=False)
        c.seg_count.setflags(write=False)
        _memo[key] = c
    return _memo[key]
