"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_nee_paths, the multi-bounce conductor NEE / MIS estimator on scene S
through the sparse-convolution medium, composed on the CPU bounce level by bounce level — one call per bounce over all live
samples — from the oracle's batch entries (oracle_scene_s_primary, oracle_sample_distance_batch with its coefficients,
oracle_nee_pdf_batch, oracle_nee_grad_batch, oracle_transmittance_batch) and a plain-C restatement in float of the set-up, shade
and bounce step (tests/native/nee_paths_shade.c, compiled with the flags of oracle/Makefile).

tests/test_nee_paths_cpu.py ties the C file to the oracle: a composite of max_path_bounces = 2 must equal
oracle_render_scene_s_nee bit for bit."""
import ctypes
import os
import subprocess

import numpy as np

import ws_oracle
from ws_scene_ref import scene_pixels

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "nee_paths_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libnee_paths_shade.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "nee_paths_small.npz")

# numpy mirror of nee_paths_shade.c's nee_paths_hit
HIT = np.dtype([
    ("d", "<f4", 3), ("w", "<f4", 3), ("F", "<f4"), ("thr", "<f4"), ("scheme", "<i4"),
    ("hit", "u1"), ("want_light", "u1"), ("want_phase", "u1"), ("want_pdf_normal", "u1"),
    ("pdf_half", "<f4"), ("grad_half", "<f4", 3), ("pdf_normal", "<f4"),
    ("go_light", "u1"), ("go_phase", "u1"), ("vis_light", "u1"), ("vis_phase", "u1"),
    ("contrib_light", "<f4"), ("contrib_phase", "<f4"),
], align=True)


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the NEE path shade step")
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
    lib.nee_paths_hit_size.restype = sz
    assert lib.nee_paths_hit_size() == HIT.itemsize
    lib.nee_paths_stream.argtypes = [vp, u32, u32, u32]
    lib.nee_paths_stream.restype = ctypes.c_uint64
    lib.nee_paths_setup.argtypes = [vp, vp, sz] + [vp] * 10
    lib.nee_paths_setup.restype = None
    lib.nee_paths_shade.argtypes = [vp, vp, sz, i32, i32] + [vp] * 9
    lib.nee_paths_shade.restype = None
    lib.nee_paths_gather.argtypes = [vp, sz, vp, vp]
    lib.nee_paths_gather.restype = None
    lib.nee_paths_sum.argtypes = [sz, vp, vp, vp, vp, vp]
    lib.nee_paths_sum.restype = None
    for name, n_args in (("conductor_reflectance", 3), ("power_heuristic", 2), ("spherical_cap_pdf", 1)):
        fn = getattr(lib, "nee_paths_" + name)
        fn.argtypes, fn.restype = [f32] * n_args, f32
    for name in ("tangent_frame", "frame_to_local", "frame_to_global"):
        getattr(lib, "nee_paths_" + name).restype = None
    return lib


class Composite:
    """Result of compose(): image and seg_count (the accumulated buffers), n_seg (= seg_count.sum()), and per bounce the segments
    marched (`marched`), the hits (`hits`) and the light / phase shadow segments marched."""

    def __init__(self):
        self.image = self.seg_count = None
        self.n_samples = self.n_miss = 0
        self.marched, self.hits, self.light, self.phase = [], [], [], []

    @property
    def n_seg(self):
        return int(self.seg_count.sum())

    def _count(self, lst, bounce, k):
        while len(lst) <= bounce:
            lst.append(0)
        lst[bounce] += int(k)


class NeePathsRef:
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
                rng[i] = self.lib.nee_paths_stream(_p(scene), x, y, k)
                pix[i] = y * w + x
                i += 1
        return rays, rng, alive, pix

    def compose(self, orc, scene, surface, max_bounces, into=None):
        """One driver call on the CPU through the oracle `orc`.  `into`: a Composite of earlier calls to accumulate into."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        surface = np.array(surface, dtype=pkg.SURFACE_S).reshape(())
        assert int(max_bounces) >= 1 and -1.0 < float(surface["cap_cos"]) < 1.0
        h, w = int(scene["height"]), int(scene["width"])
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w), dtype=np.float32)
            c.seg_count = np.zeros((h, w), dtype=np.uint32)
        rays, rng, alive, pix = self.begin(orc, scene)
        n = len(rays)
        c.n_samples += n
        c.n_miss += int(n - alive.sum())
        thr = np.ones(n, dtype=np.float32)
        emission = np.zeros(n, dtype=np.float32)
        segs = np.zeros(n, dtype=np.uint32)
        seg = np.zeros(n, dtype=pkg.SEG_OUT)
        coeff = np.zeros(n, dtype=pkg.COND_COEFF)
        hits = np.zeros(n, dtype=HIT)
        q_half, q_normal = np.zeros(n, dtype=pkg.NEE_QUERY), np.zeros(n, dtype=pkg.NEE_QUERY)
        sh_light, sh_phase = np.zeros(n, dtype=pkg.RAY_IN), np.zeros(n, dtype=pkg.RAY_IN)
        for bounce in range(int(max_bounces) - 1):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            assert (rays["segment"][idx] == bounce).all() and (rays["first_scatter"][idx] == (1 if bounce == 0 else 0)).all()
            seg[idx], coeff[idx] = orc.sample_distance(rays[idx], want_coeff=True)
            c._count(c.marched, bounce, len(idx))
            self.lib.nee_paths_setup(_p(scene), _p(surface), n, _p(alive), _p(rays), _p(seg), _p(coeff), _p(rng), _p(thr), _p(segs), _p(hits),
                                     _p(q_half), _p(q_normal))
            c._count(c.hits, bounce, hits["hit"].sum())
            k = np.nonzero(hits["want_light"])[0]
            if len(k):
                hits["pdf_half"][k] = orc.nee_pdf(q_half[k])
                hits["grad_half"][k] = orc.nee_grad(q_half[k])
            k = np.nonzero(hits["want_pdf_normal"])[0]
            if len(k):
                hits["pdf_normal"][k] = orc.nee_pdf(q_normal[k])
            self.lib.nee_paths_shade(_p(scene), _p(surface), n, bounce, int(max_bounces), _p(alive), _p(rays), _p(seg), _p(rng), _p(thr), _p(segs),
                                     _p(hits), _p(sh_light), _p(sh_phase))
            for go, vis, sh, lst in (("go_light", "vis_light", sh_light, c.light), ("go_phase", "vis_phase", sh_phase, c.phase)):
                k = np.nonzero(hits[go])[0]
                c._count(lst, bounce, len(k))
                if len(k):
                    assert (sh["segment"][k] == bounce + 1).all() and (sh["first_scatter"][k] == 0).all()
                    hits[vis][k] = orc.transmittance(sh[k])
            self.lib.nee_paths_gather(_p(surface), n, _p(hits), _p(emission))
        self.lib.nee_paths_sum(n, _p(pix), _p(emission), _p(segs), _p(c.image), _p(c.seg_count))
        return c


# ---- the frame and the media the tests and the fixture share --------------------------------------------------------------------
W, H, SPP = 24, 20, 3              # 1440 samples: a multiple of neither 64 nor 256
BOUNCES = (1, 3, 4, 6)
SCHEMES = {"uni": 0, "nee": 1, "mis": 2}


def frame(ob):
    return ob.default_scene_s(W, H, SPP)


def _c2(pkg, scheme, **kw):
    p = pkg.params_for_config("C2")
    p["scheme_1d"] = SCHEMES[scheme]
    for k, v in kw.items():
        p[k] = v
    return p


def _colour(pkg):
    # a mean-colour ramp and absorption: weight[0] != 1, so the throughput of a path is not the product of the F alone
    p = _c2(pkg, "mis")
    p["sigma_a"] = (0.25, 0.5, 1.0)
    c = p["mean_color"]
    c["enabled"], c["type"] = 1, 1
    c["min"], c["max"], c["start"], c["end"] = 0.2, 0.9, -1.0, 1.0
    c["min2"], c["max2"], c["start2"], c["end2"] = 0.5, 1.5, -0.5, 0.5
    return p


def _surface(pkg, **kw):
    s = pkg.default_surface_s()
    for k, v in kw.items():
        s[k] = v
    return s


# name -> (params, surface, guide): the schemes (UNI with the wide cap of test_render_scene_s_nee), the contexts Renewal+ (C2's own)
# and Renewal, gradient correlation off, weight[0] != 1, a single-realization medium (the scheme degenerates to UNI; on the device it
# runs on the guided kernels, as in test_drivers_on_other_media), and a darker conductor (the default surface has eta, k != 0 and
# albedo 1; a perfect mirror, eta = k = 0, is the "mirror" case).
CASES = {
    "uni": lambda pkg: (_c2(pkg, "uni"), _surface(pkg, cap_cos=0.9), False),
    "nee": lambda pkg: (_c2(pkg, "nee"), _surface(pkg), False),
    "mis": lambda pkg: (_c2(pkg, "mis"), _surface(pkg), False),
    "mis-renewal": lambda pkg: (_c2(pkg, "mis", correlation_context=pkg.CTX.RENEWAL), _surface(pkg), False),
    "mis-no_xy": lambda pkg: (_c2(pkg, "mis", correlation_xy=0), _surface(pkg), False),
    "nee-renewal-no_xy": lambda pkg: (_c2(pkg, "nee", correlation_context=pkg.CTX.RENEWAL, correlation_xy=0), _surface(pkg), False),
    "mis-colour": lambda pkg: (_colour(pkg), _surface(pkg), False),
    "single": lambda pkg: (pkg.params_for_config("C1"), _surface(pkg, cap_cos=0.5), True),
    "mis-dark": lambda pkg: (_c2(pkg, "mis"), _surface(pkg, eta=1.5, k=2.5, albedo=0.7), False),
    "mis-mirror": lambda pkg: (_c2(pkg, "mis"), _surface(pkg, eta=0.0, k=0.0, albedo=0.9), False),
}
PIN_CASES = ("uni", "nee", "mis")          # max_path_bounces = 2 against oracle_render_scene_s_nee / gpis_render_scene_s_nee
GOLDEN_BOUNCES = 4


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


def reference(pkg, ob, name, max_bounces, threads=16):
    """the composite of case `name` on the whole frame (computed once per process, never modified by its users)"""
    key = (name, int(max_bounces))
    if key not in _memo:
        params, surf, _ = CASES[name](pkg)
        orc = ob.Oracle(params, threads=threads)
        c = NeePathsRef(pkg, ob).compose(orc, frame(ob), surf, max_bounces)
        c.image.setflags(write=False)
        c.seg_count.setflags(write=False)
        _memo[key] = c
    return _memo[key]
