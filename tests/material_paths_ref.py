"""TEST INFRASTRUCTURE: the reference of gpis_render_scene_s_material_paths_rgb, the RGB path estimator on scene S whose material is
chosen per hit by the GP id, composed on the CPU bounce level by bounce level from the oracle's batch entries and a plain-C
restatement in float of the set-up, shade, bounce and gather step for both materials (tests/native/material_paths_shade.c, compiled
with the flags of oracle/Makefile).  The loop is tests/nee_paths_rgb_ref.py's; a Lambert hit asks for no neePDF / neeGrad query.

The conductor step is nee_paths_rgb_shade.c's own (tests/test_material_paths_cpu.py pins the composite of an all-equal-conductor
table to nee_paths_rgb_ref's, bit for bit).  The Lambert step is restated from TraceBase.cpp / LambertBsdf.cpp; its parity with the
reference is UNPINNED above its pieces: the disk sampler (pinned to tests/native/paths_rgb_shade.c's) and the MIS estimator (pinned
to its closed form)."""
import ctypes
import os
import subprocess

import numpy as np

import nee_paths_ref as npr
import nee_paths_rgb_ref as rgb
import ws_oracle

ROOT = ws_oracle.ROOT
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "material_paths_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libmaterial_paths_shade.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "material_paths_small.npz")

# numpy mirror of material_paths_shade.c's mat_paths_hit
HIT = np.dtype([("h", rgb.HIT), ("type", "<i4"), ("material", "<u4"), ("wi_z", "<f4"), ("wo_z", "<f4"), ("wop_z", "<f4")], align=True)


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(NATIVE, "nee_paths_rgb_shade.c"), os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the material path shade step")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-I", NATIVE, "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


_p = rgb._p


def shade_lib():
    lib = ctypes.CDLL(build())
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    lib.mat_paths_hit_size.restype = sz
    assert lib.mat_paths_hit_size() == HIT.itemsize
    lib.nee_paths_rgb_stream.argtypes = [vp, u32, u32, u32]
    lib.nee_paths_rgb_stream.restype = ctypes.c_uint64
    lib.nee_paths_rgb_points.argtypes = [sz] + [vp] * 5
    lib.nee_paths_rgb_points.restype = None
    lib.mat_paths_setup.argtypes = [vp, vp, sz, i32, i32, i32] + [vp] * 12
    lib.mat_paths_setup.restype = None
    lib.mat_paths_shade.argtypes = [vp, vp, sz, i32, i32] + [vp] * 9
    lib.mat_paths_shade.restype = None
    lib.mat_paths_gather.argtypes = [vp, sz, vp, vp]
    lib.mat_paths_gather.restype = None
    lib.nee_paths_rgb_sum.argtypes = [sz, vp, vp, vp, vp, vp]
    lib.nee_paths_rgb_sum.restype = None
    lib.mat_paths_lambert_direction.argtypes = [vp, vp, vp]
    lib.mat_paths_lambert_direction.restype = None
    return lib


class Composite(rgb.Composite):
    """nee_paths_rgb_ref.Composite, and per bounce the hits of each GP id (`ids`: a list of [n_id0, n_id1, ...]) and of each
    material type (`types`: [conductor, Lambert])"""

    def __init__(self):
        super().__init__()
        self.ids, self.types = [], []


class MaterialPathsRef:
    def __init__(self, pkg, ob):
        self.pkg, self.ob = pkg, ob
        self.lib = shade_lib()
        self._begin = rgb.NeePathsRgbRef(pkg, ob).begin          # the camera step is the RGB conductor driver's

    def lambert_direction(self, state, normal):
        """the Lambert disk sampler around `normal` from the PCG32 state: (world direction, state after)"""
        st = np.array([state], dtype=np.uint64)
        n, w = np.array(normal, dtype=np.float32), np.zeros(3, dtype=np.float32)
        self.lib.mat_paths_lambert_direction(_p(st), _p(n), _p(w))
        return w, int(st[0])

    def compose(self, orc, scene, mats, max_bounces, into=None):
        """One driver call on the CPU through the oracle `orc`.  `into`: a Composite of earlier calls to accumulate into."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        mats = np.array(mats, dtype=pkg.MATERIALS_S).reshape(())
        max_bounces = int(max_bounces)
        assert max_bounces >= 1 and -1.0 < float(mats["cap_cos"]) < 1.0 and 1 <= int(mats["n_materials"]) <= pkg.MAX_MATERIALS
        h, w = int(scene["height"]), int(scene["width"])
        E = rgb.emissive(orc.params)
        n_marched = max_bounces if E else max_bounces - 1
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w, 3), dtype=np.float32)
            c.seg_count = np.zeros((h, w), dtype=np.uint32)
        rays, rng, alive, pix = self._begin(orc, scene)
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
            self.lib.mat_paths_setup(_p(scene), _p(mats), n, bounce, max_bounces, 1 if E else 0, _p(alive), _p(rays), _p(seg), _p(coeff), _p(e),
                                     _p(rng), _p(thr), _p(em), _p(segs), _p(hits), _p(q_half), _p(q_normal))
            H = hits["h"]
            hit = H["hit"] != 0
            c._count(c.hits, bounce, hit.sum())
            while len(c.ids) <= bounce:
                c.ids.append([0] * pkg.MAX_MATERIALS)
                c.types.append([0, 0])
            for g in range(pkg.MAX_MATERIALS):
                c.ids[bounce][g] += int((hit & (seg["gp_id"] == g)).sum())
            for t in range(2):
                c.types[bounce][t] += int((hit & (hits["type"] == t)).sum())
            assert int((hit & ((seg["gp_id"] < 0) | (seg["gp_id"] >= pkg.MAX_MATERIALS))).sum()) == 0
            if bounce + 1 >= max_bounces:
                assert not hit.any() and not alive.any()
                break
            assert not (H["want_light"] | H["want_phase"] | H["want_pdf_normal"])[hits["type"] == pkg.MATERIAL.LAMBERT].any()
            k = np.nonzero(H["want_light"])[0]
            if len(k):
                H["pdf_half"][k] = orc.nee_pdf(q_half[k])
                H["grad_half"][k] = orc.nee_grad(q_half[k])
            k = np.nonzero(H["want_pdf_normal"])[0]
            if len(k):
                H["pdf_normal"][k] = orc.nee_pdf(q_normal[k])
            self.lib.mat_paths_shade(_p(scene), _p(mats), n, bounce, n_marched, _p(alive), _p(rays), _p(seg), _p(rng), _p(thr), _p(segs),
                                     _p(hits), _p(sh_light), _p(sh_phase))
            for go, vis, sh, lst in (("go_light", "vis_light", sh_light, c.light), ("go_phase", "vis_phase", sh_phase, c.phase)):
                k = np.nonzero(H[go])[0]
                c._count(lst, bounce, len(k))
                if len(k):
                    assert (sh["segment"][k] == bounce + 1).all() and (sh["first_scatter"][k] == 0).all()
                    H[vis][k] = orc.transmittance(sh[k])
            c._count(c.light_visible, bounce, (H["go_light"] & H["vis_light"]).sum())
            self.lib.mat_paths_gather(_p(mats), n, _p(hits), _p(em))
        self.lib.nee_paths_rgb_sum(n, _p(pix), _p(em), _p(segs), _p(c.image), _p(c.seg_count))
        c.sample_em, c.pix = em, pix
        return c


# ---- the frame, the media and the tables the tests and the fixture share --------------------------------------------------------
W, H, SPP = npr.W, npr.H, npr.SPP          # 24 x 20 x 3: 1440 samples, six workgroups, a multiple of neither 64 nor 256
BOUNCES = (1, 3, 4)
GOLDEN_BOUNCES = 4


def frame(ob):
    return ob.default_scene_s(W, H, SPP)


def csg(pkg, params):
    """the medium made CSG: the minimum of its mean and a sphere of radius 0.6 at (0.55, 0.35, 0.6); hits on the sphere have id 1.
    Changes `params` in place: a copy of a record does not carry its padding bytes, which the fixture compares."""
    p = params
    p["has_mean_additional"] = 1
    a = p["mean_additional"]
    a["type"], a["center"], a["radius"] = pkg.MEAN_TYPE.SPHERICAL, (0.55, 0.35, 0.6), 0.6
    return p


def conductor(pkg, eta=None, k=None, albedo=(1.0, 1.0, 1.0)):
    cu = pkg.default_surface_rgb()
    m = np.zeros((), dtype=pkg.MATERIAL_RGB)
    m["type"], m["eta"], m["k"], m["albedo"] = pkg.MATERIAL.CONDUCTOR, cu["eta"] if eta is None else eta, cu["k"] if k is None else k, albedo
    return m


def lambert(pkg, albedo=(0.8, 0.6, 0.4)):
    m = np.zeros((), dtype=pkg.MATERIAL_RGB)
    m["type"], m["albedo"] = pkg.MATERIAL.LAMBERT, albedo
    return m


def table(pkg, materials, cap_cos=None, cap_radiance=(20.0, 15.0, 10.0)):
    """a table of the given materials under nee_paths_rgb_ref.copper's light: bright enough that float rounding differs per channel"""
    t = np.zeros((), dtype=pkg.MATERIALS_S)
    t["n_materials"] = len(materials)
    t["cap_cos"] = pkg.default_surface_rgb()["cap_cos"] if cap_cos is None else cap_cos
    t["cap_radiance"] = cap_radiance
    for i, m in enumerate(materials):
        t["material"][i] = m
    return t


def table_of_surface(pkg, surface, n=2):
    """the table whose n entries all are the conductor of an RGB surface, under its light"""
    surface = np.array(surface, dtype=pkg.SURFACE_RGB_S).reshape(())
    return table(pkg, [conductor(pkg, surface["eta"], surface["k"], surface["albedo"])] * n, cap_cos=surface["cap_cos"], cap_radiance=surface["cap_radiance"])


def _tables(pkg, which, **kw):
    cu, la, la2 = conductor(pkg), lambert(pkg), lambert(pkg, albedo=(0.3, 0.5, 0.9))
    return table(pkg, {"cu-la": [cu, la], "la-cu": [la, cu], "la-la": [la, la2]}[which], **kw)


def _separate(pkg):
    # surf_vol_phase_separate: the id is the side of surf_vol_phase_amp_thresh the UNSCALED variance lies on (SCN.cpp:80-86), which is 1
    # everywhere unless the covariance is of the grid flavour (GPF.hpp:1185, GPF.cpp:1386-1391): a `var` ramp alone gives one id.
    # Hence the grid flavour, whose variance comes from a voxel grid (set on the medium and on the oracle: see grid()).
    import test_grid_oracle_cpu as G
    p = G._params(pkg, 1)
    p["multi_resolution_grid"], p["isotropic_3d_sampling"] = 1, 1
    p["correlation_context"] = pkg.CTX.RENEWAL
    p["surf_vol_phase_separate"], p["surf_vol_phase_amp_thresh"] = 1, SEPARATE_THRESHOLD
    return p


SEPARATE_THRESHOLD = 1.2          # both sides are hit on the test frame (694 / 461 first-bounce hits; 1.4 leaves 19 on one side)


def grid():
    """the variance grid of the `separate` case: (voxels, world_to_index, interpolate), for set_variance_grid of a Medium or an Oracle"""
    import test_grid_oracle_cpu as G
    return G._grid(24, seed=9), G._world_to_index(24), "linear"


# name -> (params, table, guide): the media of the GPU test.  C2 made CSG under the three schemes (UNI with the wide cap of
# nee_paths_ref) and the three tables, C1 (single realization: on the device the guided kernels) made CSG, the colour medium with
# its emission made CSG, and surf_vol_phase_separate.
CASES = {
    "mis/cu-la": lambda pkg: (csg(pkg, npr._c2(pkg, "mis")), _tables(pkg, "cu-la"), False),
    "mis/la-cu": lambda pkg: (csg(pkg, npr._c2(pkg, "mis")), _tables(pkg, "la-cu"), False),
    "mis/la-la": lambda pkg: (csg(pkg, npr._c2(pkg, "mis")), _tables(pkg, "la-la"), False),
    "nee/cu-la": lambda pkg: (csg(pkg, npr._c2(pkg, "nee")), _tables(pkg, "cu-la"), False),
    "uni/cu-la": lambda pkg: (csg(pkg, npr._c2(pkg, "uni")), _tables(pkg, "cu-la", cap_cos=0.9), False),
    "single/cu-la": lambda pkg: (csg(pkg, pkg.params_for_config("C1")), _tables(pkg, "cu-la", cap_cos=0.5), True),
    "colour-emission/cu-la": lambda pkg: (csg(pkg, rgb._emissive(pkg)), _tables(pkg, "cu-la"), False),
    "separate/cu-la": lambda pkg: (_separate(pkg), _tables(pkg, "cu-la", cap_cos=0.9), False),
}
EMISSIVE_CASE = "colour-emission/cu-la"
GRID_CASES = ("separate/cu-la",)
# the media of nee_paths_rgb_ref / nee_paths_ref WITHOUT a second mean: every id is 0
PLAIN_CASES = {
    "mis": lambda pkg: (npr._c2(pkg, "mis"), rgb.copper(pkg)),
    "nee": lambda pkg: (npr._c2(pkg, "nee"), rgb.copper(pkg)),
    "uni": lambda pkg: (npr._c2(pkg, "uni"), rgb.copper(pkg, cap_cos=0.9)),
    "mis-colour": lambda pkg: (npr._colour(pkg), rgb.copper(pkg)),
}


def medium(pkg, name):
    """the device medium of a case (guided where the case says so, with its variance grid)"""
    params, _, guide = CASES[name](pkg)
    m = pkg.Medium(params)
    if name in GRID_CASES:
        m.set_variance_grid(*grid())
    if guide:
        m.build_guide(16, 8)
    return m


def oracle(pkg, ob, name, threads=16):
    orc = ob.Oracle(CASES[name](pkg)[0], threads=threads)
    if name in GRID_CASES:
        orc.set_variance_grid(*grid())
    return orc


def parts(ob, kind):
    return npr.parts(ob, kind)          # two row ranges, the spp ranges {0}, {1, 2}, 3 shards of 4-pixel tile rows


_memo = {}


def reference(pkg, ob, name, max_bounces, mats=None, threads=16):
    """the composite of case `name` on the whole frame (computed once per process, never modified by its users); `mats`: another
    table than the case's own"""
    own = CASES[name](pkg)[1]
    mats = np.array(own if mats is None else mats, dtype=pkg.MATERIALS_S).reshape(())
    key = (name, int(max_bounces), mats.tobytes())
    if key not in _memo:
        c = MaterialPathsRef(pkg, ob).compose(oracle(pkg, ob, name, threads), frame(ob), mats, max_bounces)
        c.image.setflags(write=False)
        c.seg_count.setflags(write=False)
        _memo[key] = c
    return _memo[key]
