"""TEST INFRASTRUCTURE: the reference image of scene S through the weight-space GP medium, composed on the CPU from pieces that
exist on their own: the oracle's primary-ray generator (oracle_scene_s_primary), the plain-C restatement of the medium
(tests/native/ws_oracle.c: sampleDistance, transmittance) and a plain-C shade step and pixel sum (tests/native/ws_scene_shade.c,
compiled like ws_oracle.c with the restatement flags).  The composite always rebuilds the shadow segment's realization."""
import ctypes
import os
import subprocess

import numpy as np

import ws_oracle

ROOT = ws_oracle.ROOT
SRC = os.path.join(ROOT, "tests", "native", "ws_scene_shade.c")
LIB = os.path.join(ws_oracle.OUT_DIR, "libws_scene_shade.so")


def available():
    return ws_oracle.available()


def build():
    deps = [SRC, os.path.join(ROOT, "include", "gpis.h"), os.path.join(ROOT, "oracle", "Makefile")]
    if os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    cc = ws_oracle._compiler()
    if cc is None:
        raise RuntimeError("no C compiler for the scene-S shade step")
    os.makedirs(ws_oracle.OUT_DIR, exist_ok=True)
    tmp = LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([cc] + ws_oracle._flags() + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB)
    return LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def scene_pixels(scene):
    """(x, y) of the pixels one driver call covers, in the driver's order: the rows [y_begin, y_begin + y_count), of which with
    shard_count > 1 only the tile rows t (counted from y_begin) with t % shard_count == shard_index."""
    w, y0, yc = int(scene["width"]), int(scene["y_begin"]), int(scene["y_count"])
    sc, si, ts = int(scene["shard_count"]), int(scene["shard_index"]), int(scene["tile_size"])
    out = []
    for y in range(y0, y0 + yc):
        if sc > 1 and ((y - y0) // ts) % sc != si:
            continue
        out.extend((x, y) for x in range(w))
    return out


class Composite:
    """Result of compose(): image / hits (the accumulated buffers), n_eval (the reference's evaluations), n_seg (primary plus
    shadow segments marched) and the per-sample classes the tests assert on."""

    def __init__(self):
        self.image = self.hits = None
        self.n_eval = self.n_seg = 0
        self.n_samples = self.n_miss = self.n_exit = self.n_hit = self.n_lit = self.n_visible = self.n_occluded = 0
        self.hit_gp_ids = set()


class SceneRef:
    def __init__(self, pkg, ob, wso=None):
        self.pkg, self.ob = pkg, ob
        self.wso = wso or ws_oracle.WsOracle()
        ob.build()
        self.orc = ctypes.CDLL(ob.ORACLE_SO)
        self.orc.oracle_scene_s_primary.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        self.lib = ctypes.CDLL(build())
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.lib.ws_scene_shade.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        self.lib.ws_scene_shade.restype = None
        self.lib.ws_scene_sum.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
        self.lib.ws_scene_sum.restype = None

    def primary_rays(self, scene):
        """The valid primary rays of the call `scene` selects, in (pixel, sample) order: rays, u_shadow, pixel index, and the
        number of samples that miss the bounding sphere."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        w, s0, sn = int(scene["width"]), int(scene["spp_begin"]), int(scene["spp_count"])
        rays, us, pix = [], [], []
        miss = 0
        ray = np.zeros((), dtype=pkg.RAY_IN)
        u = ctypes.c_float()
        for x, y in scene_pixels(scene):
            for k in range(s0, s0 + sn):
                if self.orc.oracle_scene_s_primary(_p(scene), x, y, k, _p(ray), ctypes.byref(u)):
                    rays.append(ray.copy())
                    us.append(u.value)
                    pix.append(y * w + x)
                else:
                    miss += 1
        return (np.array(rays, dtype=pkg.RAY_IN).reshape(-1), np.array(us, dtype=np.float32), np.array(pix, dtype=np.uint32), miss)

    def shade(self, scene, rays, seg, us):
        n = len(rays)
        shadow = np.zeros(n, dtype=self.pkg.RAY_IN)
        cosl = np.zeros(n, dtype=np.float32)
        hit, lit = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self.lib.ws_scene_shade(_p(scene), n, _p(rays), _p(seg), _p(us), _p(shadow), _p(cosl), _p(hit), _p(lit))
        return shadow, cosl, hit, lit

    def compose(self, params, ws, scene, into=None):
        """One driver call on the CPU.  `into`: a Composite of earlier calls to accumulate into (image, hits and counts)."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        h, w = int(scene["height"]), int(scene["width"])
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w), dtype=np.float32)
            c.hits = np.zeros((h, w), dtype=np.uint32)
        rays, us, pix, miss = self.primary_rays(scene)
        seg, e1 = self.wso.sample_distance(params, ws, rays)
        shadow, cosl, hit, lit = self.shade(scene, rays, seg, us)
        idx = np.nonzero(lit)[0]
        vis = np.zeros(len(rays), dtype=np.uint8)
        e2 = 0
        if len(idx):
            v, e2 = self.wso.transmittance(params, ws, shadow[idx])
            vis[idx] = v
        self.lib.ws_scene_sum(_p(scene), len(rays), _p(pix), _p(cosl), _p(hit), _p(lit), _p(vis), _p(c.image), _p(c.hits))
        c.n_eval += e1 + e2
        c.n_seg += len(rays) + len(idx)
        c.n_samples += len(rays) + miss
        c.n_miss += miss
        c.n_exit += int((seg["exited"] != 0).sum())
        c.n_hit += int(hit.sum())
        c.n_lit += len(idx)
        c.n_visible += int(vis[idx].sum())
        c.n_occluded += len(idx) - int(vis[idx].sum())
        c.hit_gp_ids |= set(int(g) for g in seg["gp_id"][hit != 0])
        return c


# ---- the frame the tests, the fixture and the bench share ---------------------------------------------------------------------
def small_scene(ob, width=24, height=16, spp=4, spp_begin=0, fov=60.0):
    """Default scene S with a wider field of view: at 35 degrees the bounding sphere (radius 1.5 seen from z = 4, 22 degrees half
    angle) fills the frame and no sample misses it."""
    s = ob.default_scene_s(width, height, spp)
    s["spp_begin"] = spp_begin
    s["cam_fov_deg"] = fov
    return s
