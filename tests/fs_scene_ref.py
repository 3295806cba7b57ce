"""TEST INFRASTRUCTURE: the reference image of scene S through the function-space GP medium, composed on the CPU from pieces
that exist on their own: the oracle's primary-ray generator (oracle_scene_s_primary), the CPU restatement of the medium
(Oracle.fs_sample_distance / fs_transmittance), and the plain-C shade step and pixel sum of the weight-space composite
(tests/ws_scene_ref.py, tests/native/ws_scene_shade.c).

What is this medium's own is the sampler: the path's one PCG32 stream gives jx, jy and then every variate of the medium.  The
primary segment's gpis_fs_state.sampler_state is therefore the stream's state after those two draws, computed here in Python
(sampler_state_after_jitter); the shadow segment continues from the state the primary segment returned, context and sampler."""
import struct

import numpy as np

import ws_scene_ref

PCG_MULT = 6364136223846793005
MASK64 = (1 << 64) - 1


def available():
    return ws_scene_ref.available()


def lcg(state, steps=1):
    """the PCG32 state transition state * 6364136223846793005 + 1 (mod 2^64), `steps` times"""
    for _ in range(steps):
        state = (state * PCG_MULT + 1) & MASK64
    return state


def sampler_state_after_jitter(seed32):
    """State of the path's sampler when the medium takes over: set_state(seed) assigns the seed and discards two draws, then
    jx and jy are drawn: 2 + 2 transitions."""
    return lcg(int(seed32) & 0xFFFFFFFF, 2 + 2)


def pcg_draw(state):
    """(next_1d as float32, next state): the output permutation of PCG32 on the OLD state, normalised as normalized_uint does"""
    xs = ((((state >> 18) ^ state) >> 27)) & 0xFFFFFFFF
    rot = state >> 59
    i = ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF
    f = struct.unpack("<f", struct.pack("<I", (i >> 9) | 0x3F800000))[0]
    return np.float32(f) - np.float32(1.0), lcg(state)


class Composite(ws_scene_ref.Composite):
    """ws_scene_ref.Composite plus n_notok (primary segments that ended !ok: neither hit nor lit) and, of the LAST compose()
    call, the per-sample arrays (`last`: rays, states, seg, states_after, shadow, cosl, hit, lit, vis, pix)."""

    def __init__(self):
        super().__init__()
        self.n_notok = 0
        self.last = None


class FsSceneRef:
    def __init__(self, pkg, ob, threads=8):
        self.pkg, self.ob, self.threads = pkg, ob, threads
        self.base = ws_scene_ref.SceneRef(pkg, ob, wso=object())        # primary rays, shade step, pixel sum; no weight-space oracle
        self._oracles = {}

    def oracle(self, params):
        key = np.array(params, dtype=self.pkg.PARAMS).tobytes()
        if key not in self._oracles:
            self._oracles[key] = self.ob.Oracle(params, threads=self.threads)
        return self._oracles[key]

    def primary_states(self, scene, rays):
        """the empty states of the primary segments: only the sampler is set"""
        scene = np.array(scene, dtype=self.pkg.SCENE_S).reshape(())
        st = np.zeros(len(rays), dtype=self.pkg.FS_STATE)
        if len(rays):
            words = np.stack([rays["pixel"][:, 0], rays["pixel"][:, 1], rays["spp"],
                              np.full(len(rays), int(scene["scene_seed"]), dtype=np.uint32)], axis=1).astype(np.uint32)
            seeds = self.ob.xxhash32(words)
            state = (seeds.astype(np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
            for _ in range(2 + 2):                                       # sampler_state_after_jitter, on the whole array (uint64 wraps)
                state = state * np.uint64(PCG_MULT) + np.uint64(1)
            st["sampler_state"] = state
            assert int(state[0]) == sampler_state_after_jitter(int(seeds[0]) + 1)
        return st

    def compose(self, params, scene, into=None):
        """One driver call on the CPU.  `into`: a Composite of earlier calls to accumulate into (image, hits and counts)."""
        pkg = self.pkg
        scene = np.array(scene, dtype=pkg.SCENE_S).reshape(())
        h, w = int(scene["height"]), int(scene["width"])
        c = into or Composite()
        if c.image is None:
            c.image = np.zeros((h, w), dtype=np.float32)
            c.hits = np.zeros((h, w), dtype=np.uint32)
        orc = self.oracle(params)
        rays, us, pix, miss = self.base.primary_rays(scene)
        st0 = self.primary_states(scene, rays)
        seg, st1 = orc.fs_sample_distance(rays, st0)
        shadow, cosl, hit, lit = self.base.shade(scene, rays, seg, us)
        idx = np.nonzero(lit)[0]
        vis = np.zeros(len(rays), dtype=np.uint8)
        if len(idx):
            v, _ = orc.fs_transmittance(shadow[idx], st1[idx])          # continues from the primary's state
            vis[idx] = v
        _p = ws_scene_ref._p
        self.base.lib.ws_scene_sum(_p(scene), len(rays), _p(pix), _p(cosl), _p(hit), _p(lit), _p(vis), _p(c.image), _p(c.hits))
        c.n_seg += len(rays) + len(idx)
        c.n_samples += len(rays) + miss
        c.n_miss += miss
        c.n_exit += int(((seg["exited"] != 0) & (seg["ok"] != 0)).sum())
        c.n_notok += int((seg["ok"] == 0).sum())
        c.n_hit += int(hit.sum())
        c.n_lit += len(idx)
        c.n_visible += int(vis[idx].sum())
        c.n_occluded += len(idx) - int(vis[idx].sum())
        c.last = dict(rays=rays, states=st0, seg=seg, states_after=st1, shadow=shadow, cosl=cosl, hit=hit, lit=lit, vis=vis, pix=pix, u_shadow=us)
        return c


# ---- the media and frames the tests and the bench share -------------------------------------------------------------------------
def fs_params(pkg, ctx, n, step, aniso=(1.0, 1.0, 1.0), mean="SPHERICAL", radius=1.0, offset=0.0):
    """C0 with a per-path realization, sigma 0.1, length scale 0.05 and the given function-space settings"""
    p = pkg.params_for_config("C0")
    p["single_realization"] = 0
    p["correlation_context"] = getattr(pkg.CTX, ctx)
    p["mean"]["type"] = getattr(pkg.MEAN_TYPE, mean)
    p["mean"]["radius"] = radius
    p["mean"]["offset"] = offset
    p["sigma"], p["length_scale"] = 0.1, 0.05
    p["aniso"] = aniso
    p["fs_sample_points"], p["fs_step_size"] = n, step
    return p


# context, fs_sample_points, fs_step_size, (width, height, spp): every frame holds a miss, an exit, a hit, a visible and an
# occluded shadow segment
CASES = {
    "renewal-16": ("RENEWAL", 16, 0.04, (24, 16, 4)),
    "none-12": ("NONE", 12, 0.0, (24, 16, 4)),
    "global-14": ("GLOBAL", 14, 0.05, (24, 16, 4)),
    "renewal_plus-32": ("RENEWAL_PLUS", 32, 0.02, (24, 16, 4)),
    "global-64": ("GLOBAL", 64, 0.01, (12, 8, 2)),
}


def case(pkg, ob, name):
    ctx, n, step, (w, h, spp) = CASES[name]
    return fs_params(pkg, ctx, n, step), ws_scene_ref.small_scene(ob, w, h, spp, fov=60.0)


def assert_non_vacuous(c):
    assert c.n_miss > 0 and c.n_exit > 0 and c.n_hit > 0 and c.n_visible > 0 and c.n_occluded > 0, \
        (c.n_miss, c.n_exit, c.n_hit, c.n_visible, c.n_occluded)


def assert_spp_cut_equals_whole(acc_image, part_images, whole_image):
    """What a frame cut into two spp ranges must satisfy.  Each call sums its samples from zero, in sample order, and adds that
    sum to the image once, so the accumulated image IS float32(first + second), bit for bit.  Against the whole frame the cut
    changes the association of a pixel's terms, (a0 + a1) + (a2 + a3) for ((a0 + a1) + a2) + a3, which float32 does not promise
    to preserve: where only one of the two ranges contributes to a pixel the association is the whole frame's and the bits must
    be equal; elsewhere both sums are the same non-negative terms with fl(a0 + a1) in common and two further roundings of
    2^-24 relative each, so they differ by at most 4 * 2^-24 of the sum (2^-21 allows for the second-order terms)."""
    first, second = part_images
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
    assert np.array_equal(bits(acc_image), bits(first + second))
    one_sided = (first == 0) | (second == 0)
    assert one_sided.any() and (~one_sided).any()
    assert np.array_equal(bits(acc_image)[one_sided], bits(whole_image)[one_sided])
    assert (np.abs(acc_image.astype(np.float64) - whole_image.astype(np.float64)) <= 2.0 ** -21 * whole_image.astype(np.float64)).all()
