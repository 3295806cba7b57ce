"""TEST INFRASTRUCTURE: the march of a medium with a procedural SDF mean, composed on the CPU from two frozen references.

The frozen oracle (oracle/) knows no procedural mean.  What it does know is the noise: on the SAME medium with a homogeneous mean of
offset 0 its evaluate_value returns (float)((double)(amplitude * noise) + 0.0) = amplitude * noise exactly, and its gradient
amplitude * grad(noise) + 0.  The mean comes from tests/sdf_mean_ref.py (the C restatement pinned to the reference's compiled SDF
functions).  So, in the device's own float arithmetic (csrc/gpis_path.inc: evaluate_value, evaluate_gradient, conditioning):

    value    = float(double(v0) + mean_ref)
    gradient = g0 + float(grad_ref)                       per component
    conditioning = the oracle's, with the targets pre-reduced: target_val - float(mean_ref), target_grad - float(grad_ref)

SdfComposite runs intersectGP (SparseConvolutionNoiseMedium.cpp:102-183) and the scattering branch of sampleDistance /
transmittance (GaussianProcessMedium.cpp:221-393) over batches of rays on top of those three, and fills every field of gpis_seg_out.
It offers sample_distance, transmittance, scene_s_primary, mean_color_emission and params, so it can stand in for the oracle in
tests/paths_rgb_ref.py's PathsRgbRef.compose, and nee_pdf / nee_grad, so it can in tests/nee_paths_ref.py's NeePathsRef.compose.

NEE.  neeShared (SCN.cpp:601-743) is not linear in the mean's gradient, so the noise-only decomposition does not carry over.  It reads
the mean's GRADIENT only, narrowed to float, and the oracle's LinearMean with dir = +-e_k has exactly the gradient +-scale * e_k (the
other components are positive zeros).  So for a query whose reference gradient, at double(float(p)) and from the slot the CSG id
selects, has at most one non-zero component in float, nee_pdf / nee_grad are the ORACLE's own on this medium with the mean replaced by
that linear one (the homogeneous mean 0 for a zero gradient): nothing of ours is restated.  A query with a general gradient (knob_inner,
two_spheres, most of the knob) has no such stand-in: nee_pdf / nee_grad raise on it, and callers select their queries first.

Scope of the march: media whose noise amplitude is a constant (stationary kernels, the Matern ones included; the multi-resolution
wrapper is served for the three evaluator formulas only), 3D or 1D sampling (the evaluation count n_evals is the 3D evaluators'),
one mean or a CSG pair, sigma_s != 0, surf_vol_phase_separate off.  Scope of NEE: axis-aligned mean gradients, as said above."""
import numpy as np

import sdf_mean_ref

f32 = np.float32


def noise_only(pkg, params):
    """the same medium with a homogeneous mean of offset 0 and no CSG partner: what the oracle is asked for the noise"""
    p = np.array(pkg.as_params(params))
    p["mean"]["type"] = pkg.MEAN_TYPE.HOMOGENEOUS
    p["mean"]["offset"] = 0.0
    p["mean"]["func"] = 0
    p["has_mean_additional"] = 0
    p["mean_additional"] = pkg.default_params()["mean_additional"]
    return p


def transform_demo():
    """a non-trivial "transform": rotation x non-uniform scale x translation (row-major Mat4f)"""
    c, s = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    tr = np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.03], [0, 0, 1, 0.02], [0, 0, 0, 1.0]])
    return (tr @ rot @ np.diag([1.1, 0.9, 1.2, 1.0])).astype(np.float32)


def procedural(pkg, params, func, scale=1.0, offset=0.0, minimum=None, slot="mean"):
    p = np.array(pkg.as_params(params))
    p[slot]["type"] = pkg.MEAN_TYPE.PROCEDURAL
    p[slot]["func"] = pkg.SDF_FUNCTION.NAMES[func]
    p[slot]["scale"] = scale
    p[slot]["offset"] = offset
    p[slot]["min"] = -np.finfo(np.float32).max if minimum is None else minimum
    if slot == "mean_additional":
        p["has_mean_additional"] = 1
    return p


def queries(pkg, n, seed, scale=0.9):
    """n evaluator queries around the knob: points, unit directions, path identities, a distance along the segment"""
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=pkg.QUERY)
    q["p"] = rng.uniform(-scale, scale, (n, 3))
    d = rng.normal(size=(n, 3))
    q["dir"] = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    q["t_segment"] = rng.uniform(0, 1.5, n)
    q["info_t"] = rng.uniform(0, 3, n)
    q["pixel"] = rng.integers(0, 512, (n, 2))
    q["spp"] = rng.integers(0, 64, n)
    q["segment"] = rng.integers(0, 4, n)
    q["scene_seed"] = rng.integers(0, 2 ** 31, n)
    return q


def nee_queries(pkg, points, grad, seed):
    """one NEE query per point: a random unit ray_dir, the normal = normalised (mean gradient + a random vector of length <= 0.8)
    (random normals alone leave pdf > 0 on a fifth of the queries), path identities, and on every second query a conditioning record
    anchored at the segment's start"""
    rng = np.random.default_rng(seed)
    n = len(points)
    q = np.zeros(n, dtype=pkg.NEE_QUERY)
    q["p"] = points
    d = rng.normal(size=(n, 3))
    q["ray_dir"] = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    v = rng.normal(size=(n, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0, 0.8, (n, 1))
    nrm = np.asarray(grad, dtype=np.float64) + v
    q["normal"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(f32)
    q["t_segment"] = rng.uniform(0, 1.5, n)
    q["info_t"] = rng.uniform(0, 3, n)
    q["pixel"] = rng.integers(0, 512, (n, 2))
    q["spp"] = rng.integers(0, 64, n)
    q["segment"] = rng.integers(0, 4, n)
    q["scene_seed"] = rng.integers(0, 2 ** 31, n)
    cond = (np.arange(n) % 2 == 1)[:, None]
    q["coeff"]["value_scale"] = np.where(cond[:, 0], rng.normal(0, 0.05, n), 0)
    q["coeff"]["gradient_scale"] = np.where(cond, rng.normal(0, 0.5, (n, 3)), 0)
    q["coeff"]["ray_origin"] = np.where(cond, q["p"] - q["ray_dir"] * q["t_segment"][:, None], 0)
    return q


def camera_rays(pkg, n, seed, bound=1.5, first_scatter=True, state=None):
    """n camera-like rays through the ball of radius `bound`: from a pinhole at (0.3, 0.4, 4) towards points of the ball, clipped
    to it (near_t / far_t); continued segments start from `state` = (last_val, last_aniso, last_gp_id) arrays"""
    rng = np.random.default_rng(seed)
    eye = np.array([0.3, 0.4, 4.0])
    tgt = rng.normal(size=(n, 3))
    tgt = tgt / np.linalg.norm(tgt, axis=1)[:, None] * (bound * 0.93 * rng.uniform(0, 1, (n, 1)) ** (1 / 3))
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1)[:, None]
    d32 = d.astype(f32)
    dd = d32.astype(np.float64)
    dd /= np.linalg.norm(dd, axis=1)[:, None]
    b = (dd * eye).sum(1)
    disc = b * b - (eye @ eye - bound * bound)
    assert (disc > 0).all()
    r = np.zeros(n, dtype=pkg.RAY_IN)
    r["pos"] = eye
    r["dir"] = d32
    r["near_t"] = -b - np.sqrt(disc)
    r["far_t"] = -b + np.sqrt(disc)
    r["u_jitter"] = rng.uniform(0, 1, n)
    r["pixel"] = rng.integers(0, 512, (n, 2))
    r["spp"] = rng.integers(0, 16, n)
    r["segment"] = 0
    r["scene_seed"] = 99
    r["first_scatter"] = 1 if first_scatter else 0
    r["bounce"] = 0
    if not first_scatter:
        r["last_val"], r["last_aniso"], r["last_gp_id"] = state
        r["segment"] = 1
        r["bounce"] = 1
    return r


class SdfComposite:
    def __init__(self, pkg, ob, params, transforms=(None, None), threads=16):
        self.pkg, self.ob = pkg, ob
        self.params = np.array(pkg.as_params(params))
        self.transforms = transforms
        self.threads = threads
        self.noise = ob.Oracle(noise_only(pkg, params), threads=threads)
        self.mref = sdf_mean_ref.SdfMeanRef()
        self.derived = self.noise.derived()
        P = self.params
        self.sigma_s_over_t = np.array([f32(f32(P["sigma_s"][c]) * f32(P["density"])) /
                                        f32(f32(f32(P["sigma_a"][c]) * f32(P["density"])) + f32(f32(P["sigma_s"][c]) * f32(P["density"])))
                                        for c in range(3)], dtype=f32)
        self.last_n_eval = 0          # noise evaluations of the last sample_distance / transmittance batch, counted as the device counts

    # ---- the three evaluator formulas -----------------------------------------------------------------------------
    def mean(self, points):
        return self.mref.mean(self.params, points, self.transforms)

    def eval_value(self, q):
        v0, _ = self.noise.eval_value(q)
        m, gid, _ = self.mean(np.asarray(q["p"], dtype=f32).astype(np.float64))
        return (v0.astype(np.float64) + m).astype(f32), gid

    def eval_gradient(self, q):
        g0 = self.noise.eval_gradient(q)
        _, _, g = self.mean(np.asarray(q["p"], dtype=f32).astype(np.float64))
        return (g0 + g.astype(f32)).astype(f32)

    def conditioning(self, q, target_val, target_grad):
        m, _, g = self.mean(np.asarray(q["p"], dtype=f32).astype(np.float64))
        tv = (np.asarray(target_val, dtype=f32) - m.astype(f32)).astype(f32)
        tg = (np.asarray(target_grad, dtype=f32) - g.astype(f32)).astype(f32)
        return self.noise.conditioning(q, tv, tg)

    def mean_color_emission(self, points):
        """colour at Vec3d(T^-1 . Vec3f(a)) when the primary mean is procedural (ProceduralMean::color), emission at a itself"""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        orc = self.noise                  # the ramps of the colour / emission fields are the oracle's own
        pc = p
        if int(self.params["mean"]["type"]) == self.pkg.MEAN_TYPE.PROCEDURAL:
            T = np.eye(4, dtype=f32) if self.transforms[0] is None else self.transforms[0]
            pc = self.mref.transform_point(self.mref.invert(T), p.astype(f32)).astype(np.float64)
        col, _ = orc.mean_color_emission(pc)
        _, emi = orc.mean_color_emission(p)
        return col, emi

    # ---- NEE: the oracle itself through a linear stand-in ------------------------------------------------------------
    def nee_standin(self, q):
        """(k, s) per NEE query: the mean's gradient at double(float(p)), from the slot the CSG id selects, narrowed to float, is
        s * e_k (k = -1, s = 0: the zero gradient).  Raises on a query whose gradient has more than one non-zero component."""
        p = np.asarray(q["p"], dtype=f32).astype(np.float64).reshape(-1, 3)
        g = self.mean(p)[2].astype(f32)
        nz = g != 0
        if (nz.sum(axis=1) > 1).any():
            bad = np.nonzero(nz.sum(axis=1) > 1)[0]
            raise ValueError("NEE reference: the mean gradient of %d queries is not axis-aligned (first: %d, %r)" % (len(bad), bad[0], g[bad[0]]))
        k = np.where(nz.any(axis=1), nz.argmax(axis=1), -1)
        s = np.where(k >= 0, g[np.arange(len(g)), np.maximum(k, 0)], f32(0)).astype(f32)
        return k, s

    def _nee_oracle(self, k, s):
        """the oracle of this medium with the mean replaced by the one whose gradient is exactly s * e_k in float: LinearMean with
        dir = sign(s) * e_k, scale = |s|, min = -FLT_MAX, centre 0, no CSG partner (the zeros of its gradient are positive, as the
        one-sided difference's are); the homogeneous mean 0 for the zero gradient.  nee_shared reads the mean's gradient alone."""
        if k < 0:
            return self.noise
        cache = self.__dict__.setdefault("_nee_oracles", {})
        key = (int(k), np.array(s, dtype=f32).view(np.uint32).item())
        if key not in cache:
            p = noise_only(self.pkg, self.params)
            mu = p["mean"]
            mu["type"] = self.pkg.MEAN_TYPE.LINEAR
            mu["center"] = 0.0
            d = np.zeros(3)
            d[k] = -1.0 if s < 0 else 1.0
            mu["dir"] = d
            mu["scale"] = abs(f32(s))
            mu["min"] = -np.finfo(f32).max
            cache[key] = self.ob.Oracle(p, threads=self.threads)
        return cache[key]

    def _nee(self, q, what):
        q = np.ascontiguousarray(q, dtype=self.pkg.NEE_QUERY)
        k, s = self.nee_standin(q)
        out = np.zeros(len(q), dtype=f32) if what == "pdf" else np.zeros((len(q), 3), dtype=f32)
        keys = np.stack([k.astype(np.int64), s.view(np.uint32).astype(np.int64)], axis=1)
        for kk, sb in np.unique(keys, axis=0):
            idx = np.nonzero((keys[:, 0] == kk) & (keys[:, 1] == sb))[0]
            orc = self._nee_oracle(int(kk), np.array(sb, dtype=np.uint32).view(f32))
            out[idx] = orc.nee_pdf(q[idx]) if what == "pdf" else orc.nee_grad(q[idx])
        return out

    def nee_pdf(self, q):
        return self._nee(q, "pdf")

    def nee_grad(self, q):
        return self._nee(q, "grad")

    # ---- the march ------------------------------------------------------------------------------------------------
    def _query(self, rays, idx, t, coeff):
        """evaluator queries at ray(t) for the rays idx: Vec3f(p + t * rd) in double, narrowed"""
        r = rays[idx]
        q = np.zeros(len(idx), dtype=self.pkg.QUERY)
        p = r["pos"].astype(np.float64) + t[:, None] * r["dir"].astype(np.float64)
        q["p"] = p.astype(f32)
        q["dir"] = r["dir"]
        q["t_segment"] = t.astype(f32)
        q["info_t"] = r["info_t"]
        q["pixel"], q["spp"], q["segment"], q["scene_seed"] = r["pixel"], r["spp"], r["segment"], r["scene_seed"]
        q["coeff"] = coeff[idx]
        return q

    def _value(self, rays, idx, t, coeff):
        if len(idx) == 0:
            return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32)
        v, gid = self.eval_value(self._query(rays, idx, t, coeff))
        return v.astype(np.float64), gid

    def _intersect(self, rays, first, last_val, last_aniso):
        """intersectGP for every ray at once: (hit, t, trips, gp_id, last_val, coeff)"""
        P = self.params
        n = len(rays)
        near, far = rays["near_t"].astype(f32), rays["far_t"].astype(f32)
        step = ((far - near) / f32(int(P["min_step"]))).astype(f32)
        step = np.where(f32(P["step_size"]) < step, f32(P["step_size"]), step).astype(f32)
        coeff = np.zeros(n, dtype=self.pkg.COND_COEFF)
        nev = np.zeros(n, dtype=np.int64)        # noise evaluations per ray (gpis_cond_coeff.n_evals); 3D sampling only
        allr = np.arange(n)
        cont = np.nonzero(~first)[0]
        if len(cont):
            q = self._query(rays, cont, np.zeros(len(cont)), coeff)
            q["p"] = rays["pos"][cont]
            coeff[cont] = self.conditioning(q, last_val[cont].astype(f32), last_aniso[cont].astype(f32))
            if int(self.derived["activate_conditioning"]):
                # 3D conditioning (SCN.cpp:431-595 as csrc/gpis_path.inc counts it): the unconditioned evaluation, the discarded
                # re-evaluation, and with Renewal+ the second unconditioned evaluation and the second discarded one
                nev[cont] += 4 if int(P["correlation_context"]) == self.pkg.CTX.RENEWAL_PLUS else 2
        t = near.astype(np.float64)
        f0, gp = self._value(rays, allr, t, coeff)
        nev += 1
        sign0 = np.where(f0 < 0, -1, 1)
        pf = f0.copy()
        t = (near + (step * rays["u_jitter"].astype(f32)).astype(f32)).astype(f32).astype(np.float64)
        stepno = np.zeros(n, dtype=np.int64)
        hit = np.zeros(n, dtype=bool)
        done = np.zeros(n, dtype=bool)
        t_out = far.astype(np.float64)
        trips = np.zeros(n, dtype=np.int64)
        out_val = np.zeros(n, dtype=f32)
        while True:
            act = np.nonzero(~done & (t < far.astype(np.float64)))[0]
            if len(act) == 0:
                break
            stepno[act] += 1
            nev[act] += 1
            fc, g = self._value(rays, act, t[act], coeff)
            gp[act] = g
            signc = np.where(fc < 0, -1, 1)
            reset = (~first[act]) & (stepno[act] == 1)
            sign0[act[reset]] = signc[reset]
            cross = ~reset & (signc != sign0[act])
            for j in np.nonzero(cross)[0]:          # the refinement of one crossing (scalar: few rays reach it per step)
                i = act[j]
                one = np.array([i])
                intp = pf[i] / (pf[i] - fc[j])
                a = t[i] - np.float64(step[i])
                lerp = lambda ratio: a * (1.0 - ratio) + t[i] * ratio
                t_prev = lerp(intp)
                while True:
                    trips[i] += 1
                    nev[i] += 1
                    t_test = lerp(intp)
                    ft, g1 = self._value(rays, one, np.array([t_test]), coeff)
                    gp[i] = g1[0]
                    if (-1 if ft[0] < 0 else 1) == sign0[i]:
                        break
                    intp *= 0.9
                    if intp <= 0.01:
                        t_prev = t_test = 0.0
                        break
                    t_prev = t_test
                t_out[i] = t_prev
                hit[i] = True
                done[i] = True
            keep = ~cross
            pf[act[keep]] = fc[keep]
            t[act[keep]] = t[act[keep]] + step[act[keep]].astype(np.float64)
        ex = np.nonzero(~hit)[0]
        nev[ex] += 1
        v, g = self._value(rays, ex, far[ex].astype(np.float64), coeff)
        gp[ex] = g
        out_val[ex] = v.astype(f32)
        return hit, t_out, trips, gp, out_val, coeff, nev

    def _gradient(self, rays, idx, t, coeff):
        """sampleGradient at ro + rd_normalised * t (GPM.cpp:280-283)"""
        r = rays[idx]
        rd = r["dir"].astype(np.float64)
        l2 = np.zeros(len(idx))
        for k in range(3):
            l2 = l2 + rd[:, k] * rd[:, k]
        inv = 1.0 / np.sqrt(l2)
        q = self._query(rays, idx, t, coeff)
        q["p"] = (r["pos"].astype(np.float64) + (rd * inv[:, None]) * t[:, None]).astype(f32)
        return self.eval_gradient(q).astype(np.float64), q["p"].astype(np.float64)

    def sample_distance(self, rays, want_coeff=False, want_trips=False):
        """the scattering branch of sampleDistance for finite segments with far_t > 0 and bounce < max_bounces"""
        pkg = self.pkg
        rays = np.ascontiguousarray(rays, dtype=pkg.RAY_IN)
        n = len(rays)
        assert np.isfinite(rays["far_t"]).all() and (rays["far_t"] != 0).all() and (rays["bounce"] < int(self.params["max_bounces"])).all()
        first = rays["first_scatter"] != 0
        hit, t, trips, gp, exit_val, coeff, nev = self._intersect(rays, first, rays["last_val"], rays["last_aniso"])
        far = rays["far_t"].astype(f32)
        out = np.zeros(n, dtype=pkg.SEG_OUT)
        allr = np.arange(n)
        nev += 1                                              # the one gradient evaluation of every segment
        coeff["n_evals"] = nev
        self.last_n_eval = int(nev.sum())
        aniso, _ = self._gradient(rays, allr, t, coeff)      # t < maxT: after the march; t == maxT (exit): the else branch of GPM.cpp:318-321
        d = np.zeros(n)
        l2 = np.zeros(n)
        dirs = rays["dir"].astype(np.float64)
        for k in range(3):
            d = d + aniso[:, k] * dirs[:, k]
            l2 = l2 + aniso[:, k] * aniso[:, k]
        # a hit whose gradient is not finite (a refinement that fell back to t = 0 on a continued segment of a Matern medium: the
        # conditioning kernel's derivative at distance 0 is 0 / 0) fails the segment before the two sign tests (GPM.cpp:291)
        nonfinite = hit & ~np.isfinite((aniso[:, 0] + aniso[:, 1] + aniso[:, 2]) / 3.0)
        wrong = hit & ~nonfinite & (d > 0)
        zero = hit & ~nonfinite & ~wrong & (l2 < np.float64(f32(0.0000001)))
        bad = wrong | zero | nonfinite
        aniso[zero | nonfinite] = (1.0, 0.0, 0.0)
        out["t"] = t
        out["exited"] = ~hit
        out["aniso"] = aniso
        out["last_val"] = np.where(hit, f32(0), exit_val)
        out["gp_id"] = np.where(hit, gp, rays["last_gp_id"])
        ok = ~bad
        ft = t.astype(f32)
        out["sample_t"] = np.where(ok, np.where(ft < far, ft, far), f32(0))
        out["continued_t"] = np.where(ok, ft, f32(0))
        col = np.ones((n, 3), dtype=np.float64)
        h = np.nonzero(hit & ok)[0]
        if len(h) and int(self.params["mean_color"]["enabled"]):
            r = rays[h]
            rd = r["dir"].astype(np.float64)
            rd = rd * (1.0 / np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2]))[:, None]
            c, _ = self.mean_color_emission(r["pos"].astype(np.float64) + rd * t[h][:, None])
            col[h] = c
        w = (col.astype(f32) * self.sigma_s_over_t[None, :]).astype(f32)
        out["weight"] = np.where(ok[:, None], w, f32(0))
        out["continued_weight"] = out["weight"]
        out["scheme"] = np.where(hit & ok, int(self.derived["effective_scheme_1d"]), 0)
        pp = (rays["pos"].astype(f32) + rays["dir"].astype(f32) * out["sample_t"][:, None]).astype(f32)
        out["p"] = np.where(ok[:, None], pp, f32(0))
        out["ok"] = ok
        res = [out]
        if want_coeff:
            res.append(coeff)
        if want_trips:
            res.append(trips)
        return tuple(res) if len(res) > 1 else out

    def transmittance(self, rays):
        rays = np.ascontiguousarray(rays, dtype=self.pkg.RAY_IN)
        first = rays["first_scatter"] != 0
        hit, t, trips, gp, exit_val, coeff, nev = self._intersect(rays, first, rays["last_val"], rays["last_aniso"])
        vis = ~hit
        self.last_n_eval = int(nev.sum() + hit.sum())         # a hit evaluates the gradient, an exit does not
        return vis.astype(np.uint8)     # t < maxT: the gradient is evaluated; finite or not, the segment is blocked

    def scene_s_primary(self, scene, x, y, spp):
        return self.noise.scene_s_primary(scene, x, y, spp)
