// gpis_material_rgb.hpp — the per-bounce kernels of gpis_render_scene_s_material_paths_rgb: the RGB path estimator of
// gpis_render_scene_s_nee_paths_rgb with the material of every hit chosen by its GP id (GPM.cpp:335: sample.phase =
// _phaseFunctions[state.lastGPId]), a BRDFPhaseFunction over a ConductorBsdf or over a LambertBsdf, under one cap light.
//
// A section of tu_scene.hip in a file of its own: it is included there once, BEHIND gpis_cond_rgb.hpp (CondRgbArrays,
// k_cond_rgb_emit, k_cond_rgb_gather, which this driver launches as they are), and is no header for another unit.  The marches,
// neePDF / neeGrad and the camera step are launched as the RGB conductor driver launches them.  One thread per sample, 256 threads
// per workgroup, no LDS.
//
// The two kernels switch per lane on the hit's material around nee_setup_sample / nee_shade_sample with N = 3 (CONDUCTOR) and the
// steps L1-L4 of include/gpis.h (LAMBERT).  A Lambert hit asks for no neePDF / neeGrad query: its want_* masks are 0, and its light
// and phase shadow rays go into b.shadow_light / b.shadow_phase, so that the two transmittance launches and k_cond_rgb_gather
// serve both materials.
//
// The table is a kernel argument.  A lane reads its material through material_pick: every field is loaded with constant indices
// and chosen by compares, because a kernel argument indexed by a lane's id is copied to scratch first.
#pragma once

#pragma clang fp contract(off)

struct MatAux {                        // per sample, between the set-up and the shading kernel
    NeeAuxN<3> n;                      // CONDUCTOR: as in the RGB conductor driver.  LAMBERT: d = the light direction, w = the phase
                                       //   direction w_p, v1 / v2 = the look-ahead jitters; F and scheme are not used
    float wo_z, wop_z;                 // LAMBERT: cos of the light direction and of the phase direction in the hit's frame
    uint32_t material;                 // the index into the table
    uint32_t _pad;
};

__device__ __forceinline__ uint32_t material_index(const gpis_materials_s &mt, int32_t gp_id)
{
    return (uint32_t)gp_id < mt.n_materials ? (uint32_t)gp_id : 0u;
}
// material[k] of the table with the table's light, as the surface nee_setup_sample / nee_shade_sample take
__device__ __forceinline__ float material_pick(float m0, float m1, float m2, float m3, uint32_t k)
{
    float v = m0;
    if (k == 1) v = m1;
    if (k == 2) v = m2;
    if (k == 3) v = m3;
    return v;
}
__device__ __forceinline__ gpis_surface_rgb_s material_surface(const gpis_materials_s &mt, uint32_t k, int32_t &type)
{
    const gpis_material_rgb *M = mt.material;
    gpis_surface_rgb_s sf;
    for_channels<3>([&](int c) __attribute__((always_inline)) {
        sf.eta[c] = material_pick(M[0].eta[c], M[1].eta[c], M[2].eta[c], M[3].eta[c], k);
        sf.k[c] = material_pick(M[0].k[c], M[1].k[c], M[2].k[c], M[3].k[c], k);
        sf.albedo[c] = material_pick(M[0].albedo[c], M[1].albedo[c], M[2].albedo[c], M[3].albedo[c], k);
        sf.cap_radiance[c] = mt.cap_radiance[c];
        sf._pad[c] = 0.f;
    });
    sf.cap_cos = mt.cap_cos;
    type = M[0].type;
    if (k == 1) type = M[1].type;
    if (k == 2) type = M[2].type;
    if (k == 3) type = M[3].type;
    return sf;
}

// LambertBsdf::sample's direction in the hit's frame: the unit-disk rejection of k_paths_rgb_shade
__device__ __forceinline__ V3 lambert_disk_sample(Pcg32 &g)
{
    float dx, dy, d2;
    do {
        dx = 2.f * normalized_uint(g.next_i()) - 1.f;
        dy = 2.f * normalized_uint(g.next_i()) - 1.f;
        d2 = dx * dx + dy * dy;
    } while (!(d2 < 1.f));
    const float rem = 1.0f - d2;
    return v3(dx, dy, sqrtf(rem > 0.f ? rem : 0.f));
}

// wi of the hit `o` of `ray` in the frame of its normal, as nee_setup_sample states it
__device__ __forceinline__ V3 material_wi(const gpis_ray_in &ray, const gpis_seg_out &o, Frame &fr)
{
    fr = frame_from_normal(hit_normal(o));
    return normalized(to_local(fr, v3(-ray.dir[0], -ray.dir[1], -ray.dir[2])));
}

// Steps L1 and L2 up to the shadow segments: the light direction (always drawn) and, for wi.z > 0, the phase direction.
__device__ __forceinline__ void lambert_setup_sample(const SceneConst &sc, float cap_cos, const gpis_ray_in &ray, const gpis_seg_out &o, Pcg32 &g, MatAux &x)
{
    Frame fr;
    const V3 wi = material_wi(ray, o, fr);
    const V3 capDir = v3(sc.light[0], sc.light[1], sc.light[2]);
    const float z = normalized_uint(g.next_i()) * (1.0f - cap_cos) + cap_cos;
    float dx, dy, d2;
    do {
        dx = 2.f * normalized_uint(g.next_i()) - 1.f;
        dy = 2.f * normalized_uint(g.next_i()) - 1.f;
        d2 = dx * dx + dy * dy;
    } while (!(d2 < 1.f) || !(d2 > 1e-12f));
    const float rr = 1.0f - z * z;
    const float rad = sqrtf(rr > 0.f ? rr : 0.f) / sqrtf(d2);
    const Frame cf = frame_from_normal(capDir);
    const V3 d = to_global(cf, v3(dx * rad, dy * rad, z));
    const V3 wo = normalized(to_local(fr, d));
    x.n.d[0] = d.x; x.n.d[1] = d.y; x.n.d[2] = d.z;
    x.wo_z = wo.z;
    x.n.w[0] = x.n.w[1] = x.n.w[2] = 0.f;
    x.wop_z = 0.f;
    if (wi.z > 0.0f) {
        const V3 wop = lambert_disk_sample(g);
        const V3 w = normalized(to_global(fr, wop));
        x.n.w[0] = w.x; x.n.w[1] = w.y; x.n.w[2] = w.z;
        x.wop_z = wop.z;
    }
    x.n.F[0] = x.n.F[1] = x.n.F[2] = 0.f;
    x.n.scheme = o.scheme;
}

// After sampleDistance of segment `bounce`: k_cond_rgb_setup's step with the material of the hit.
__global__ void __launch_bounds__(256) k_mat_rgb_setup(SceneConst sc, gpis_materials_s mt, size_t n_samples, int bounce, int max_bounces, int emissive,
                                                       PathArrays a, NeeArrays b, NeePathArrays c, CondRgbArrays r, MatAux *aux)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t wl = 0, wp = 0, wn = 0, emit = 0;
    V3d at = {0., 0., 0.};
    if (a.alive[i]) {
        c.segs[i] += 1;
        uint8_t hit = 0;
        const gpis_seg_out o = a.seg[i];
        if (o.ok && !o.exited) {        // the light seen directly is never added, and nothing reads the throughput of a path that left
            float thr[3];
            for (int ch = 0; ch < 3; ++ch) thr[ch] = bounce == 0 ? 1.f : r.thr[ch * r.plane + i];
            const gpis_ray_in ray = a.rays[i];
            if (emissive) {
                // ro + rd * t: the point of GPM.cpp:317 and of gpis_mean_color_emission_*
                V3d rd = to_d(v3(ray.dir[0], ray.dir[1], ray.dir[2]));
                { double inv = 1.0 / length_d(rd); rd.x *= inv; rd.y *= inv; rd.z *= inv; }
                at = ray_at(to_d(v3(ray.pos[0], ray.pos[1], ray.pos[2])), rd, o.t);
                emit = 1;
            }
            for (int ch = 0; ch < 3; ++ch) thr[ch] = thr[ch] * o.weight[ch];
            if (bounce + 1 < max_bounces) {
                Pcg32 g;
                g.state = a.rng[i];
                MatAux x;
                x.wo_z = x.wop_z = 0.f;
                const uint32_t k = material_index(mt, o.gp_id);
                int32_t type;
                const gpis_surface_rgb_s sf = material_surface(mt, k, type);
                if (type == GPIS_MATERIAL_CONDUCTOR)
                    nee_setup_sample(sc, sf, ray, o, g, i, b, x.n, wl, wp, wn);
                else
                    lambert_setup_sample(sc, sf.cap_cos, ray, o, g, x);
                a.rng[i] = g.state;     // v1, v2 look ahead: how many of them the shadow segments take is known in k_mat_rgb_shade
                x.n.v1 = normalized_uint(g.next_i());
                x.n.v2 = normalized_uint(g.next_i());
                x.material = k;
                x._pad = 0;
                aux[i] = x;
                for (int ch = 0; ch < 3; ++ch) r.thr_hit[ch * r.plane + i] = thr[ch];
                hit = 1;
            }
        }
        a.alive[i] = hit;
    }
    b.want_light[i] = wl;
    b.want_phase[i] = wp;
    b.want_pdf_normal[i] = wn;
    if (emissive) {
        r.points[3 * i] = at.x; r.points[3 * i + 1] = at.y; r.points[3 * i + 2] = at.z;
        r.emit[i] = emit;
    }
}

// Steps L1 and L2 from the shadow segments on: which are marched (gl, gp) and what each adds to L when it is visible.
__device__ __forceinline__ void lambert_shade_sample(const SceneConst &sc, const gpis_surface_rgb_s &sf, const gpis_ray_in &ray, const gpis_seg_out &o,
                                                     const MatAux &x, float wi_z, size_t i, const NeeArrays &b, float *contrib_light, float *contrib_phase,
                                                     size_t plane, uint8_t &gl, uint8_t &gp)
{
    const float pdf_l = (0.5f * (1.0f / 3.1415926536f)) / (1.0f - sf.cap_cos);
    const V3 capDir = v3(sc.light[0], sc.light[1], sc.light[2]);
    const V3 p = v3(o.p[0], o.p[1], o.p[2]);
    const gpis_ray_in sh0 = scene_next_ray(ray, o);      // handleVolume's copy of the state: last_aniso is the hit's own
    {
        float f[3];
        bool some = false;
        const bool lit = wi_z > 0.0f && x.wo_z > 0.0f;
        for_channels<3>([&](int c) __attribute__((always_inline)) {
            f[c] = lit ? sf.albedo[c] * (1.0f / 3.1415926536f) * x.wo_z : 0.0f;
            some = some || f[c] != 0.0f;
        });
        float t0, t1;
        const V3 d = v3(x.n.d[0], x.n.d[1], x.n.d[2]);
        if (some && sphere_chord(p, d, sc.s.bound_radius, t0, t1)) {
            gpis_ray_in sh = sh0;
            sh.dir[0] = d.x; sh.dir[1] = d.y; sh.dir[2] = d.z;
            sh.far_t = t1;
            sh.u_jitter = x.n.v1;
            b.shadow_light[i] = sh;
            const float pdf = x.wo_z * (1.0f / 3.1415926536f);
            for_channels<3>([&](int c) __attribute__((always_inline)) {
                const float e = 1.f * sf.cap_radiance[c];
                float lightF = f[c] * e / pdf_l;
                lightF *= power_heuristic(pdf_l, pdf);
                contrib_light[c * plane + i] = lightF;
            });
            gl = 1;
        }
    }
    if (wi_z > 0.0f) {
        float t0, t1;
        const V3 w = v3(x.n.w[0], x.n.w[1], x.n.w[2]);
        if (!(dot(w, capDir) < sf.cap_cos) && sphere_chord(p, w, sc.s.bound_radius, t0, t1)) {
            gpis_ray_in sh = sh0;
            sh.dir[0] = w.x; sh.dir[1] = w.y; sh.dir[2] = w.z;
            sh.far_t = t1;
            sh.u_jitter = gl ? x.n.v2 : x.n.v1;
            b.shadow_phase[i] = sh;
            const float pdf = x.wop_z * (1.0f / 3.1415926536f);
            for_channels<3>([&](int c) __attribute__((always_inline)) {
                const float e = 1.f * sf.cap_radiance[c];
                float phaseF = e * sf.albedo[c];
                phaseF *= power_heuristic(pdf, pdf_l);
                contrib_phase[c * plane + i] = phaseF;
            });
            gp = 1;
        }
    }
}

// After neePDF / neeGrad: k_cond_rgb_shade's step with the material of the hit.  n_marched as there.
__global__ void __launch_bounds__(256) k_mat_rgb_shade(SceneConst sc, gpis_materials_s mt, size_t n_samples, int bounce, int n_marched, PathArrays a,
                                                       NeeArrays b, NeePathArrays c, CondRgbArrays r, const MatAux *aux)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t gl = 0, gp = 0;
    if (a.alive[i]) {       // hit at this bounce
        const gpis_seg_out o = a.seg[i];
        const gpis_ray_in ray = a.rays[i];
        const MatAux &x = aux[i];           // read in place: a local copy lands in scratch (v1 / v2 are picked by address)
        int32_t type;
        const gpis_surface_rgb_s sf = material_surface(mt, x.material, type);
        const bool lambert = type != GPIS_MATERIAL_CONDUCTOR;
        Frame fr;
        float wi_z = 0.f;
        if (lambert) {
            wi_z = material_wi(ray, o, fr).z;
            lambert_shade_sample(sc, sf, ray, o, x, wi_z, i, b, r.contrib_light, r.contrib_phase, r.plane, gl, gp);
        } else if (b.want_light[i] || b.want_phase[i]) {
            nee_shade_sample(sc, sf, ray, o, x.n, i, b, r.contrib_light, r.contrib_phase, r.plane, gl, gp);
        }
        c.segs[i] += (uint32_t)gl + (uint32_t)gp;
        Pcg32 g;
        g.state = a.rng[i];
        for (int k = 0; k < (int)gl + (int)gp; ++k)     // one jitter per shadow segment that is marched
            (void)g.next_i();
        // the bounce: no Russian roulette; throughput.max() == 0 ends the path (PathTracer.cpp:143, Vec.hpp:418-425)
        V3 w = v3(x.n.w[0], x.n.w[1], x.n.w[2]);        // CONDUCTOR: the mirror direction
        bool alive = true;
        if (lambert) {                                  // a second, independent cosine sample (TraceBase.cpp:552)
            alive = wi_z > 0.0f;
            if (alive)
                w = normalized(to_global(fr, lambert_disk_sample(g)));
        }
        float thr[3];
        for (int ch = 0; ch < 3; ++ch) {
            thr[ch] = r.thr_hit[ch * r.plane + i] * (lambert ? sf.albedo[ch] : x.n.F[ch]);
            r.thr[ch * r.plane + i] = thr[ch];
        }
        float top = thr[0];
        if (thr[1] > top) top = thr[1];
        if (thr[2] > top) top = thr[2];
        float t0, t1;
        alive = alive && !(top == 0.0f) && sphere_chord(v3(o.p[0], o.p[1], o.p[2]), w, sc.s.bound_radius, t0, t1) && bounce + 1 < n_marched;
        if (alive) {
            gpis_ray_in next = scene_next_ray(ray, o);
            next.dir[0] = w.x; next.dir[1] = w.y; next.dir[2] = w.z;
            next.far_t = t1;
            next.u_jitter = normalized_uint(g.next_i());
            a.rays[i] = next;
        }
        a.rng[i] = g.state;
        a.alive[i] = alive ? 1 : 0;
    }
    b.go_light[i] = gl;
    b.go_phase[i] = gp;
}
