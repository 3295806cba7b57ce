// gpis_cond_rgb.hpp — the per-bounce kernels of gpis_render_scene_s_nee_paths_rgb: the conductor NEE / MIS path estimator of
// gpis_render_scene_s_nee_paths carried in RGB (ConductorBsdf's Vec3f eta / k, Fresnel.hpp:136-143; a Vec3f cap emission), with the
// medium's per-channel weight and its emission (PathTracer.cpp:72-73, as gpis_paths_rgb.hpp).
//
// A section of tu_scene.hip in a file of its own: it is included there once, BEHIND the mono estimator (PathArrays, NeeArrays,
// NeePathArrays, NeeAuxN, nee_setup_sample, nee_shade_sample), and is no header for another unit.  The marches, neePDF / neeGrad,
// the camera step (k_paths_begin, k_paths_adaptive_begin) and the directions, queries, shadow rays and draws (nee_setup_sample,
// nee_shade_sample with N = 3) are the mono driver's; only F, the contributions, the throughput and the emission carry colour.
// One thread per sample, 256 threads per workgroup, no LDS.  Colour state is SoA as PathsRgbArrays': channel c of sample i at
// [c * plane + i].  The mono planes of the workspace (a.throughput, a.emission, c.thr_hit, b.contrib_*, b.aux) are written by the
// camera step or not at all and never read.
//
// Per bounce the order of additions into a sample's em is: the hit's own emission (thr BEFORE the segment's weight, the product
// rounded to float on its own: k_cond_rgb_emit), then, after the shadow marches, thr_hit * L (k_cond_rgb_gather).
// The emission itself is evaluated by gpis_mean_color_emission_batch, launched as it is on the points k_cond_rgb_setup leaves: the
// noise evaluators behind field_vec are real functions, and a kernel that calls them carries their call frames as scratch
// (k_paths_rgb_shade does); the kernels here carry none.  That launch has no mask: the slots that did not hit evaluate the origin,
// and nothing reads their result.
#pragma once

#pragma clang fp contract(off)

struct CondRgbArrays {                 // per sample; `plane` floats per channel plane
    float *thr, *thr_hit, *em;         // throughput, throughput at this bounce's hit (weight included, F not), emission
    float *contrib_light, *contrib_phase;
    NeeAuxN<3> *aux;
    double *points;                    // emissive media only: 3 per sample, where the hit's emission is evaluated (the origin elsewhere)
    float *e3;                         //   3 per sample, interleaved: gpis_mean_color_emission_batch's output
    uint8_t *emit;                     //   the sample hit at this bounce
    size_t plane;
};

// After sampleDistance of segment `bounce` (k_nee_paths_setup's step): the segment count, !ok / exited, on an emissive medium the
// point of the hit's emission, the weight (r.thr keeps the throughput before it until k_cond_rgb_shade), and — unless this is the
// extra last segment of an emissive medium — the set-up of the two estimators.  a.alive[i] becomes "hit, and the estimators follow".
__global__ void __launch_bounds__(256) k_cond_rgb_setup(SceneConst sc, gpis_surface_rgb_s sf, size_t n_samples, int bounce, int max_bounces, int emissive,
                                                        PathArrays a, NeeArrays b, NeePathArrays c, CondRgbArrays r)
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
                NeeAuxN<3> x;
                nee_setup_sample(sc, sf, ray, o, g, i, b, x, wl, wp, wn);
                a.rng[i] = g.state;     // v1, v2 look ahead: how many of them the shadow segments take is known after neePDF
                x.v1 = normalized_uint(g.next_i());
                x.v2 = normalized_uint(g.next_i());
                r.aux[i] = x;
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

// Emissive media, after gpis_mean_color_emission_batch on r.points: em[c] = em[c] + (thr[c] * e[c]) with the throughput BEFORE this
// segment's weight (1 at the first bounce, where r.thr is not written yet).
__global__ void __launch_bounds__(256) k_cond_rgb_emit(size_t n_samples, int bounce, CondRgbArrays r)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    if (!r.emit[i]) return;
    for (int ch = 0; ch < 3; ++ch) {
        const float thr = bounce == 0 ? 1.f : r.thr[ch * r.plane + i];
        const float prod = thr * r.e3[3 * i + ch];
        r.em[ch * r.plane + i] = r.em[ch * r.plane + i] + prod;
    }
}

// After neePDF / neeGrad (k_nee_paths_shade's step): the shadow segments and their contributions per channel, then the bounce.
// n_marched: the segments the host marches, max_bounces - 1 or, on an emissive medium, max_bounces; the next ray is drawn only if
// its segment is one of them.
__global__ void __launch_bounds__(256) k_cond_rgb_shade(SceneConst sc, gpis_surface_rgb_s sf, size_t n_samples, int bounce, int n_marched, PathArrays a,
                                                        NeeArrays b, NeePathArrays c, CondRgbArrays r)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    uint8_t gl = 0, gp = 0;
    if (a.alive[i]) {       // hit at this bounce
        const gpis_seg_out o = a.seg[i];
        const gpis_ray_in ray = a.rays[i];
        const NeeAuxN<3> &x = r.aux[i];     // read in place: a local copy lands in scratch (v1 / v2 are picked by address)
        if (b.want_light[i] || b.want_phase[i])
            nee_shade_sample(sc, sf, ray, o, x, i, b, r.contrib_light, r.contrib_phase, r.plane, gl, gp);
        c.segs[i] += (uint32_t)gl + (uint32_t)gp;
        Pcg32 g;
        g.state = a.rng[i];
        for (int k = 0; k < (int)gl + (int)gp; ++k)     // one jitter per shadow segment that is marched
            (void)g.next_i();
        // the bounce: no Russian roulette; throughput.max() == 0 ends the path (PathTracer.cpp:143, Vec.hpp:418-425)
        float thr[3];
        for (int ch = 0; ch < 3; ++ch) {
            thr[ch] = r.thr_hit[ch * r.plane + i] * x.F[ch];
            r.thr[ch * r.plane + i] = thr[ch];
        }
        float top = thr[0];
        if (thr[1] > top) top = thr[1];
        if (thr[2] > top) top = thr[2];
        float t0, t1;
        const V3 w = v3(x.w[0], x.w[1], x.w[2]);
        bool alive = !(top == 0.0f) && sphere_chord(v3(o.p[0], o.p[1], o.p[2]), w, sc.s.bound_radius, t0, t1) && bounce + 1 < n_marched;
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

// After the shadow marches: em[c] = em[c] + thr_hit[c] * L[c].  A hit without a shadow segment has L = 0 and leaves em as it is.
// L = 0 for both estimators iff cap_radiance is zero in every channel (TraceBase.cpp:374, 410 on a Vec3f).
__global__ void __launch_bounds__(256) k_cond_rgb_gather(float cap0, float cap1, float cap2, size_t n_samples, NeeArrays b, CondRgbArrays r)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_samples) return;
    if (!(b.go_light[i] || b.go_phase[i])) return;
    const bool lit = !(cap0 == 0.0f && cap1 == 0.0f && cap2 == 0.0f);
    const bool light = lit && b.go_light[i] && b.vis_light[i], phase = lit && b.go_phase[i] && b.vis_phase[i];
    for (int ch = 0; ch < 3; ++ch) {
        float L = 0.f;
        if (light) L += r.contrib_light[ch * r.plane + i];
        if (phase) L += r.contrib_phase[ch * r.plane + i];
        r.em[ch * r.plane + i] = r.em[ch * r.plane + i] + r.thr_hit[ch * r.plane + i] * L;
    }
}
