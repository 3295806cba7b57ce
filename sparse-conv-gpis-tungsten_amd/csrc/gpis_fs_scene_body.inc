// gpis_fs_scene_body.inc — the body of the fused scene-S kernels of the function-space medium (gpis_fs_scene.hpp), included once per
// kernel: k_fs_scene (GPIS_FS_SAMPLE_WHERE = first_pixel, a chunk with spp_count samples per pixel) and k_fs_scene_adaptive
// (GPIS_FS_SAMPLE_WHERE = ch, the records of an adaptive pass).  The macro names scene_sample's second argument; nothing else
// depends on the sample layout, and sample i of the chunk leaves recs[i] either way.  It reads the kernel's own parameters (Mp, sc,
// n_samples, next, recs, workspace, slots).  A text, not a function: as a GPIS_DEV template on that argument the same statements
// cost k_fs_scene 1.3 % of its frame time (DESIGN.md 5, "Adaptive sampling of the function-space drivers").
    __shared__ FsLds L;
    FsGlob &G = workspace[blockIdx.x];
    gpis_fs_state *st = slots + blockIdx.x;
    const DevModel &M = *Mp;
    const gpis_scene_s &s = sc.s;
    const int lane = (int)threadIdx.x;
    const V3 l = v3(sc.light[0], sc.light[1], sc.light[2]);
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(next, 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_samples) break;
        // ---- k_scene_primary, with the path's sampler in place of the four per-sample draws
        uint32_t x, y, spp;
        Pcg32 g = scene_sample(sc, GPIS_FS_SAMPLE_WHERE, i, x, y, spp);
        const float jx = normalized_uint(g.next_i()), jy = normalized_uint(g.next_i());
        FsSceneRec rec{0.f, 0u};
        gpis_ray_in ray;
        if (scene_camera_ray(sc, x, y, spp, jx, jy, ray)) {
            fs_reset_state(st, lane);            // the slot still holds the previous sample's context
            FsState state = fs_state_of(ray);
            FS_SYNC();
            const gpis_seg_out r = fs_sample_distance_one(M, L, G, g, &ray, st, state, lane);
            // ---- k_scene_shade
            if (r.ok && !r.exited) {
                rec.flags = 1u;
                const float c = dot(hit_normal(r), l);
                float s0, s1;
                if (c > 0.f && sphere_chord(v3(r.p[0], r.p[1], r.p[2]), l, s.bound_radius, s0, s1)) {
                    gpis_ray_in sh = scene_next_ray(ray, r);
                    sh.dir[0] = l.x; sh.dir[1] = l.y; sh.dir[2] = l.z;
                    sh.far_t = s1;
                    // the shadow segment: in place on the state (context and sampler) the primary segment left
                    FsState shadow = fs_state_of(sh);
                    FS_SYNC();
                    const bool vis = fs_transmittance_one(M, L, G, g, &sh, st, shadow, lane);
                    rec.cv = c * (vis ? 1.f : 0.f);
                    rec.flags = 3u;
                }
            }
        }
        if (lane == 0) recs[i] = rec;
    }
