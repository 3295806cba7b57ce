// gpis_host.hpp — host side of a sparse-convolution / function-space handle, shared by the translation units that implement its
// entries (gpis_hip.hip: model build, handle, batch and *_host entries; tu_scene.hip: the staged scene-S frame drivers).  The
// weight-space medium's counterpart is gpis_ws_host.hpp.
//
// The handle owns what it allocates: every member has an initialiser, every device or pinned block is a DevBuf / PinBuf
// (gpis_host_base.hpp, with the error layer and the *_host round trip), and ~gpis_medium releases the rest, so gpis_destroy and
// the failure paths of gpis_create are one delete.  The helpers declared here are defined in gpis_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "gpis.h"
#include "gpis_device.hpp"
#include "gpis_host_base.hpp"  // set_err, HIP_TRY, CHECK_ARGS, launch_check; DevBuf, PinBuf; host_round_trip
#include "gpis_scene.hpp"     // SceneRay, SceneHit
#include "gpis_tables.hpp"    // FastTable, GuideField: the records only, none of the fast or guided device code

// ======================================================================================
// handle
// ======================================================================================
struct gpis_medium {
    gpis_params params{};
    gpis::DevModel host_model{};
    gpis_derived derived{};
    int device = 0;
    gpis::DevBuf<gpis::DevModel> d_model;
    gpis::DevBuf<gpis::Counters> d_counters;
    gpis::FastTable fast{};    // single-realization wave-cooperative path (gpis_tables.hpp, gpis_fast.hpp); enabled == 0 when unused
    gpis::GuideField guide{};  // certified guide field (gpis_tables.hpp, gpis_guide.hpp); enabled == 0 until gpis_build_guide
    gpis::DevBuf<unsigned long long> d_guide_cnt;
    uint64_t selfcheck_tabulated = 0;   // points of the last gpis_guide_selfcheck that fell into tabulated bricks
    gpis::DevBuf<gpis::GuideField> d_guide;   // device copy of `guide` (the resident guided kernels read it through scalar loads instead of 14 kernel-argument SGPRs)
    gpis::DevBuf<float> d_grid_vox;      // GridNonstationaryCovariance voxels (gpis_set_variance_grid)
    gpis::DevBuf<float> d_mean_vox[2];   // TabulatedMean voxels of the two mean slots (gpis_set_mean_grid)
    unsigned lambert_calls = 0;       // gpis_render_scene_s calls so far (the first one works in small chunks, see lambert_ws_plan)
    gpis::DevBuf<> fs_ws;             // function-space workspace: one FsGlob per resident workgroup (gpis_fs.hpp)
    unsigned fs_ws_blocks = 0;
    gpis_fs_state *fs_slots = nullptr;   // ... followed by two banks of fs_ws_blocks states: the frame drivers' path states (gpis_fs_scene.hpp),
                                         // then the path driver's shadow copies (gpis_fs_paths.hpp)
    gpis::DevBuf<> fs_scene_recs;     // gpis_fs_render_scene_s: one record per sample of a chunk, and the chunk's work counter
    gpis::DevBuf<uint32_t> fs_scene_next;
    // staging for the *_host entries and workspace for the renderer (grown on demand)
    // slots 0-2: *_host staging; 3: renderer workspace (Lambert driver: primary rays + jitters + mask); 4: wavefront march;
    // 5, 6: the Lambert driver's segment results and its shadow-ray arrays — separate allocations, so that each can be made while
    // the kernel that does not need it yet runs (gpis_render_scene_s) or ahead of time from another thread (gpis_reserve_scene_workspace)
    static constexpr int kStageSlots = 7;
    gpis::DevBuf<> stage[kStageSlots];
    std::mutex stage_mu[kStageSlots];   // guards the growth of one slot (the reserve entry does not take `mu`)
    std::mutex mu;
    std::mutex fs_host_mu;   // serialises the function-space host entries, which own fs_stage[] end to end, and the function-space
                             // adaptive frame entries (tu_fs_adaptive.hip), which hold it over their passes and take `mu` inside
    gpis::DevBuf<> fs_stage[3];
    int batch_hint = GPIS_ORDER_COHERENT;   // gpis_set_batch_order: which form of the guided march the *_batch / *_host entries use
    // tuning options (gpis_set_option; defaults from the GPIS_* environment variables read ONCE in gpis_create)
    long long opt[GPIS_OPT_COUNT_] = {};
    // the renderer's workspace (stage[3]) and the wavefront march's (stage[4]) are shared by all callers of this
    // handle: the last user records an event, the next one makes its stream wait for it
    hipEvent_t ws_event[2] = {nullptr, nullptr};
    bool ws_event_set[2] = {false, false};
    // pipelined host path (gpis_sample_distance_host / gpis_transmittance_host): two slots, each with its own stream,
    // pinned staging and device buffers, so that chunk k's H2D copy overlaps chunk k-1's kernel and chunk k-2's D2H
    struct HostSlot {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        gpis::PinBuf pin_in, pin_out, pin_aux;       // pinned host staging (used when the caller's memory is pageable)
        gpis::DevBuf<> dev_in, dev_out, dev_aux;
        size_t cap = 0;                              // chunk capacity in records
    } hs[2];
    // persistent march (gpis_persist.inc): ring of ray counters (one per launch in flight), resident-wave budget
    gpis::DevBuf<unsigned int> d_next;
    unsigned next_slot = 0;
    int persist_waves[8] = {};    // cached occupancy * CUs per kernel instance; 0 = not queried yet
    int n_cus = 0;
    // optional per-kernel timing (gpis_set_profiling): event pairs around each march launch
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events[3];     // 0: sampleDistance, 1: transmittance, 2: the NEE driver's neePDF / neeGrad launches
    size_t events_used[3] = {0, 0, 0};
    double prof_ms[3] = {0., 0., 0.};
    uint64_t prof_launches[3] = {0, 0, 0};

    // what is not a buffer; the buffers follow as members, after the streams that used them are gone.  The caller has set the
    // device and waited for it (gpis_destroy, the failure paths of gpis_create).
    ~gpis_medium()
    {
        for (HostSlot &S : hs) {
            if (S.done) (void)hipEventDestroy(S.done);
            if (S.stream) (void)hipStreamDestroy(S.stream);
        }
        for (auto &list : events)
            for (auto &ev : list) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        for (hipEvent_t e : ws_event)
            if (e) (void)hipEventDestroy(e);
        gpis::fast_table_free(&fast);
        gpis::guide_free(&guide);
    }
};

namespace gpis {

// a weight-space handle (tu_ws.hip) is refused by every sparse-convolution / function-space entry: its first word is not abi_version
bool std_handle(const gpis_medium *m);

// ---- the handle's staging slots and the hand-over of the shared workspaces between callers on different streams
// (slot 0: stage[3], slot 1: stage[4])
int ensure_stage(gpis_medium *m, int slot, size_t bytes, bool exact = false);
size_t stage_size(gpis_medium *m, int slot);
int ws_acquire(gpis_medium *m, int slot, hipStream_t s);
int ws_release(gpis_medium *m, int slot, hipStream_t s);
// the next `bytes` of a workspace laid out from `off`: their offset; every array starts 256-byte aligned
inline size_t ws_carve(size_t &off, size_t bytes)
{
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
}

struct ProfScope {   // records an event pair around one march-kernel launch when profiling is on
    gpis_medium *m; int kind; hipStream_t s; bool on;
    ProfScope(gpis_medium *m_, int kind_, hipStream_t s_) : m(m_), kind(kind_), s(s_), on(m_->profiling)
    {
        if (!on) return;
        if (m->events_used[kind] == m->events[kind].size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            m->events[kind].emplace_back(a, b);
        }
        (void)hipEventRecord(m->events[kind][m->events_used[kind]].first, s);
    }
    ~ProfScope()
    {
        if (!on) return;
        (void)hipEventRecord(m->events[kind][m->events_used[kind]].second, s);
        m->events_used[kind]++;
    }
};

// ---- the marches.  Which form of the guided march runs: the resident kernels win on batches whose waves are already coherent
// (camera rays in pixel order: 131 vs 181 ms on C1), the wavefront on scattered rays (1.4x on the second bounce), so the
// caller's hint decides; GPIS_MARCH=wave|resident overrides it.
enum MarchHint { MARCH_COHERENT = GPIS_ORDER_COHERENT, MARCH_SCATTERED = GPIS_ORDER_SCATTERED };
bool wave_march_selected(const gpis_medium *m, int hint);
int sample_distance_impl(gpis_medium *m, size_t n, const gpis_ray_in *rays, gpis_seg_out *out, gpis_cond_coeff *coeff, const uint8_t *mask, hipStream_t s,
                         int hint = MARCH_COHERENT, bool exit_state = true);
int transmittance_impl(gpis_medium *m, size_t n, const gpis_ray_in *rays, uint8_t *visible, const uint8_t *mask, hipStream_t s, int hint = MARCH_COHERENT);
// the Lambert frame driver's compact body (gpis_scene.hpp: 32-byte records)
bool lambert_compact(const gpis_medium *m, bool guided);
int scene_sample_distance_compact(gpis_medium *m, size_t n, const SceneRay *rays, SceneHit *out, const float origin[3], hipStream_t s);
int scene_transmittance_compact(gpis_medium *m, size_t n, const SceneRay *rays, const float light[3], uint8_t *visible, hipStream_t s);
int nee_instance(const DevModel &H);      // neePDF / neeGrad: the launch::Inst of the medium

// ---- function-space comparison path (gpis_fs.hpp)
int fs_check(gpis_medium *m);
int fs_workspace(gpis_medium *m, unsigned &cap, size_t scene_rec_bytes = 0);

}   // namespace gpis
