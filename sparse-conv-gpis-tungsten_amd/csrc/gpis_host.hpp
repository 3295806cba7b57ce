// gpis_host.hpp — host side of a sparse-convolution / function-space handle, shared by the translation units that implement its
// entries (gpis_hip.hip: model build, handle, batch and *_host entries; tu_scene.hip: the staged scene-S frame drivers).  The
// weight-space medium's counterpart is gpis_ws_host.hpp.
//
// The helpers declared here are defined in gpis_hip.hip; the error text (g_err, gpis_last_error) lives there too.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "gpis.h"
#include "gpis_device.hpp"
#include "gpis_scene.hpp"     // SceneRay, SceneHit
#include "gpis_tables.hpp"    // FastTable, GuideField: the records only, none of the fast or guided device code

// ======================================================================================
// handle
// ======================================================================================
struct gpis_medium {
    gpis_params params;
    gpis::DevModel host_model;
    gpis_derived derived;
    int device;
    gpis::DevModel *d_model;
    gpis::Counters *d_counters;
    gpis::FastTable fast;    // single-realization wave-cooperative path (gpis_tables.hpp, gpis_fast.hpp); enabled == 0 when unused
    gpis::GuideField guide;  // certified guide field (gpis_tables.hpp, gpis_guide.hpp); enabled == 0 until gpis_build_guide
    unsigned long long *d_guide_cnt;
    uint64_t selfcheck_tabulated = 0;   // points of the last gpis_guide_selfcheck that fell into tabulated bricks
    gpis::GuideField *d_guide;   // device copy of `guide` (the resident guided kernels read it through scalar loads instead of 14 kernel-argument SGPRs)
    float *d_grid_vox = nullptr;      // GridNonstationaryCovariance voxels (gpis_set_variance_grid)
    float *d_mean_vox[2] = {nullptr, nullptr};   // TabulatedMean voxels of the two mean slots (gpis_set_mean_grid)
    unsigned lambert_calls = 0;       // gpis_render_scene_s calls so far (the first one works in small chunks, see lambert_ws_plan)
    void *fs_ws = nullptr;            // function-space workspace: one FsGlob per resident workgroup (gpis_fs.hpp)
    unsigned fs_ws_blocks = 0;
    gpis_fs_state *fs_slots = nullptr;   // ... followed by two banks of fs_ws_blocks states: the frame drivers' path states (gpis_fs_scene.hpp),
                                         // then the path driver's shadow copies (gpis_fs_paths.hpp)
    void *fs_scene_recs = nullptr;    // gpis_fs_render_scene_s: one record per sample of a chunk, and the chunk's work counter
    size_t fs_scene_rec_bytes = 0;
    uint32_t *fs_scene_next = nullptr;
    // staging for the *_host entries and workspace for the renderer (grown on demand)
    // slots 0-2: *_host staging; 3: renderer workspace (Lambert driver: primary rays + jitters + mask); 4: wavefront march;
    // 5, 6: the Lambert driver's segment results and its shadow-ray arrays — separate allocations, so that each can be made while
    // the kernel that does not need it yet runs (gpis_render_scene_s) or ahead of time from another thread (gpis_reserve_scene_workspace)
    static constexpr int kStageSlots = 7;
    void *stage[kStageSlots];
    size_t stage_bytes[kStageSlots];
    std::mutex stage_mu[kStageSlots];   // guards the growth of one slot (the reserve entry does not take `mu`)
    std::mutex mu;
    std::mutex fs_host_mu;   // serialises the function-space host entries, which own fs_stage[] end to end
    void *fs_stage[3] = {nullptr, nullptr, nullptr};
    size_t fs_stage_bytes[3] = {0, 0, 0};
    // optional per-kernel timing (gpis_set_profiling): event pairs around each march launch
    int batch_hint;          // gpis_set_batch_order: which form of the guided march the *_batch / *_host entries use
    // tuning options (gpis_set_option; defaults from the GPIS_* environment variables read ONCE in gpis_create)
    long long opt[GPIS_OPT_COUNT_];
    // the renderer's workspace (stage[3]) and the wavefront march's (stage[4]) are shared by all callers of this
    // handle: the last user records an event, the next one makes its stream wait for it
    hipEvent_t ws_event[2];
    bool ws_event_set[2];
    // persistent march (gpis_persist.inc): ring of ray counters (one per launch in flight), resident-wave budget
    // pipelined host path (gpis_sample_distance_host / gpis_transmittance_host): two slots, each with its own stream,
    // pinned staging and device buffers, so that chunk k's H2D copy overlaps chunk k-1's kernel and chunk k-2's D2H
    struct HostSlot {
        hipStream_t stream;
        hipEvent_t done;
        char *pin_in, *pin_out, *pin_aux;       // pinned host staging (used when the caller's memory is pageable)
        char *dev_in, *dev_out, *dev_aux;
        size_t cap;                             // chunk capacity in records
    } hs[2];
    unsigned int *d_next;
    unsigned next_slot;
    int persist_waves[8];    // cached occupancy * CUs per kernel instance; 0 = not queried yet
    int n_cus;
    bool profiling;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events[3];     // 0: sampleDistance, 1: transmittance, 2: the NEE driver's neePDF / neeGrad launches
    size_t events_used[3];
    double prof_ms[3];
    uint64_t prof_launches[3];
};

namespace gpis {

// ======================================================================================
// errors
// ======================================================================================
int set_err(int code, const char *fmt, ...);      // the library's thread-local error text (gpis_last_error); returns `code`

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(GPIS_ERR_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define CHECK_ARGS(cond)                                                        \
    do {                                                                        \
        if (!(cond)) return set_err(GPIS_ERR_INVALID_ARG, "%s: invalid argument (%s)", __func__, #cond); \
    } while (0)

// a weight-space handle (tu_ws.hip) is refused by every sparse-convolution / function-space entry: its first word is not abi_version
bool std_handle(const gpis_medium *m);
int launch_check(const char *what);

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
