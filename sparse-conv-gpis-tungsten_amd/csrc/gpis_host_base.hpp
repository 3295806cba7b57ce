// gpis_host_base.hpp — what the host side of both handle families stands on (gpis_host.hpp: sparse-convolution / function-space;
// gpis_ws_host.hpp: weight-space): the one error layer, the owning device and pinned buffers, and the round trip of a
// host-pointer entry over its device-pointer entry.  Host code only: no device function, no kernel launch.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <mutex>

#include "gpis.h"

namespace gpis {

// ---- errors: the library's thread-local text (gpis_last_error; defined in gpis_hip.hip, cut at 511 characters); returns `code`
int set_err(int code, const char *fmt, ...);
int launch_check(const char *what);

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

// ---- a device allocation and its size in bytes, freed with its owner.  grow() makes no call when the block is large enough,
// else frees it and allocates `want` bytes (slack: 25 % + 4096 more, for staging that follows a batch size).  Whatever must
// happen before the old block goes (a synchronise) is the caller's, in front of grow().
template <typename T = void>
struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    T *release() { T *q = p; p = nullptr; bytes = 0; return q; }      // the allocation goes on to another owner ...
    void adopt(T *q, size_t n) { reset(); p = q; bytes = n; }         // ... which frees what it held
    hipError_t grow(size_t want, bool slack = false)
    {
        if (bytes >= want) return hipSuccess;
        reset();
        const size_t cap = slack ? want + want / 4 + 4096 : want;
        const hipError_t e = hipMalloc((void **)&p, cap);
        if (e == hipSuccess) bytes = cap; else p = nullptr;
        return e;
    }
};
// ... and the same over pinned host memory
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { reset(); }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
    hipError_t grow(size_t want)
    {
        if (bytes >= want) return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) bytes = want; else p = nullptr;
        return e;
    }
};

// ---- one array of a host-pointer entry: `bytes` at offset `off` of staging slot `slot` (0..2), copied in from `in` before the
// call and back to `out` after it; either may be null (an output nobody asked for still has its room)
struct HostArray { const void *in; void *out; size_t bytes; int slot; size_t off = 0; };
enum { kTripNoSync = 1, kTripKeepUnsupported = 2 };

// staging slots that the caller's own lock covers (function-space host staging, weight-space handle): grown with slack
struct GrowStage {
    DevBuf<> *stage;
    int operator()(int slot, size_t bytes) const { HIP_TRY(stage[slot].grow(bytes, true)); return GPIS_OK; }
};

// The round trip: lock `mu`, set the device, grow the slots the arrays name (`grow(slot, bytes)`: GrowStage, or the handle's
// ensure_stage where a slot has a lock of its own), copy the inputs in, `call` the device-pointer entry on the slots, stop on its
// error, synchronise the device, copy the outputs back.  kTripNoSync: the call has drained its stream itself;
// kTripKeepUnsupported: GPIS_ERR_UNSUPPORTED from the call still copies back and is returned after that.
template <typename Grow, typename Call>
inline int host_round_trip(std::mutex &mu, int device, DevBuf<> *stage, Grow grow, std::initializer_list<HostArray> arrays, Call call, int flags = 0)
{
    std::lock_guard<std::mutex> lock(mu);
    HIP_TRY(hipSetDevice(device));
    size_t need[3] = {0, 0, 0};
    for (const HostArray &a : arrays)
        if (need[a.slot] < a.off + a.bytes) need[a.slot] = a.off + a.bytes;
    for (int k = 0; k < 3; ++k)
        if (need[k])
            if (int st = grow(k, need[k])) return st;
    for (const HostArray &a : arrays)
        if (a.in) HIP_TRY(hipMemcpy((char *)stage[a.slot].p + a.off, a.in, a.bytes, hipMemcpyHostToDevice));
    const int st = call();
    if (st && !((flags & kTripKeepUnsupported) && st == GPIS_ERR_UNSUPPORTED)) return st;
    if (!(flags & kTripNoSync)) HIP_TRY(hipDeviceSynchronize());
    for (const HostArray &a : arrays)
        if (a.out) HIP_TRY(hipMemcpy(a.out, (char *)stage[a.slot].p + a.off, a.bytes, hipMemcpyDeviceToHost));
    return st;
}

}   // namespace gpis
