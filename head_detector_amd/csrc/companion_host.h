// The host plumbing of the six companion libraries (libvghview.so: csrc/aligned.hip, csrc/draw.hip, csrc/mesh_render.hip; libvghvis.so: csrc/visibility.hip;
// libvghtex.so: csrc/texture.hip; libvgheval.so: csrc/mesh_metrics.hip, csrc/detection_ap.hip; libvghmerge.so: csrc/slice_merge.hip; libvghtrack.so: csrc/head_track.hip)
// and of the application library libvghanon.so (csrc/anonymize.hip): the return codes, the calling thread's error message, the check / require macros of
// the C entry points, the per-device staging block and the queue-then-record discipline around it.  Host-only, header-only and internal: everything is
// inline, and the companions are built with -fvisibility=hidden, so the sources of one library share one message and no library exports any of this or
// sees another's.  Nothing of libvgh.so (csrc/vgh_internal.h) is used here and libvgh.so uses nothing of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace companion {

// ---- error plumbing: never throw across the C ABI -------------------------------------------------------------------------------------------------
// The codes of the six public headers are the same numbers; every includer static_asserts its own against these.
constexpr int OK = 0, ERR_INVALID = -1, ERR_HIP = -2, ERR_NOMEM = -3;

inline thread_local char g_error[512] = "";  // one per thread and library: an inline variable is one object across the sources of a shared object

inline void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

inline const char* last_error() { return g_error; }

// check: a HIP call that must succeed before anything is queued
#define CH_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            companion::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return companion::ERR_HIP;                                                                 \
        }                                                                                              \
    } while (0)

// require: an argument check
#define CH_REQUIRE(cond, ...)                  \
    do {                                       \
        if (!(cond)) {                         \
            companion::set_error(__VA_ARGS__); \
            return companion::ERR_INVALID;     \
        }                                      \
    } while (0)

// queue-then-record: from the staging copy on, the first failure is kept and nothing more is queued after it (CH_QUEUE; launches ask q.ok()), and
// finish() records the event on every path, so that the next call never rewrites the staging block or the library's scratch under work that is still
// queued.
struct Queue {
    hipError_t err = hipSuccess;
    const char* failed = "";
    bool ok() const { return err == hipSuccess; }
};
#define CH_QUEUE(q, expr)                      \
    do {                                       \
        if ((q).ok()) {                        \
            (q).err = (expr);                  \
            if (!(q).ok()) (q).failed = #expr; \
        }                                      \
    } while (0)

// ---- staging: what one call uploads, one pinned block and one device block per device, grown on demand --------------------------------------------
// A block is rewritten only after the previous call's copy and kernels have run (the event), whatever stream they were queued on.
struct Staging {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// waits for the block's previous user, then makes room for `need` bytes; `who` names the caller in the message
inline int reserve(Staging& s, size_t need, const char* who) {
    if (s.recorded) CH_HIP(hipEventSynchronize(s.ev));
    s.recorded = false;
    if (!s.ev) CH_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (need <= s.bytes) return OK;
    hipHostFree(s.host);
    hipFree(s.dev);
    s.host = s.dev = nullptr;
    s.bytes = 0;
    const size_t cap = align16(need + need / 2);
    if (hipHostMalloc((void**)&s.host, cap, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s.dev, cap) != hipSuccess) {
        hipHostFree(s.host);
        s.host = nullptr;
        set_error("%s: allocating %zu bytes of staging failed", who, cap);
        return ERR_NOMEM;
    }
    s.bytes = cap;
    return OK;
}

// Library scratch on the device that the staging block's event guards as well (the rasterisers' triangle boxes, draw's key plane), grown on demand.
// grow() comes after reserve(): nothing is using the old block, the wait there covered the previous call's kernels.  false = out of memory, the block is
// then empty and the caller words the message.
template <typename T>
struct Scratch {
    T* ptr = nullptr;
    size_t bytes = 0;
};

template <typename T>
inline bool grow(Scratch<T>& s, size_t need) {
    if (need <= s.bytes) return true;
    hipFree(s.ptr);
    s.ptr = nullptr;
    s.bytes = 0;
    if (hipMalloc((void**)&s.ptr, need) != hipSuccess) return false;
    s.bytes = need;
    return true;
}

// The end of queue-then-record.  `guarded`: the call queued work that reads the staging block or the scratch, so the event has to cover it; if it
// cannot be recorded the stream is waited for instead.  Returns the call's code and words the first failure as "<who>: <call> -> <HIP's message>".
inline int finish(Queue& q, Staging& s, bool guarded, hipStream_t st, const char* who) {
    CH_QUEUE(q, hipGetLastError());
    if (guarded) {
        if (hipEventRecord(s.ev, st) == hipSuccess) {
            s.recorded = true;
        } else {
            hipStreamSynchronize(st);  // no event to wait for next time: wait now
            CH_QUEUE(q, hipErrorUnknown);
        }
    }
    if (q.ok()) return OK;
    set_error("%s: %s -> %s", who, q.failed, hipGetErrorString(q.err));
    return ERR_HIP;
}

}  // namespace companion
