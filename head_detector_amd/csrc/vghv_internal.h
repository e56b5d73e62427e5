// What the sources of libvghview.so share (csrc/aligned.hip, csrc/draw.hip, csrc/mesh_render.hip): the calling thread's error message and, for
// aligned.hip and draw.hip, the argument / HIP check macros of the C entry points and the per-device staging block (pinned + device memory,
// guarded by an event); mesh_render.hip takes those from csrc/tile_fold.h and only the message from here.  Internal: hidden visibility,
// nothing of libvgh.so (csrc/vgh_internal.h) is used here and libvgh.so uses nothing of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vgh_view.h"

namespace vghv {

// ---- error plumbing: never throw across the C ABI (defined in aligned.hip) -----------------------------------------------------------
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();

#define VGHV_HIP(expr)                                                                              \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            vghv::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
            return VGHV_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)

#define VGHV_REQUIRE(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            vghv::set_error(__VA_ARGS__);  \
            return VGHV_ERR_INVALID;       \
        }                                  \
    } while (0)

// ---- staging: what one call uploads, one pinned block and one device block per device, grown on demand ----------------------------------
// A block is rewritten only after the previous call's copy and kernels have run (the event), whatever stream they were queued on.
struct Staging {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// waits for the block's previous user, then makes room for `need` bytes (defined in aligned.hip); `who` names the caller in the message
int staging_reserve(Staging& s, size_t need, const char* who);

}  // namespace vghv
