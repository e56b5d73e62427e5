// What csrc/yuv_anonymize.hip and csrc/yuv_pack.hip (libvghvideo.so) and csrc/osd.hip with csrc/osd_rules.h (libvghosd.so) share: a frame's byte planes addressed
// in place.  A plane is a pointer, a pitch and a step on its source and on its destination side; two step-2 planes that are the bytes of one even-aligned
// 16-bit pair (the U and V views of an NV12 / NV21 plane) are read and written with one 16-bit access.  One rule, stated once: the checks of a plane and their
// messages, "a destination is exactly its source plane or overlaps no source plane", the pair test, the pair access and the copy of a plane that is out of
// place.  Generic over a plane struct with the fields src_dev, dst_dev, src_pitch, dst_pitch, src_step, dst_step (each library's public header has one); no
// public header is included and neither library's prefix is named.  Header-only and internal: every definition is inline or has internal linkage, so each library compiles its
// own copy and stays a library of its own (no shared object, no exported symbol, no link dependency).
// HOST PART: plain C++ without the HIP runtime, so that csrc/osd_rules.h includes it and the host programs under tests/ compile it under the sanitizers.
// DEVICE PART: for a source that has included the HIP runtime (csrc/companion_host.h) before this header; integer arithmetic only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace planes {

// ---- the host part ---------------------------------------------------------------------------------------------------------------------------------------------
// One plane as the kernels read it.
struct Chan {
    const uint8_t* src;
    uint8_t* dst;
    int64_t spitch, dpitch;
    int32_t sstep, dstep;
};

template <typename Plane>
inline Chan chan_of(const Plane& q) {
    return Chan{q.src_dev, q.dst_dev, q.src_pitch, q.dst_pitch, q.src_step, q.dst_step};
}

// in place: the destination is exactly the source plane
template <typename Plane>
inline bool in_place(const Plane& q) {
    return q.dst_dev == q.src_dev && q.dst_pitch == q.src_pitch && q.dst_step == q.src_step;
}

// the byte range [a, b) of a plane of pw x ph samples
inline void plane_range(const uint8_t* p, int64_t pitch, int32_t step, int64_t pw, int64_t ph, uintptr_t& a, uintptr_t& b) {
    a = (uintptr_t)p;
    b = a + (uintptr_t)((ph - 1) * pitch + (pw - 1) * step + 1);
}

// 1 / 2: plane a / b is the even, lower byte of interleaved pairs that one 16-bit access reaches; 0: handled as two planes
inline int pair_of(const void* a, const void* b, int64_t apitch, int64_t bpitch, int astep, int bstep) {
    if (astep != 2 || bstep != 2 || apitch != bpitch || (apitch & 1)) return 0;
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    if (q == p + 1 && !(p & 1)) return 1;
    if (p == q + 1 && !(q & 1)) return 2;
    return 0;
}

// The checks return NULL, or the message of the first refusal, written to the caller's msg[msg_bytes].  `who` and the plane's `label` word the message.
#define PLANES_REFUSE(cond, ...)                   \
    do {                                           \
        if (!(cond)) {                             \
            snprintf(msg, msg_bytes, __VA_ARGS__); \
            return msg;                            \
        }                                          \
    } while (0)

// one pitch ("src" or "dst") of a plane with pw samples in a row, `step` bytes apart
inline const char* check_pitch(int64_t pitch, int32_t step, int64_t pw, const char* who, const char* label, const char* side, char* msg, size_t msg_bytes) {
    PLANES_REFUSE(pitch >= (pw - 1) * step + 1 && pitch <= ((int64_t)1 << 40), "%s: plane %s: %s_pitch %lld outside %lld .. 2^40", who, label, side, (long long)pitch,
                  (long long)((pw - 1) * step + 1));
    return nullptr;
}

// one plane with pw samples in a row: its pointers, its steps (1 .. max_step, 2 or 3) and its pitches
template <typename Plane>
inline const char* check_plane(const Plane& q, int64_t pw, int max_step, const char* who, const char* label, char* msg, size_t msg_bytes) {
    PLANES_REFUSE(q.src_dev && q.dst_dev, "%s: plane %s: null plane (src_dev %p, dst_dev %p)", who, label, (const void*)q.src_dev, (void*)q.dst_dev);
    PLANES_REFUSE(q.src_step >= 1 && q.src_step <= max_step && q.dst_step >= 1 && q.dst_step <= max_step, "%s: plane %s: steps %d and %d are not %s", who, label, q.src_step, q.dst_step,
                  max_step == 2 ? "1 or 2" : "1, 2 or 3");
    if (const char* m = check_pitch(q.src_pitch, q.src_step, pw, who, label, "src", msg, msg_bytes)) return m;
    return check_pitch(q.dst_pitch, q.dst_step, pw, who, label, "dst", msg, msg_bytes);
}

// n checked planes, plane k of pw[k] x ph[k] samples: a destination plane is exactly its source plane, or overlaps no source plane
template <typename Plane>
inline const char* check_overlap(const Plane* p, int n, const int64_t* pw, const int64_t* ph, const char* who, const char* const* labels, char* msg, size_t msg_bytes) {
    for (int k = 0; k < n; ++k) {
        const Plane& q = p[k];
        if (in_place(q)) continue;
        PLANES_REFUSE(q.dst_dev != q.src_dev, "%s: plane %s: the destination starts where the source does with another pitch or step (%lld and %d, not %lld and %d): in place means exactly the source plane",
                      who, labels[k], (long long)q.dst_pitch, q.dst_step, (long long)q.src_pitch, q.src_step);
        uintptr_t d0, d1, s0, s1;
        plane_range(q.dst_dev, q.dst_pitch, q.dst_step, pw[k], ph[k], d0, d1);
        for (int m = 0; m < n; ++m) {
            plane_range(p[m].src_dev, p[m].src_pitch, p[m].src_step, pw[m], ph[m], s0, s1);
            PLANES_REFUSE(d1 <= s0 || s1 <= d0, "%s: plane %s: the destination overlaps source plane %s without being exactly its own source plane", who, labels[k], labels[m]);
        }
    }
    return nullptr;
}

// ---- the device part -------------------------------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__) && defined(HIP_INCLUDE_HIP_HIP_RUNTIME_H)
namespace {

// Sample (x, y) of the planes c[0 .. n), channel k in v[k].  pair = 0: a byte per plane.  pair = 1 / 2 (n = 2 alone): c[0] / c[1] holds the even, lower bytes
// of interleaved pairs, that pointer and the pitch are even (pair_of): one aligned 16-bit access.  C is Chan or a struct derived from it.
template <int N, typename C>
__device__ __forceinline__ void load(const C (&c)[N], int n, int x, int y, int pair, uint32_t (&v)[N]) {
    if constexpr (N >= 2) {
        if (pair) {
            const C& lo = c[pair - 1];
            const uint32_t w = *reinterpret_cast<const uint16_t*>(lo.src + (int64_t)y * lo.spitch + 2 * (int64_t)x);
            const uint32_t a = w & 255u, b = w >> 8;
            v[0] = pair == 1 ? a : b;
            v[1] = pair == 1 ? b : a;
            return;
        }
    }
    for (int k = 0; k < n; ++k) v[k] = c[k].src[(int64_t)y * c[k].spitch + (int64_t)x * c[k].sstep];
}

template <int N, typename C>
__device__ __forceinline__ void store(const C (&c)[N], int n, int x, int y, int pair, const uint32_t (&v)[N]) {
    if constexpr (N >= 2) {
        if (pair) {
            const C& lo = c[pair - 1];
            const uint32_t a = pair == 1 ? v[0] : v[1], b = pair == 1 ? v[1] : v[0];
            *reinterpret_cast<uint16_t*>(lo.dst + (int64_t)y * lo.dpitch + 2 * (int64_t)x) = (uint16_t)(a | b << 8);
            return;
        }
    }
    for (int k = 0; k < n; ++k) c[k].dst[(int64_t)y * c[k].dpitch + (int64_t)x * c[k].dstep] = (uint8_t)v[k];
}

// A plane that is out of place: every sample copied, four of a row per lane; one aligned dword where both sides are dense, aligned and whole.
// Grid: ((W + 1023) / 1024, rows), 256 lanes.
__global__ __launch_bounds__(256) void copy_kernel(const uint8_t* __restrict__ src, int64_t spitch, int sstep, uint8_t* __restrict__ dst, int64_t dpitch, int dstep, int W) {
    const int x0 = (int)(blockIdx.x * 256u + threadIdx.x) * 4, y = (int)blockIdx.y;
    if (x0 >= W) return;
    const uint8_t* s = src + (int64_t)y * spitch + (int64_t)x0 * sstep;
    uint8_t* d = dst + (int64_t)y * dpitch + (int64_t)x0 * dstep;
    if (sstep == 1 && dstep == 1 && x0 + 4 <= W && (((uintptr_t)s | (uintptr_t)d) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
        return;
    }
    for (int b = 0; b < 4 && x0 + b < W; ++b) d[(int64_t)b * dstep] = s[(int64_t)b * sstep];
}

}  // namespace
#endif

}  // namespace planes
