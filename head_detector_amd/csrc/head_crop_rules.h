// What the host half and the kernel of csrc/head_tensors.hip (libvghcrop.so, include/vgh_crop.h) must not hold twice: the limits, the integer functions of the
// rule (sub-sample position, source pixel and fractions, the four-tap value, the YUV tap, the uint8 rounding), the validation of a job and the tile count.
// HIP-free: plain C++ that tests/head_crop_host.hip compiles for the host alone under the sanitizers; under hipcc the functions are host and device functions.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vgh_crop.h"

#if defined(__HIPCC__)
#define HEAD_CROP_HD __host__ __device__ inline
#else
#define HEAD_CROP_HD inline
#endif

namespace head_crop {

constexpr int kTile = 16;      // a block computes a 16 x 16 tile of one head's crop, one output pixel per lane
constexpr int kFracBits = 5;   // fractions of a source pixel
constexpr int kWeightSum = (1 << kFracBits) * (1 << kFracBits);  // 1024
constexpr int64_t kPosLimit = (int64_t)1 << 62;
constexpr int32_t kMaxCoef = 1 << 20;  // |YUV coefficient|

// sum <= 255 * 1024 * K^2 must be exactly a float32: this is why K stops at 8 and the fractions have 5 bits
static_assert(255ll * kWeightSum * VGHC_MAX_SUPERSAMPLE * VGHC_MAX_SUPERSAMPLE < (1ll << 24), "every sum is exactly a float32");
static_assert(255ll * kWeightSum * (VGHC_MAX_SUPERSAMPLE + 1) * (VGHC_MAX_SUPERSAMPLE + 1) >= (1ll << 24), "K = 8 is the largest factor with that property");
static_assert((int64_t)VGHC_MAX_HEADS * ((VGHC_MAX_SIZE + kTile - 1) / kTile) * ((VGHC_MAX_SIZE + kTile - 1) / kTile) < (1ll << 31), "the unchecked tile count fits int32");

// ---- the rule ------------------------------------------------------------------------------------------------------------------------------------------------
// position of sub-sample (p, q) along one axis, Q32: validate() bounds |c0| + S K (|cp| + |cq|) below 2^62, so nothing here overflows
HEAD_CROP_HD int64_t sub_position(int64_t c0, int64_t cp, int64_t cq, int32_t p, int32_t q) { return c0 + (int64_t)p * cp + (int64_t)q * cq; }

HEAD_CROP_HD int32_t source_pixel(int64_t pos) { return (int32_t)(pos >> 32); }  // flooring; |pos| < 2^62, so it fits

HEAD_CROP_HD int32_t fraction(int64_t pos) { return (int32_t)(pos >> (32 - kFracBits)) & ((1 << kFracBits) - 1); }

// the four weights sum to 1024; <= 255 * 1024
HEAD_CROP_HD int32_t tap4(int32_t fx, int32_t fy, int32_t t00, int32_t t01, int32_t t10, int32_t t11) {
    return (32 - fx) * (32 - fy) * t00 + fx * (32 - fy) * t01 + (32 - fx) * fy * t10 + fx * fy * t11;
}

HEAD_CROP_HD int32_t clamp8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one YUV sample as channel c (0 R, 1 G, 2 B) of its RGB pixel: the integer rule of include/vgh.h, clamped to a byte
HEAD_CROP_HD int32_t yuv_channel(const vghc_source& s, int32_t Y, int32_t U, int32_t V, int c) {
    const int32_t luma = s.cy * (Y - s.y_offset) + 32768, d = U - 128, e = V - 128;
    return clamp8((c == 0 ? luma + s.crv * e : c == 1 ? luma + s.cgu * d + s.cgv * e : luma + s.cbu * d) >> 16);
}

// the mean of K^2 sub-samples as a byte, rounded half up
HEAD_CROP_HD int32_t round_u8(int32_t sum, int32_t K) {
    const int32_t d = kWeightSum * K * K;
    return (2 * sum + d) / (2 * d);
}

// ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------------
inline int element_bytes(int dtype) { return dtype == VGHC_DTYPE_U8 ? 1 : dtype == VGHC_DTYPE_F32 ? 4 : 2; }

inline int tiles_per_side(int S) { return (S + kTile - 1) / kTile; }

inline int64_t tile_count(int n_heads, int S) { return (int64_t)n_heads * tiles_per_side(S) * tiles_per_side(S); }

// ---- validation ----------------------------------------------------------------------------------------------------------------------------------------------
inline uint64_t magnitude(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }

// |c0| + m (|cp| + |cq|) < 2^62, in unsigned arithmetic that cannot wrap
inline bool positions_fit(int64_t c0, int64_t cp, int64_t cq, int64_t m) {
    const uint64_t limit = (uint64_t)kPosLimit, a0 = magnitude(c0), ap = magnitude(cp), aq = magnitude(cq), um = (uint64_t)m;
    if (a0 >= limit || ap > limit / um || aq > limit / um) return false;
    return a0 + um * (ap + aq) < limit;  // <= 2^62 + 2 * 2^62: no wrap
}

inline bool is_finite(float v) { return v - v == 0.0f; }

#define HEAD_CROP_REFUSE(cond, ...)             \
    do {                                        \
        if (!(cond)) {                          \
            snprintf(msg, msg_bytes, __VA_ARGS__); \
            return msg;                         \
        }                                       \
    } while (0)

// NULL for a job vghc_head_tensors takes, otherwise the message of its first refusal (written to msg).  Reads host memory only.
inline const char* validate(const vghc_job* job, char* msg, size_t msg_bytes) {
    HEAD_CROP_REFUSE(job, "head_tensors: null job");
    const vghc_job& j = *job;
    HEAD_CROP_REFUSE(j.size >= 1 && j.size <= VGHC_MAX_SIZE, "head_tensors: size %d outside 1 .. %d", j.size, VGHC_MAX_SIZE);
    HEAD_CROP_REFUSE(j.n_heads >= 0 && j.n_heads <= VGHC_MAX_HEADS, "head_tensors: n_heads %d outside 0 .. %d", j.n_heads, VGHC_MAX_HEADS);
    HEAD_CROP_REFUSE(j.n_sources >= 0, "head_tensors: n_sources %d", j.n_sources);
    HEAD_CROP_REFUSE(j.dtype >= VGHC_DTYPE_U8 && j.dtype <= VGHC_DTYPE_BF16, "head_tensors: unknown dtype %d", j.dtype);
    HEAD_CROP_REFUSE(j.layout == VGHC_LAYOUT_NCHW || j.layout == VGHC_LAYOUT_NHWC, "head_tensors: unknown layout %d", j.layout);
    HEAD_CROP_REFUSE(j.channel_order == VGHC_ORDER_RGB || j.channel_order == VGHC_ORDER_BGR, "head_tensors: unknown channel order %d", j.channel_order);
    HEAD_CROP_REFUSE(j.fill >= 0 && j.fill < (1 << 24), "head_tensors: fill %d is not three bytes", j.fill);
    HEAD_CROP_REFUSE(j.dst_bytes >= 0, "head_tensors: dst_bytes %lld", (long long)j.dst_bytes);
    for (int c = 0; c < 3; ++c) HEAD_CROP_REFUSE(is_finite(j.b[c]), "head_tensors: b[%d] is not finite", c);
    if (j.n_heads == 0) return nullptr;
    HEAD_CROP_REFUSE(j.sources && j.n_sources >= 1, "head_tensors: null sources");
    HEAD_CROP_REFUSE(j.heads, "head_tensors: null heads");
    HEAD_CROP_REFUSE(j.dst_dev, "head_tensors: null dst_dev");
    const int eb = element_bytes(j.dtype);
    HEAD_CROP_REFUSE((uintptr_t)j.dst_dev % (uintptr_t)eb == 0, "head_tensors: dst_dev is not aligned to its %d-byte elements", eb);
    const int64_t need = (int64_t)j.n_heads * 3 * j.size * j.size * eb;  // <= 2^16 * 3 * 2^20 * 4 < 2^40
    HEAD_CROP_REFUSE(need <= j.dst_bytes, "head_tensors: the result of %d heads needs %lld bytes, the destination has %lld", j.n_heads, (long long)need, (long long)j.dst_bytes);
    HEAD_CROP_REFUSE(tile_count(j.n_heads, j.size) <= VGHC_MAX_TILES, "head_tensors: %lld tiles exceed one launch (%d)", (long long)tile_count(j.n_heads, j.size), VGHC_MAX_TILES);
    for (int i = 0; i < j.n_sources; ++i) {
        const vghc_source& s = j.sources[i];
        HEAD_CROP_REFUSE(s.kind == VGHC_SOURCE_RGB || s.kind == VGHC_SOURCE_YUV420, "head_tensors: source %d: unknown kind %d", i, s.kind);
        HEAD_CROP_REFUSE(s.h >= 1 && s.w >= 1 && s.h <= VGHC_MAX_SIDE && s.w <= VGHC_MAX_SIDE, "head_tensors: source %d: %d x %d outside 1 .. %d", i, s.h, s.w, VGHC_MAX_SIDE);
        if (s.kind == VGHC_SOURCE_RGB) {
            HEAD_CROP_REFUSE(s.rgb_dev, "head_tensors: source %d: null rgb_dev", i);
            HEAD_CROP_REFUSE(s.rgb_pitch_bytes >= (int64_t)s.w * 3, "head_tensors: source %d: rgb_pitch_bytes %lld < w * 3 = %lld", i, (long long)s.rgb_pitch_bytes, (long long)s.w * 3);
        } else {
            HEAD_CROP_REFUSE(s.y_dev && s.u_dev && s.v_dev, "head_tensors: source %d: null plane", i);
            HEAD_CROP_REFUSE(s.chroma_step == 1 || s.chroma_step == 2, "head_tensors: source %d: chroma_step %d (1 = planar, 2 = interleaved)", i, s.chroma_step);
            HEAD_CROP_REFUSE(s.y_pitch_bytes >= s.w, "head_tensors: source %d: y_pitch_bytes %lld < w = %d", i, (long long)s.y_pitch_bytes, s.w);
            const int64_t row = (int64_t)s.chroma_step * ((s.w + 1) / 2);
            HEAD_CROP_REFUSE(s.uv_pitch_bytes >= row, "head_tensors: source %d: uv_pitch_bytes %lld < chroma_step * ((w + 1) / 2) = %lld", i, (long long)s.uv_pitch_bytes, (long long)row);
            HEAD_CROP_REFUSE(s.y_offset >= 0 && s.y_offset <= 255, "head_tensors: source %d: y_offset %d outside 0 .. 255", i, s.y_offset);
            const int32_t coef[5] = {s.cy, s.crv, s.cgu, s.cgv, s.cbu};
            for (int c = 0; c < 5; ++c)
                HEAD_CROP_REFUSE(coef[c] >= -kMaxCoef && coef[c] <= kMaxCoef, "head_tensors: source %d: coefficient %d outside +-2^20", i, coef[c]);
        }
    }
    for (int i = 0; i < j.n_heads; ++i) {
        const vghc_head& h = j.heads[i];
        HEAD_CROP_REFUSE(h.source >= 0 && h.source < j.n_sources, "head_tensors: head %d: source %d outside the %d supplied", i, h.source, j.n_sources);
        HEAD_CROP_REFUSE(h.supersample >= 1 && h.supersample <= VGHC_MAX_SUPERSAMPLE, "head_tensors: head %d: supersample %d outside 1 .. %d", i, h.supersample, VGHC_MAX_SUPERSAMPLE);
        HEAD_CROP_REFUSE(h.reserved == 0, "head_tensors: head %d: reserved is %d", i, h.reserved);
        for (int c = 0; c < 3; ++c) HEAD_CROP_REFUSE(is_finite(h.a[c]), "head_tensors: head %d: a[%d] is not finite", i, c);
        const int64_t m = (int64_t)j.size * h.supersample;
        HEAD_CROP_REFUSE(positions_fit(h.x0, h.xp, h.xq, m), "head_tensors: head %d: |x0| + S K (|xp| + |xq|) reaches 2^62", i);
        HEAD_CROP_REFUSE(positions_fit(h.y0, h.yp, h.yq, m), "head_tensors: head %d: |y0| + S K (|yp| + |yq|) reaches 2^62", i);
    }
    return nullptr;
}

}  // namespace head_crop
