// libvghview.so (include/vgh_view.h): PredictionResult.draw (head_detector/detection_result.py:45-51, head_detector/draw_utils.py) without the
// reference's Python loop of 4 816 cv2.polylines and 2 470 cv2.circle calls per head.
//
// Painter's order without serialising the primitives: all primitives of one (head, class) share a colour, so the order of a pixel is decided by
//   key = 1 + NUM_CLASSES * head + class
// STAMP: every primitive does atomicMax(key) on the pixels it covers in a u32 plane [H, W] that was cleared to 0 (the technique of csrc/raster.hip).
// RESOLVE: every pixel writes colour[(key - 1) % NUM_CLASSES] if its key is non-zero, else the source pixel.
// The primitives are expanded on the device from one upload per call (points, boxes, topology, circle table); one launch per class plus the
// clear and the resolve, whatever the number of heads.  A further class (say, pose arrows) is one more enumerator, colour and stamp kernel.
//
// The pixel sets are OpenCV 4.x's (drawing.cpp: rectangle of thickness 2, clipLine + the thickness-1 Line walk, FillCircle) as restated in
// tests/draw_ref.py.  PARITY UNPINNED against cv2 itself (absent where this was written); bit-exact against tests/draw_ref.py.
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_view.h"
#include "companion_host.h"

namespace {

using namespace companion;
static_assert(VGHV_OK == OK && VGHV_ERR_INVALID == ERR_INVALID && VGHV_ERR_HIP == ERR_HIP && VGHV_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

enum DrawClass : uint32_t { CLASS_BOX = 0, CLASS_WIRE = 1, CLASS_DOTS = 2, NUM_CLASSES = 3 };  // in the order one head's classes are painted

// colour of a class as the bytes of channels 0, 1, 2 (little-endian in a u32)
__device__ __forceinline__ uint32_t class_colour(uint32_t cls) {
    return cls == CLASS_BOX ? 0x0000ffu /* (255, 0, 0) */ : cls == CLASS_WIRE ? 0xff0000u /* (0, 0, 255) */ : 0xffffffu /* (255, 255, 255) */;
}

__device__ __forceinline__ uint32_t order_key(int head, DrawClass cls) { return 1u + (uint32_t)NUM_CLASSES * (uint32_t)head + (uint32_t)cls; }

// every stamp goes through here: a pixel outside the plane is never touched, whatever the arithmetic before it did
__device__ __forceinline__ void stamp(uint32_t* keys, int W, int H, int x, int y, uint32_t key) {
    if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) atomicMax(keys + (size_t)y * W + x, key);
}

// ---- class 0: boxes ---------------------------------------------------------------------------------------------------------------------
// blockIdx.x = head * 4 + band, blockIdx.y * 256 + threadIdx.x = position along the band (clipped to the image first: no lane walks a band).
// Bands 0, 1: rows y - 1 .. y + 1 and y2 - 1 .. y2 + 1 over columns x .. x2; bands 2, 3: columns x - 1 .. x + 1 and x2 - 1 .. x2 + 1 over rows y .. y2.
__global__ __launch_bounds__(256) void stamp_boxes_kernel(const int32_t* __restrict__ boxes, uint32_t* __restrict__ keys, int W, int H) {
    const int head = blockIdx.x >> 2, band = blockIdx.x & 3;
    const int x = boxes[4 * head], y = boxes[4 * head + 1], x2 = x + boxes[4 * head + 2], y2 = y + boxes[4 * head + 3];
    const int t = blockIdx.y * 256 + threadIdx.x;
    const uint32_t key = order_key(head, CLASS_BOX);
    if (band < 2) {
        const int col = max(x, 0) + t, row = band == 0 ? y : y2;
        if (col > min(x2, W - 1)) return;
        for (int o = -1; o <= 1; ++o) stamp(keys, W, H, col, row + o, key);
    } else {
        const int row = max(y, 0) + t, col = band == 2 ? x : x2;
        if (row > min(y2, H - 1)) return;
        for (int o = -1; o <= 1; ++o) stamp(keys, W, H, col + o, row, key);
    }
}

// ---- class 1: wire ------------------------------------------------------------------------------------------------------------------------
// One clipped, oriented segment: start pixel, extents along the major (D) and minor (d) axis, direction of y, which axis is the major one.
struct Seg {
    int x, y, D, d, sy, y_major;
    int count;  // D + 1 pixels, 0 = not drawn
};

// trunc(double(a) * b / c): one double product, one double division, truncation toward zero (the order is part of the rule)
__device__ __forceinline__ int trunc_div(int a, int b, int c) { return (int)((double)a * (double)b / (double)c); }

// OpenCV's clipLine to [0, W-1] x [0, H-1] (the endpoints move) and the orientation of the walk (left to right)
__device__ Seg clip_and_orient(int x1, int y1, int x2, int y2, int W, int H) {
    const int right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + 2 * (x1 > right) + 4 * (y1 < 0) + 8 * (y1 > bottom);
    int c2 = (x2 < 0) + 2 * (x2 > right) + 4 * (y2 < 0) + 8 * (y2 > bottom);
    Seg s = {0, 0, 0, 0, 1, 0, 0};
    if (c1 & c2) return s;
    if (c1 | c2) {
        if (c1 & 12) {
            const int a = c1 < 8 ? 0 : bottom;
            x1 += trunc_div(a - y1, x2 - x1, y2 - y1);
            y1 = a;
            c1 = (x1 < 0) + 2 * (x1 > right);
        }
        if (c2 & 12) {
            const int a = c2 < 8 ? 0 : bottom;
            x2 += trunc_div(a - y2, x1 - x2, y1 - y2);
            y2 = a;
            c2 = (x2 < 0) + 2 * (x2 > right);
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const int a = c1 == 1 ? 0 : right;
                y1 += trunc_div(a - x1, y2 - y1, x2 - x1);
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const int a = c2 == 1 ? 0 : right;
                y2 += trunc_div(a - x2, y1 - y2, x1 - x2);
                x2 = a;
                c2 = 0;
            }
        }
        if (c1 | c2) return s;
    }
    int dx = x2 - x1, dy = y2 - y1;
    s.x = x1;
    s.y = y1;
    if (dx < 0) {
        dx = -dx;
        dy = -dy;
        s.x = x2;
        s.y = y2;
    }
    s.sy = dy < 0 ? -1 : 1;
    dy = abs(dy);
    s.y_major = dy > dx;
    s.D = s.y_major ? dy : dx;
    s.d = s.y_major ? dx : dy;
    s.count = s.D + 1;
    return s;
}

constexpr int WIRE_SHORT = 24;  // segments of up to this many pixels are walked by their own lane, longer ones by the whole wave

// One segment per lane: P[c] -> P[a], P[a] -> P[b], P[b] -> P[c] of every triangle of every head (cv2.polylines, closed).  Ordinary heads have
// segments of a few pixels: each lane walks its own (Bresenham as written).  A head that fills the image, or a mesh with long edges, has
// segments of hundreds of pixels: those are painted by all 64 lanes of the wave, lane i taking pixels i, i + 64, ... by the closed form
// (after k major steps the minor offset is (2 k d + D - 1) / (2 D)), so that no lane walks a long line alone.
__global__ __launch_bounds__(256) void stamp_wire_kernel(const int32_t* __restrict__ points, const int32_t* __restrict__ triangles, uint32_t* __restrict__ keys, int n_segments,
                                                         int V, int T, int W, int H) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    Seg seg = {0, 0, 0, 0, 1, 0, 0};
    uint32_t key = 0;
    if (s < n_segments) {
        const int head = s / (3 * T), r = s - head * 3 * T, tri = r / 3, e = r - tri * 3;
        const int32_t* t = triangles + 3 * tri;
        const int from = t[e == 0 ? 2 : e - 1], to = t[e];
        const int32_t* p = points + (size_t)head * V * 2;
        seg = clip_and_orient(p[2 * from], p[2 * from + 1], p[2 * to], p[2 * to + 1], W, H);
        key = order_key(head, CLASS_WIRE);
    }
    if (seg.count > 0 && seg.count <= WIRE_SHORT) {
        int x = seg.x, y = seg.y, err = seg.D - 2 * seg.d;
        for (int k = 0; k < seg.count; ++k) {
            stamp(keys, W, H, x, y, key);
            if (err < 0) {
                if (seg.y_major) x += 1; else y += seg.sy;
                err += 2 * seg.D - 2 * seg.d;
            } else {
                err -= 2 * seg.d;
            }
            if (seg.y_major) y += seg.sy; else x += 1;
        }
    }
    // the long ones, one after the other, by the whole wave (all 64 lanes reach this point: no lane has returned)
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(seg.count > WIRE_SHORT);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int x0 = __shfl(seg.x, src), y0 = __shfl(seg.y, src), sy = __shfl(seg.sy, src), ym = __shfl(seg.y_major, src);
        const uint32_t D = (uint32_t)__shfl(seg.D, src), d = (uint32_t)__shfl(seg.d, src), k0 = __shfl(key, src);
        for (uint32_t k = lane; k <= D; k += 64) {  // D >= WIRE_SHORT > 0; 2 k d + D - 1 < 2^32 for clipped coordinates (< 2^15)
            const int minor = (int)((2u * k * d + D - 1u) / (2u * D));
            stamp(keys, W, H, ym ? x0 + minor : x0 + (int)k, ym ? y0 + sy * (int)k : y0 + sy * minor, k0);
        }
    }
}

// ---- class 2: dots ------------------------------------------------------------------------------------------------------------------------
// One lane per row of one filled circle: rows cy - R .. cy + R, columns cx - hw[|j|] .. cx + hw[|j|] (R <= 32: at most 65 pixels a lane).
__global__ __launch_bounds__(256) void stamp_dots_kernel(const int32_t* __restrict__ points, const int32_t* __restrict__ indices, const int32_t* __restrict__ half_widths,
                                                         uint32_t* __restrict__ keys, int n_rows, int V, int K, int R, int W, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int rows = 2 * R + 1, disc = i / rows, j = i - disc * rows - R, head = disc / K, k = disc - head * K;
    const int32_t* p = points + ((size_t)head * V + indices[k]) * 2;
    const int cx = p[0], y = p[1] + j;
    if ((unsigned)y >= (unsigned)H) return;
    const int half = half_widths[abs(j)];
    const uint32_t key = order_key(head, CLASS_DOTS);
    for (int x = max(cx - half, 0); x <= min(cx + half, W - 1); ++x) stamp(keys, W, H, x, y, key);
}

// ---- resolve ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t resolved(uint32_t key, uint32_t src_rgb) { return key ? class_colour((key - 1u) % (uint32_t)NUM_CLASSES) : src_rgb; }

// Four pixels per lane: 16 B of keys in, 12 B of destination out (the planes are dense and 4-byte aligned, so both are whole dwords).  The
// source rows may be pitched and start at any byte: when the four pixels lie in one row their 12 bytes come as three or four ALIGNED dwords
// that are shifted into place (an aligned dword that holds a byte of the image cannot leave the image's pages); four pixels that straddle
// two rows, and the tail of the image, go byte by byte.
__global__ __launch_bounds__(256) void resolve_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ src, int64_t src_pitch, uint8_t* __restrict__ dst, int W,
                                                      uint32_t n_pixels) {
    const uint32_t p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p0 >= n_pixels) return;
    const uint32_t row = p0 / (uint32_t)W, col = p0 - row * (uint32_t)W;
    if (p0 + 4u <= n_pixels && col + 4u <= (uint32_t)W) {
        const uint4 k = *reinterpret_cast<const uint4*>(keys + p0);
        const uint8_t* s = src + (size_t)row * src_pitch + (size_t)col * 3;
        const uint32_t shift = (uint32_t)((uintptr_t)s & 3);
        const uint32_t* a = reinterpret_cast<const uint32_t*>(s - shift);
        uint32_t w0 = a[0], w1 = a[1], w2 = a[2];
        if (shift) {  // bytes shift .. shift + 11 of the 16-byte window
            const uint32_t w3 = a[3];
            w0 = __builtin_amdgcn_alignbyte(w1, w0, shift);
            w1 = __builtin_amdgcn_alignbyte(w2, w1, shift);
            w2 = __builtin_amdgcn_alignbyte(w3, w2, shift);
        }
        // pixel j = bytes 3 j .. 3 j + 2 of (w0, w1, w2)
        const uint32_t q0 = resolved(k.x, w0 & 0xffffffu), q1 = resolved(k.y, (w0 >> 24 | w1 << 8) & 0xffffffu);
        const uint32_t q2 = resolved(k.z, (w1 >> 16 | w2 << 16) & 0xffffffu), q3 = resolved(k.w, w2 >> 8);
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + (size_t)p0 * 3);
        o[0] = q0 | q1 << 24;
        o[1] = q1 >> 8 | q2 << 16;
        o[2] = q2 >> 16 | q3 << 8;
        return;
    }
    for (uint32_t p = p0; p < min(p0 + 4u, n_pixels); ++p) {
        const uint32_t r = p / (uint32_t)W, c = p - r * (uint32_t)W;
        const uint8_t* s = src + (size_t)r * src_pitch + (size_t)c * 3;
        const uint32_t q = resolved(keys[p], (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16);
        uint8_t* o = dst + (size_t)p * 3;
        o[0] = (uint8_t)q;
        o[1] = (uint8_t)(q >> 8);
        o[2] = (uint8_t)(q >> 16);
    }
}

// ---- per-device state: the staging block of the uploads and the key plane, cleared by every call and guarded by the block's event (companion_host.h) ----
struct DrawState {
    Staging staging;
    Scratch<uint32_t> keys;
};

std::mutex g_mutex;
std::map<int, DrawState> g_state;

bool coord_ok(int32_t v) { return v > -VGHV_MAX_COORD && v < VGHV_MAX_COORD; }

}  // namespace

extern "C" VGHV_API int vghv_draw_heads(const vghv_draw_job* job, void* stream) {
    CH_REQUIRE(job, "draw_heads: null job");
    const vghv_draw_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.src_dev && j.dst_dev, "draw_heads: null image (src_dev %p, dst_dev %p)", (const void*)j.src_dev, (void*)j.dst_dev);
    CH_REQUIRE(j.channels == 3, "draw_heads: %d channels (needs 3: u8 RGB)", j.channels);
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHV_MAX_SIDE && j.width <= VGHV_MAX_SIDE, "draw_heads: image %d x %d outside 1 .. %d", j.height, j.width,
               VGHV_MAX_SIDE);
    CH_REQUIRE(j.src_pitch_bytes >= (int64_t)j.width * 3, "draw_heads: src_pitch_bytes %lld < width * 3 = %lld", (long long)j.src_pitch_bytes, (long long)j.width * 3);
    CH_REQUIRE(((uintptr_t)j.dst_dev & 3) == 0, "draw_heads: dst_dev %p is not 4-byte aligned", (void*)j.dst_dev);
    CH_REQUIRE(j.n_heads >= 0 && j.n_heads <= VGHV_MAX_DRAW_HEADS, "draw_heads: %d heads outside 0 .. %d", j.n_heads, VGHV_MAX_DRAW_HEADS);
    CH_REQUIRE(j.n_triangles >= 0 && j.n_indices >= 0 && j.n_vertices >= 0, "draw_heads: negative count");
    const int n = j.n_heads, V = j.n_vertices, T = j.n_triangles, K = j.n_indices, R = j.radius;
    const bool boxes = n && j.boxes, wire = n && T, dots = n && K;
    if (wire || dots) CH_REQUIRE(j.points && V >= 1, "draw_heads: wire and dots need points (points %p, n_vertices %d)", (const void*)j.points, V);
    if (wire) {
        CH_REQUIRE(j.triangles, "draw_heads: null triangles");
        CH_REQUIRE((int64_t)n * T * 3 <= INT32_MAX, "draw_heads: %lld segments exceed one launch", (long long)n * T * 3);
        for (int64_t i = 0; i < (int64_t)T * 3; ++i)
            CH_REQUIRE(j.triangles[i] >= 0 && j.triangles[i] < V, "draw_heads: triangle %lld: index %d outside the %d vertices", (long long)(i / 3), j.triangles[i], V);
    }
    if (dots) {
        CH_REQUIRE(j.indices && j.half_widths, "draw_heads: null indices or half_widths");
        CH_REQUIRE(R >= 1 && R <= VGHV_MAX_RADIUS, "draw_heads: radius %d outside 1 .. %d", R, VGHV_MAX_RADIUS);
        CH_REQUIRE((int64_t)n * K * (2 * R + 1) <= INT32_MAX, "draw_heads: %lld circle rows exceed one launch", (long long)n * K * (2 * R + 1));
        for (int i = 0; i < K; ++i) CH_REQUIRE(j.indices[i] >= 0 && j.indices[i] < V, "draw_heads: indices[%d] = %d outside the %d vertices", i, j.indices[i], V);
        for (int i = 0; i <= R; ++i) CH_REQUIRE(j.half_widths[i] >= 0 && j.half_widths[i] <= R, "draw_heads: half_widths[%d] = %d outside 0 .. radius", i, j.half_widths[i]);
    }
    const size_t n_points = (wire || dots) ? (size_t)n * V * 2 : 0;
    for (size_t i = 0; i < n_points; ++i)
        CH_REQUIRE(coord_ok(j.points[i]), "draw_heads: head %zu: coordinate %d outside +-2^24", i / ((size_t)V * 2), j.points[i]);
    if (boxes)
        for (int i = 0; i < n; ++i) {
            const int32_t* b = j.boxes + 4 * i;
            CH_REQUIRE(coord_ok(b[0]) && coord_ok(b[1]) && b[2] >= 0 && b[3] >= 0 && b[2] < VGHV_MAX_COORD && b[3] < VGHV_MAX_COORD, "draw_heads: head %d: bad box (%d, %d, %d, %d)", i,
                       b[0], b[1], b[2], b[3]);
        }

    const int W = j.width, H = j.height;
    const uint32_t n_pixels = (uint32_t)W * (uint32_t)H;  // < 2^30
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    DrawState& s = g_state[device];
    // one upload: [points | boxes | triangles | indices | half_widths], each from a 16-byte boundary
    const size_t at_boxes = align16(n_points * 4), at_tri = align16(at_boxes + (boxes ? (size_t)n * 16 : 0)), at_idx = align16(at_tri + (wire ? (size_t)T * 12 : 0));
    const size_t at_hw = align16(at_idx + (dots ? (size_t)K * 4 : 0)), total = align16(at_hw + (dots ? (size_t)(R + 1) * 4 : 0));
    if (int rc = reserve(s.staging, total ? total : 16, "draw_heads")) return rc;  // also waits for this device's previous draw
    if (!grow(s.keys, (size_t)n_pixels * 4)) {
        set_error("draw_heads: allocating the %zu-byte key plane failed", (size_t)n_pixels * 4);
        return ERR_NOMEM;
    }
    uint8_t* h = s.staging.host;
    if (n_points) memcpy(h, j.points, n_points * 4);
    if (boxes) memcpy(h + at_boxes, j.boxes, (size_t)n * 16);
    if (wire) memcpy(h + at_tri, j.triangles, (size_t)T * 12);
    if (dots) {
        memcpy(h + at_idx, j.indices, (size_t)K * 4);
        memcpy(h + at_hw, j.half_widths, (size_t)(R + 1) * 4);
    }
    // from here on work is queued (companion_host.h, queue-then-record); the event also guards the key plane, so it is recorded by every call that gets here
    const uint8_t* d = s.staging.dev;
    uint32_t* keys = s.keys.ptr;
    Queue q;
    if (total) CH_QUEUE(q, hipMemcpyAsync(s.staging.dev, h, total, hipMemcpyHostToDevice, st));
    CH_QUEUE(q, hipMemsetAsync(keys, 0, (size_t)n_pixels * 4, st));  // every call clears what it resolves: no stale keys from another image size
    const int32_t* d_points = (const int32_t*)d;
    if (boxes && q.ok()) {
        const int longest = W > H ? W : H;
        hipLaunchKernelGGL(stamp_boxes_kernel, dim3((unsigned)n * 4, (unsigned)(longest + 255) / 256), dim3(256), 0, st, (const int32_t*)(d + at_boxes), keys, W, H);
    }
    if (wire && q.ok()) {
        const int n_segments = n * T * 3;
        hipLaunchKernelGGL(stamp_wire_kernel, dim3((unsigned)(n_segments + 255) / 256), dim3(256), 0, st, d_points, (const int32_t*)(d + at_tri), keys, n_segments, V, T, W, H);
    }
    if (dots && q.ok()) {
        const int n_rows = n * K * (2 * R + 1);
        hipLaunchKernelGGL(stamp_dots_kernel, dim3((unsigned)(n_rows + 255) / 256), dim3(256), 0, st, d_points, (const int32_t*)(d + at_idx), (const int32_t*)(d + at_hw), keys, n_rows,
                           V, K, R, W, H);
    }
    if (q.ok()) hipLaunchKernelGGL(resolve_kernel, dim3((n_pixels / 4 + 256) / 256), dim3(256), 0, st, (const uint32_t*)keys, j.src_dev, j.src_pitch_bytes, j.dst_dev, W, n_pixels);
    return finish(q, s.staging, true, st, "draw_heads");
}
