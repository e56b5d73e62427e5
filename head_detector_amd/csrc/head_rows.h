// The head rows that csrc/anonymize.hip (libvghanon.so: RGB images) and csrc/yuv_anonymize.hip (libvghvideo.so: the planes of a YUV 4:2:0 frame) share: one
// head in one plane as the kernels read it, the prefix sums that enumerate heads x tiles, x cells and x row segments, the owner painter, the per-head checks
// and offsets on the host, and the staged upload of a group of rows.  One rule, stated once: an image is a plane of three-byte samples, a luma plane one of
// one-byte samples, the chroma planes one of two-byte samples; every count and offset here is in SAMPLES, and the kernels that touch the samples are the
// includer's.  Header-only and internal: every definition has internal linkage or is inline, so each library compiles its own copy and stays a library of its
// own (no shared object, no exported symbol, no link dependency).  Integer arithmetic only.
#pragma once
#include <string.h>

#include <vector>

#include "companion_host.h"

namespace head_rows {
using namespace companion;
namespace {

constexpr int TILE_W = 64, TILE_H = 4;  // a tile of the owner painter and of every pass that walks the clipped boxes: 256 lanes, one wave a row
constexpr int SEGMENT = 256;            // samples of one row segment of the horizontal pass
// The caps and the methods; each includer static_asserts them against those of its public header.
constexpr int MAX_SIDE = 32767, MAX_COORD = 1 << 24, MAX_HEADS = 65536, MAX_CELLS = 64, MAX_RADIUS = 1024, TAP_SUM = 65536;
constexpr int METHOD_FILL = 0, METHOD_PIXELATE = 1, METHOD_BLUR = 2;

// One head in one plane.  (cx0, cy0, cx1, cy1) is the geometry box clipped to the plane, all 0 if nothing is left.  A sample's value lies at
// values[val_at + ((y - vy0) / vdiv) * vstride + (x - vx0) / vdiv]: pixelate (x0, y0, cell, cells in a row), blur (cx0, cy0, 1, clipped width).
struct HeadRow {
    int32_t x0, y0, x1, y1;
    int32_t cx0, cy0, cx1, cy1;
    int32_t vx0, vy0, vdiv, vstride;
    int32_t radius, tap_at, hy0, hy1;  // blur: h holds rows hy0 .. hy1 - 1 = the clipped box extended by r rows and clamped to the plane
    int64_t val_at, h_at;              // in samples, of the values and of h
};
static_assert(sizeof(HeadRow) == 80, "uploaded as it is");

// the largest i in [0, n) with prefix[i] <= item; prefix[0] = 0 and item < prefix[n], so prefix[i + 1] > item: heads without items are stepped over
__device__ __forceinline__ int head_of(const uint32_t* __restrict__ prefix, int n, uint32_t item) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool in_ellipse(const HeadRow& r, int x, int y) {
    const int64_t wb = r.x1 - r.x0, hb = r.y1 - r.y0, ex = 2 * (int64_t)(x - r.x0) + 1 - wb, ey = 2 * (int64_t)(y - r.y0) + 1 - hb;
    return ex * ex * hb * hb + ey * ey * wb * wb <= wb * wb * hb * hb;
}

// the sample of lane `threadIdx.x` in tile `t` of the head's clipped box; false = outside the box
__device__ __forceinline__ bool tile_sample(const HeadRow& r, uint32_t t, int& x, int& y) {
    const uint32_t across = (uint32_t)(r.cx1 - r.cx0 + TILE_W - 1) / TILE_W, ty = t / across, tx = t - ty * across;
    x = r.cx0 + (int)tx * TILE_W + (int)(threadIdx.x & 63);
    y = r.cy0 + (int)ty * TILE_H + (int)(threadIdx.x >> 6);
    return x < r.cx1 && y < r.cy1;  // cx1 <= W and cy1 <= H of the plane: a sample that passes lies in the plane
}

// ---- owner: every sample of a head's clipped box (of the inscribed ellipse) does atomicMax(head) on an i32 plane [H, W] that starts at -1 ---------------
__global__ __launch_bounds__(256) void paint_owner_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ tiles, int n, int32_t* __restrict__ owner, int W, int ellipse) {
    const int i = head_of(tiles, n, blockIdx.x);
    const HeadRow r = rows[i];
    int x, y;
    if (!tile_sample(r, blockIdx.x - tiles[i], x, y)) return;
    if (ellipse && !in_ellipse(r, x, y)) return;
    atomicMax(owner + (size_t)y * W + x, i);
}

// ---- the host half: every per-head check and every offset, no HIP call ------------------------------------------------------------------------------
struct GroupPlan {  // the heads of one plane
    std::vector<HeadRow> rows;
    std::vector<uint32_t> tiles, cells, segments;  // prefix sums over the heads, n + 1 entries each
    int64_t n_values = 0, n_h = 0;                 // samples
};

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// The rows of `n` heads in a plane of W x H samples.  `Head` is the public header's row (eight int32: x0, y0, x1, y1, cell, radius, tap_offset, reserved);
// `who` and `label` word the messages: "<who>: <label> <i>: ...".
template <typename Head>
int plan_heads(const Head* heads, int n, int method, const int32_t* taps, int n_taps, int64_t W, int64_t H, GroupPlan& p, const char* who, const char* label) {
    const bool blur = method == METHOD_BLUR, pixelate = method == METHOD_PIXELATE;
    p.rows.assign((size_t)n, HeadRow{});
    p.tiles.assign((size_t)n + 1, 0);
    p.cells.assign((size_t)n + 1, 0);
    p.segments.assign((size_t)n + 1, 0);
    p.n_values = p.n_h = 0;
    int64_t n_tiles = 0, n_cells = 0, n_segments = 0;
    int32_t ok_at = -1, ok_radius = -1;  // the table checked last: heads usually share one
    for (int i = 0; i < n; ++i) {
        const Head& g = heads[i];
        HeadRow& r = p.rows[(size_t)i];
        CH_REQUIRE(g.x0 > -MAX_COORD && g.x0 < MAX_COORD && g.y0 > -MAX_COORD && g.y0 < MAX_COORD, "%s: %s %d: corner (%d, %d) outside +-2^24", who, label, i, g.x0, g.y0);
        const int64_t wb = (int64_t)g.x1 - g.x0, hb = (int64_t)g.y1 - g.y0;
        CH_REQUIRE(wb >= 0 && hb >= 0 && wb <= MAX_SIDE && hb <= MAX_SIDE, "%s: %s %d: box sides %lld x %lld outside 0 .. %d", who, label, i, (long long)wb, (long long)hb, MAX_SIDE);
        CH_REQUIRE(g.reserved == 0, "%s: %s %d: reserved is %d, not 0", who, label, i, g.reserved);
        r.x0 = g.x0, r.y0 = g.y0, r.x1 = g.x1, r.y1 = g.y1;
        r.vdiv = 1;
        const int cx0 = g.x0 > 0 ? g.x0 : 0, cy0 = g.y0 > 0 ? g.y0 : 0, cx1 = g.x1 < W ? g.x1 : (int)W, cy1 = g.y1 < H ? g.y1 : (int)H;
        const bool empty = cx1 <= cx0 || cy1 <= cy0;
        if (!empty) r.cx0 = cx0, r.cy0 = cy0, r.cx1 = cx1, r.cy1 = cy1;
        const int64_t cw = r.cx1 - r.cx0, ch = r.cy1 - r.cy0;
        if (pixelate) {
            CH_REQUIRE(g.cell >= 1 && g.cell <= MAX_SIDE, "%s: %s %d: cell side %d outside 1 .. %d", who, label, i, g.cell, MAX_SIDE);
            const int64_t across = (wb + g.cell - 1) / g.cell, down = (hb + g.cell - 1) / g.cell;
            CH_REQUIRE(across <= MAX_CELLS && down <= MAX_CELLS, "%s: %s %d: %lld x %lld cells of side %d exceed %d a side", who, label, i, (long long)across, (long long)down, g.cell, MAX_CELLS);
            r.vx0 = g.x0, r.vy0 = g.y0, r.vdiv = g.cell, r.vstride = (int32_t)across, r.val_at = p.n_values;
            if (!empty) n_cells += across * down, p.n_values += across * down;
        }
        if (blur) {
            CH_REQUIRE(g.radius >= 0 && g.radius <= MAX_RADIUS, "%s: %s %d: radius %d outside 0 .. %d", who, label, i, g.radius, MAX_RADIUS);
            CH_REQUIRE(g.tap_offset >= 0 && (int64_t)g.tap_offset + g.radius < n_taps, "%s: %s %d: taps %d .. %lld outside the table of %d", who, label, i, g.tap_offset,
                       (long long)g.tap_offset + g.radius, n_taps);
            if (g.tap_offset != ok_at || g.radius != ok_radius) {
                int64_t sum = 0;
                for (int k = 0; k <= g.radius; ++k) {
                    const int32_t t = taps[g.tap_offset + k];
                    CH_REQUIRE(t >= 0 && t <= TAP_SUM, "%s: %s %d: tap %d is %d, outside 0 .. %d", who, label, i, k, t, TAP_SUM);
                    sum += k ? 2 * (int64_t)t : t;
                }
                CH_REQUIRE(sum == TAP_SUM, "%s: %s %d: tap sum %lld is not %d", who, label, i, (long long)sum, TAP_SUM);
                ok_at = g.tap_offset, ok_radius = g.radius;
            }
            r.radius = g.radius, r.tap_at = g.tap_offset;
            r.vx0 = r.cx0, r.vy0 = r.cy0, r.vdiv = 1, r.vstride = (int32_t)cw, r.val_at = p.n_values, r.h_at = p.n_h;
            r.hy0 = r.cy0 - g.radius > 0 ? r.cy0 - g.radius : 0;
            r.hy1 = r.cy1 + g.radius < H ? r.cy1 + g.radius : (int)H;
            if (!empty) {
                p.n_values += cw * ch;
                p.n_h += (int64_t)(r.hy1 - r.hy0) * cw;
                n_segments += (int64_t)(r.hy1 - r.hy0) * ((cw + SEGMENT - 1) / SEGMENT);
            }
        }
        if (!empty) n_tiles += ((cw + TILE_W - 1) / TILE_W) * ((ch + TILE_H - 1) / TILE_H);
        CH_REQUIRE(n_tiles <= INT32_MAX && n_cells <= INT32_MAX && n_segments <= INT32_MAX, "%s: %s %d: the boxes so far exceed one launch (%lld tiles, %lld cells, %lld row segments)", who,
                   label, i, (long long)n_tiles, (long long)n_cells, (long long)n_segments);
        p.tiles[(size_t)i + 1] = (uint32_t)n_tiles, p.cells[(size_t)i + 1] = (uint32_t)n_cells, p.segments[(size_t)i + 1] = (uint32_t)n_segments;
    }
    return OK;
}

// ---- the staged upload of a group: [rows | tiles | cells | segments], each from a 16-byte boundary --------------------------------------------------
inline size_t group_bytes(int n) { return align16((size_t)n * sizeof(HeadRow)) + 3 * align16(((size_t)n + 1) * 4); }

struct GroupOnDevice {
    const HeadRow* rows;
    const uint32_t *tiles, *cells, *segments;
};

// copies the group into the pinned block from byte `at` (a multiple of 16; group_bytes(n) are taken) and returns where the device block will hold it
inline GroupOnDevice stage_group(const GroupPlan& p, const Staging& s, size_t at) {
    const size_t n = p.rows.size(), prefix_bytes = (n + 1) * 4, prefix_room = align16(prefix_bytes), at_prefix = at + align16(n * sizeof(HeadRow));
    if (n) memcpy(s.host + at, p.rows.data(), n * sizeof(HeadRow));
    memcpy(s.host + at_prefix, p.tiles.data(), prefix_bytes);
    memcpy(s.host + at_prefix + prefix_room, p.cells.data(), prefix_bytes);
    memcpy(s.host + at_prefix + 2 * prefix_room, p.segments.data(), prefix_bytes);
    const uint8_t* d = s.dev + at_prefix;
    return GroupOnDevice{(const HeadRow*)(s.dev + at), (const uint32_t*)d, (const uint32_t*)(d + prefix_room), (const uint32_t*)(d + 2 * prefix_room)};
}

}  // namespace
}  // namespace head_rows
