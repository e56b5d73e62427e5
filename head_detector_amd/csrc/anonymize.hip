// libvghanon.so (include/vgh_anon.h): PredictionResult.anonymize -- every head of an image pixelated, blurred or filled, without a launch per head.
//
// OWNER: which head a pixel belongs to is an i32 plane [H, W], -1 = nobody.  For the box and ellipse regions it is painted by box, every pixel of a head's
// clipped box doing atomicMax(head) (the technique of csrc/draw.hip's order keys); for a mesh silhouette or a caller's mask the plane comes in as a pointer.
// VALUES: what an owned pixel becomes is looked up in one u32 (three channel bytes) per pixelation cell, or per pixel of a blurred head's clipped box:
//   pixelate   cells_kernel     one workgroup per cell: 64-bit integer sums of the cell's in-image pixels, rounded mean
//   blur       blur_rows_kernel one workgroup per 256-pixel row segment: the source row and its 2 r halo in LDS, h = the u16 horizontal pass
//              blur_cols_kernel one lane per pixel of the clipped box, a wave along a row: the vertical pass over h, rows read coalesced over columns
// RESOLVE: every destination pixel is written once, the source pixel or its owner's value (fill: the colour).
// Heads x tiles, x cells and x row segments are enumerated through prefix sums made on the host; a workgroup finds its head by bisection.  The memset of
// the owner plane, at most three launches and the resolve, whatever the number of heads.  Integer arithmetic only; every effect reads the source alone.
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/vgh_anon.h"
#include "companion_host.h"

namespace {

using namespace companion;
static_assert(VGHAN_OK == OK && VGHAN_ERR_INVALID == ERR_INVALID && VGHAN_ERR_HIP == ERR_HIP && VGHAN_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

constexpr int PAINT_W = 64, PAINT_H = 4;  // a tile of the owner painter and of the vertical pass: 256 lanes, one wave a row
constexpr int SEGMENT = 256;              // pixels of one row segment of the horizontal pass
constexpr int LINE_BYTES = (SEGMENT + 2 * VGHAN_MAX_RADIUS) * 3;  // the segment and the widest halo in LDS: 6912 bytes, so r is never chunked
static_assert(LINE_BYTES <= 65536, "static LDS only");

// One head as the kernels read it.  (cx0, cy0, cx1, cy1) is the geometry box clipped to the image, all 0 if nothing is left.  A pixel's value lies at
// values[val_at + ((y - vy0) / vdiv) * vstride + (x - vx0) / vdiv]: pixelate (x0, y0, cell, cells in a row), blur (cx0, cy0, 1, clipped width).
struct HeadRow {
    int32_t x0, y0, x1, y1;
    int32_t cx0, cy0, cx1, cy1;
    int32_t vx0, vy0, vdiv, vstride;
    int32_t radius, tap_at, hy0, hy1;  // blur: h holds rows hy0 .. hy1 - 1 = the clipped box extended by r rows and clamped to the image
    int64_t val_at, h_at;              // in u32 of the values, in u16 of h
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

// the pixel of lane `threadIdx.x` in tile `t` of the head's clipped box; false = outside the box
__device__ __forceinline__ bool tile_pixel(const HeadRow& r, uint32_t t, int& x, int& y) {
    const uint32_t across = (uint32_t)(r.cx1 - r.cx0 + PAINT_W - 1) / PAINT_W, ty = t / across, tx = t - ty * across;
    x = r.cx0 + (int)tx * PAINT_W + (int)(threadIdx.x & 63);
    y = r.cy0 + (int)ty * PAINT_H + (int)(threadIdx.x >> 6);
    return x < r.cx1 && y < r.cy1;  // cx1 <= W and cy1 <= H: a pixel that passes lies in the image
}

// ---- owner ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paint_owner_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ tiles, int n, int32_t* __restrict__ owner, int W, int ellipse) {
    const int i = head_of(tiles, n, blockIdx.x);
    const HeadRow r = rows[i];
    int x, y;
    if (!tile_pixel(r, blockIdx.x - tiles[i], x, y)) return;
    if (ellipse && !in_ellipse(r, x, y)) return;
    atomicMax(owner + (size_t)y * W + x, i);
}

// ---- pixelate -------------------------------------------------------------------------------------------------------------------------------
// One workgroup per cell: the four waves take the cell's in-image rows in turn, the lanes its columns (three adjacent bytes a lane, so a wave reads
// one contiguous stretch of a row).  64-bit sums: 255 * 32767^2 does not fit 32 bits.
__global__ __launch_bounds__(256) void cells_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ cells, int n, const uint8_t* __restrict__ src, int64_t pitch,
                                                    uint32_t* __restrict__ values, int W, int H) {
    __shared__ unsigned long long part[3][256];
    const int i = head_of(cells, n, blockIdx.x);
    const HeadRow r = rows[i];
    const uint32_t q = blockIdx.x - cells[i], cy = q / (uint32_t)r.vstride, cx = q - cy * (uint32_t)r.vstride;
    const int s = r.vdiv, gx = r.x0 + (int)cx * s, gy = r.y0 + (int)cy * s;
    const int ax = max(gx, 0), ay = max(gy, 0), bx = min(min(gx + s, r.x1), W), by = min(min(gy + s, r.y1), H);  // the cell, in the box, in the image
    if (bx <= ax || by <= ay) return;  // m = 0: never referenced (the whole workgroup leaves)
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int y = ay + (int)(threadIdx.x >> 6); y < by; y += 4) {
        const uint8_t* line = src + (size_t)y * pitch;
        for (int x = ax + (int)(threadIdx.x & 63); x < bx; x += 64) {
            const uint8_t* p = line + (size_t)x * 3;
            a0 += p[0];
            a1 += p[1];
            a2 += p[2];
        }
    }
    part[0][threadIdx.x] = a0;
    part[1][threadIdx.x] = a1;
    part[2][threadIdx.x] = a2;
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int c = 0; c < 3; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long m = (unsigned long long)(bx - ax) * (unsigned long long)(by - ay);
        uint32_t v = 0;
        for (int c = 0; c < 3; ++c) v |= (uint32_t)((2 * part[c][0] + m) / (2 * m)) << (8 * c);
        values[r.val_at + q] = v;
    }
}

// ---- blur -----------------------------------------------------------------------------------------------------------------------------------
// Horizontal pass.  One workgroup per (head, row of h, 256-pixel segment of the clipped box): the segment's source bytes and r pixels either side, columns
// clamped to the image, staged in LDS; lane t then sums pixel t of the segment.  The sum is at most 65536 * 255.
__global__ __launch_bounds__(256) void blur_rows_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ segments, int n, const int32_t* __restrict__ taps,
                                                        const uint8_t* __restrict__ src, int64_t pitch, uint16_t* __restrict__ h, int W) {
    __shared__ uint8_t line[LINE_BYTES];
    const int i = head_of(segments, n, blockIdx.x);
    const HeadRow r = rows[i];
    const int cw = r.cx1 - r.cx0;
    const uint32_t q = blockIdx.x - segments[i], across = (uint32_t)(cw + SEGMENT - 1) / SEGMENT, row = q / across, seg = q - row * across;
    const int y = r.hy0 + (int)row, sx = r.cx0 + (int)seg * SEGMENT, pixels = min(SEGMENT, r.cx1 - sx), rad = r.radius;
    const uint8_t* from = src + (size_t)y * pitch;
    for (int b = threadIdx.x; b < (pixels + 2 * rad) * 3; b += 256) {
        const int j = b / 3, c = b - 3 * j;
        line[b] = from[(size_t)min(max(sx - rad + j, 0), W - 1) * 3 + c];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= pixels) return;
    const int32_t* tap = taps + r.tap_at;
    const uint8_t* mid = line + (t + rad) * 3;
    uint32_t a0 = (uint32_t)tap[0] * mid[0], a1 = (uint32_t)tap[0] * mid[1], a2 = (uint32_t)tap[0] * mid[2];
    for (int k = 1; k <= rad; ++k) {
        const uint32_t w = (uint32_t)tap[k];
        const uint8_t *l = mid - 3 * k, *g = mid + 3 * k;
        a0 += w * ((uint32_t)l[0] + g[0]);
        a1 += w * ((uint32_t)l[1] + g[1]);
        a2 += w * ((uint32_t)l[2] + g[2]);
    }
    uint16_t* o = h + r.h_at + ((int64_t)row * cw + (sx - r.cx0 + t)) * 3;
    o[0] = (uint16_t)((a0 + 128u) >> 8);
    o[1] = (uint16_t)((a1 + 128u) >> 8);
    o[2] = (uint16_t)((a2 + 128u) >> 8);
}

// Vertical pass.  One lane per pixel of the clipped box, a wave along a row, so that every tap reads a row of h coalesced over the columns.  Only the
// pixels the head owns are computed: no other value is ever looked up.  The sum stays below 65536 * 65280 + 2^23 < 2^32.
__global__ __launch_bounds__(256) void blur_cols_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ tiles, int n, const int32_t* __restrict__ taps,
                                                        const int32_t* __restrict__ owner, const uint16_t* __restrict__ h, uint32_t* __restrict__ values, int W, int H) {
    const int i = head_of(tiles, n, blockIdx.x);
    const HeadRow r = rows[i];
    int x, y;
    if (!tile_pixel(r, blockIdx.x - tiles[i], x, y)) return;
    if (owner[(size_t)y * W + x] != i) return;
    const int cw = r.cx1 - r.cx0;
    const int32_t* tap = taps + r.tap_at;
    const uint16_t* col = h + r.h_at + (int64_t)(x - r.cx0) * 3;  // row yy of the image is row yy - hy0 of h; clamp(y +- k) stays inside hy0 .. hy1 - 1
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    for (int k = -r.radius; k <= r.radius; ++k) {
        const uint32_t w = (uint32_t)tap[abs(k)];
        const uint16_t* p = col + (int64_t)(min(max(y + k, 0), H - 1) - r.hy0) * cw * 3;
        a0 += w * p[0];
        a1 += w * p[1];
        a2 += w * p[2];
    }
    values[r.val_at + (int64_t)(y - r.cy0) * cw + (x - r.cx0)] = (a0 + (1u << 23)) >> 24 | ((a1 + (1u << 23)) >> 24) << 8 | ((a2 + (1u << 23)) >> 24) << 16;
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t resolved(const HeadRow* __restrict__ rows, int n, const uint32_t* __restrict__ values, int fill, uint32_t colour, int32_t o, int x, int y,
                                             uint32_t src_rgb) {
    if ((uint32_t)o >= (uint32_t)n) return src_rgb;
    const HeadRow* r = rows + o;
    if (x < r->x0 || x >= r->x1 || y < r->y0 || y >= r->y1) return src_rgb;  // outside its owner's geometry box: unchanged
    if (fill) return colour;
    return values[r->val_at + (int64_t)((y - r->vy0) / r->vdiv) * r->vstride + (x - r->vx0) / r->vdiv];
}

// Four pixels per lane, as csrc/draw.hip resolves its keys: 16 B of owners in, 12 B of destination out (both planes are dense and the owner plane is
// 16-byte aligned).  The source rows may be pitched and start at any byte: four pixels of one row come as three or four ALIGNED dwords that are
// shifted into place (an aligned dword that holds a byte of the image cannot leave the image's pages); four pixels that straddle two rows, and the
// tail of the image, go byte by byte.
__global__ __launch_bounds__(256) void resolve_kernel(const HeadRow* __restrict__ rows, int n, const int32_t* __restrict__ owner, const uint32_t* __restrict__ values, int fill,
                                                      uint32_t colour, const uint8_t* __restrict__ src, int64_t src_pitch, uint8_t* __restrict__ dst, int W, uint32_t n_pixels) {
    const uint32_t p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p0 >= n_pixels) return;
    const uint32_t row = p0 / (uint32_t)W, col = p0 - row * (uint32_t)W;
    if (p0 + 4u <= n_pixels && col + 4u <= (uint32_t)W) {
        const int4 k = *reinterpret_cast<const int4*>(owner + p0);
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
        const int x = (int)col, y = (int)row;
        const uint32_t q0 = resolved(rows, n, values, fill, colour, k.x, x, y, w0 & 0xffffffu);
        const uint32_t q1 = resolved(rows, n, values, fill, colour, k.y, x + 1, y, (w0 >> 24 | w1 << 8) & 0xffffffu);
        const uint32_t q2 = resolved(rows, n, values, fill, colour, k.z, x + 2, y, (w1 >> 16 | w2 << 16) & 0xffffffu);
        const uint32_t q3 = resolved(rows, n, values, fill, colour, k.w, x + 3, y, w2 >> 8);
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + (size_t)p0 * 3);
        o[0] = q0 | q1 << 24;
        o[1] = q1 >> 8 | q2 << 16;
        o[2] = q2 >> 16 | q3 << 8;
        return;
    }
    for (uint32_t p = p0; p < min(p0 + 4u, n_pixels); ++p) {
        const uint32_t r = p / (uint32_t)W, c = p - r * (uint32_t)W;
        const uint8_t* s = src + (size_t)r * src_pitch + (size_t)c * 3;
        const uint32_t q = resolved(rows, n, values, fill, colour, owner[p], (int)c, (int)r, (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16);
        uint8_t* o = dst + (size_t)p * 3;
        o[0] = (uint8_t)q;
        o[1] = (uint8_t)(q >> 8);
        o[2] = (uint8_t)(q >> 16);
    }
}

// ---- the host half: every check and every offset, no HIP call -----------------------------------------------------------------------------------
struct Plan {
    std::vector<HeadRow> rows;
    std::vector<uint32_t> tiles, cells, segments;  // prefix sums over the heads, n + 1 entries each
    int64_t at_values = 0, at_h = 0, total = 0;    // byte offsets in the workspace (the owner plane, if painted, is at 0)
};

int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// `who` words the messages: the two entry points share every check of the job
int make_plan(const vghan_job* job, Plan& p, const char* who) {
    CH_REQUIRE(job, "%s: null job", who);
    const vghan_job& j = *job;
    CH_REQUIRE(j.src_dev && j.dst_dev, "%s: null image (src_dev %p, dst_dev %p)", who, (const void*)j.src_dev, (void*)j.dst_dev);
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHAN_MAX_SIDE && j.width <= VGHAN_MAX_SIDE, "%s: image %d x %d outside 1 .. %d", who, j.height, j.width, VGHAN_MAX_SIDE);
    const int64_t H = j.height, W = j.width;
    CH_REQUIRE(j.src_pitch_bytes >= W * 3, "%s: src_pitch_bytes %lld < width * 3 = %lld", who, (long long)j.src_pitch_bytes, (long long)W * 3);
    CH_REQUIRE(j.src_pitch_bytes <= ((int64_t)1 << 40), "%s: src_pitch_bytes %lld is too large", who, (long long)j.src_pitch_bytes);
    CH_REQUIRE(((uintptr_t)j.dst_dev & 3) == 0, "%s: dst_dev %p is not 4-byte aligned", who, (void*)j.dst_dev);
    CH_REQUIRE(j.n_heads >= 0 && j.n_heads <= VGHAN_MAX_HEADS, "%s: n_heads %d outside 0 .. %d", who, j.n_heads, VGHAN_MAX_HEADS);
    CH_REQUIRE(j.method >= VGHAN_METHOD_FILL && j.method <= VGHAN_METHOD_BLUR, "%s: unknown method %d", who, j.method);
    CH_REQUIRE(j.region >= VGHAN_REGION_BOX && j.region <= VGHAN_REGION_MAP, "%s: unknown region %d", who, j.region);
    CH_REQUIRE((j.color & ~0xffffff) == 0, "%s: color 0x%x has more than three bytes", who, (unsigned)j.color);
    CH_REQUIRE(j.reserved == 0, "%s: reserved is %d, not 0", who, j.reserved);
    CH_REQUIRE((j.region == VGHAN_REGION_MAP) == (j.owner_dev != nullptr), "%s: owner_dev is %s for region %d (needed by VGHAN_REGION_MAP alone)", who, j.owner_dev ? "set" : "null", j.region);
    CH_REQUIRE(((uintptr_t)j.owner_dev & 15) == 0, "%s: owner_dev %p is not 16-byte aligned", who, (const void*)j.owner_dev);
    const int n = j.n_heads;
    const bool blur = j.method == VGHAN_METHOD_BLUR, pixelate = j.method == VGHAN_METHOD_PIXELATE;
    CH_REQUIRE(n == 0 || j.heads, "%s: null heads", who);
    CH_REQUIRE(j.n_taps >= 0, "%s: n_taps %d is negative", who, j.n_taps);
    if (blur && n) CH_REQUIRE(j.taps && j.n_taps >= 1, "%s: blur needs a tap table (taps %p, n_taps %d)", who, (const void*)j.taps, j.n_taps);
    {  // source and destination as byte ranges
        const uintptr_t s0 = (uintptr_t)j.src_dev, s1 = s0 + (uintptr_t)((H - 1) * j.src_pitch_bytes + W * 3), d0 = (uintptr_t)j.dst_dev, d1 = d0 + (uintptr_t)(H * W * 3);
        CH_REQUIRE(s1 <= d0 || d1 <= s0, "%s: source and destination overlap (the source is never modified)", who);
    }
    p.rows.assign((size_t)n, HeadRow{});
    p.tiles.assign((size_t)n + 1, 0);
    p.cells.assign((size_t)n + 1, 0);
    p.segments.assign((size_t)n + 1, 0);
    int64_t n_tiles = 0, n_cells = 0, n_segments = 0, n_values = 0, n_h = 0;
    int32_t ok_at = -1, ok_radius = -1;  // the table checked last: heads usually share one
    for (int i = 0; i < n; ++i) {
        const vghan_head& g = j.heads[i];
        HeadRow& r = p.rows[(size_t)i];
        CH_REQUIRE(g.x0 > -VGHAN_MAX_COORD && g.x0 < VGHAN_MAX_COORD && g.y0 > -VGHAN_MAX_COORD && g.y0 < VGHAN_MAX_COORD, "%s: head %d: corner (%d, %d) outside +-2^24", who, i, g.x0, g.y0);
        const int64_t wb = (int64_t)g.x1 - g.x0, hb = (int64_t)g.y1 - g.y0;
        CH_REQUIRE(wb >= 0 && hb >= 0 && wb <= VGHAN_MAX_SIDE && hb <= VGHAN_MAX_SIDE, "%s: head %d: box sides %lld x %lld outside 0 .. %d", who, i, (long long)wb, (long long)hb, VGHAN_MAX_SIDE);
        CH_REQUIRE(g.reserved == 0, "%s: head %d: reserved is %d, not 0", who, i, g.reserved);
        r.x0 = g.x0, r.y0 = g.y0, r.x1 = g.x1, r.y1 = g.y1;
        r.vdiv = 1;
        const int cx0 = g.x0 > 0 ? g.x0 : 0, cy0 = g.y0 > 0 ? g.y0 : 0, cx1 = g.x1 < W ? g.x1 : (int)W, cy1 = g.y1 < H ? g.y1 : (int)H;
        const bool empty = cx1 <= cx0 || cy1 <= cy0;
        if (!empty) r.cx0 = cx0, r.cy0 = cy0, r.cx1 = cx1, r.cy1 = cy1;
        const int64_t cw = r.cx1 - r.cx0, ch = r.cy1 - r.cy0;
        if (pixelate) {
            CH_REQUIRE(g.cell >= 1 && g.cell <= VGHAN_MAX_SIDE, "%s: head %d: cell side %d outside 1 .. %d", who, i, g.cell, VGHAN_MAX_SIDE);
            const int64_t across = (wb + g.cell - 1) / g.cell, down = (hb + g.cell - 1) / g.cell;
            CH_REQUIRE(across <= VGHAN_MAX_CELLS && down <= VGHAN_MAX_CELLS, "%s: head %d: %lld x %lld cells of side %d exceed %d a side", who, i, (long long)across, (long long)down, g.cell,
                       VGHAN_MAX_CELLS);
            r.vx0 = g.x0, r.vy0 = g.y0, r.vdiv = g.cell, r.vstride = (int32_t)across, r.val_at = n_values;
            if (!empty) n_cells += across * down, n_values += across * down;
        }
        if (blur) {
            CH_REQUIRE(g.radius >= 0 && g.radius <= VGHAN_MAX_RADIUS, "%s: head %d: radius %d outside 0 .. %d", who, i, g.radius, VGHAN_MAX_RADIUS);
            CH_REQUIRE(g.tap_offset >= 0 && (int64_t)g.tap_offset + g.radius < j.n_taps, "%s: head %d: taps %d .. %lld outside the table of %d", who, i, g.tap_offset,
                       (long long)g.tap_offset + g.radius, j.n_taps);
            if (g.tap_offset != ok_at || g.radius != ok_radius) {
                int64_t sum = 0;
                for (int k = 0; k <= g.radius; ++k) {
                    const int32_t t = j.taps[g.tap_offset + k];
                    CH_REQUIRE(t >= 0 && t <= VGHAN_TAP_SUM, "%s: head %d: tap %d is %d, outside 0 .. %d", who, i, k, t, VGHAN_TAP_SUM);
                    sum += k ? 2 * (int64_t)t : t;
                }
                CH_REQUIRE(sum == VGHAN_TAP_SUM, "%s: head %d: tap sum %lld is not %d", who, i, (long long)sum, VGHAN_TAP_SUM);
                ok_at = g.tap_offset, ok_radius = g.radius;
            }
            r.radius = g.radius, r.tap_at = g.tap_offset;
            r.vx0 = r.cx0, r.vy0 = r.cy0, r.vdiv = 1, r.vstride = (int32_t)cw, r.val_at = n_values, r.h_at = n_h;
            r.hy0 = r.cy0 - g.radius > 0 ? r.cy0 - g.radius : 0;
            r.hy1 = r.cy1 + g.radius < H ? r.cy1 + g.radius : (int)H;
            if (!empty) {
                n_values += cw * ch;
                n_h += (int64_t)(r.hy1 - r.hy0) * cw * 3;
                n_segments += (int64_t)(r.hy1 - r.hy0) * ((cw + SEGMENT - 1) / SEGMENT);
            }
        }
        if (!empty) n_tiles += ((cw + PAINT_W - 1) / PAINT_W) * ((ch + PAINT_H - 1) / PAINT_H);
        CH_REQUIRE(n_tiles <= INT32_MAX && n_cells <= INT32_MAX && n_segments <= INT32_MAX, "%s: head %d: the boxes so far exceed one launch (%lld tiles, %lld cells, %lld row segments)", who,
                   i, (long long)n_tiles, (long long)n_cells, (long long)n_segments);
        p.tiles[(size_t)i + 1] = (uint32_t)n_tiles, p.cells[(size_t)i + 1] = (uint32_t)n_cells, p.segments[(size_t)i + 1] = (uint32_t)n_segments;
    }
    p.at_values = up16(j.region == VGHAN_REGION_MAP ? 0 : 4 * H * W);
    p.at_h = up16(p.at_values + 4 * n_values);
    p.total = up16(p.at_h + 2 * n_h);
    if (p.total < 16) p.total = 16;
    return OK;
}

std::mutex g_mutex;
std::map<int, Staging> g_staging;  // per device: the head rows, the prefix sums and the taps of one call

}  // namespace

extern "C" VGHAN_API const char* vghan_version(void) { return "vghanon 1 (gfx950)"; }
extern "C" VGHAN_API const char* vghan_last_error(void) { return last_error(); }

extern "C" VGHAN_API int64_t vghan_workspace_bytes(const vghan_job* job) {
    Plan p;
    return make_plan(job, p, "workspace_bytes") == OK ? p.total : 0;
}

extern "C" VGHAN_API int vghan_anonymize(const vghan_job* job, void* workspace_dev, void* stream) {
    Plan p;
    // everything is checked before anything is allocated, written or queued
    if (int rc = make_plan(job, p, "anonymize")) return rc;
    CH_REQUIRE(workspace_dev, "anonymize: null workspace");
    CH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "anonymize: workspace is not 16-byte aligned");
    const vghan_job& j = *job;
    const int n = j.n_heads, W = j.width, H = j.height;
    const uint32_t n_pixels = (uint32_t)W * (uint32_t)H;  // < 2^30
    const bool blur = j.method == VGHAN_METHOD_BLUR, pixelate = j.method == VGHAN_METHOD_PIXELATE, paint = j.region != VGHAN_REGION_MAP;
    const uint32_t n_tiles = p.tiles[(size_t)n], n_cells = p.cells[(size_t)n], n_segments = p.segments[(size_t)n];
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    // one upload: [rows | tiles | cells | segments | taps], each from a 16-byte boundary
    const size_t prefix_bytes = ((size_t)n + 1) * 4, at_tiles = align16((size_t)n * sizeof(HeadRow)), at_cells = align16(at_tiles + prefix_bytes);
    const size_t at_segments = align16(at_cells + prefix_bytes), at_taps = align16(at_segments + prefix_bytes), total = align16(at_taps + (blur ? (size_t)j.n_taps * 4 : 0));
    if (int rc = reserve(s, total, "anonymize")) return rc;  // also waits for this device's previous call
    uint8_t* host = s.host;
    if (n) memcpy(host, p.rows.data(), (size_t)n * sizeof(HeadRow));
    memcpy(host + at_tiles, p.tiles.data(), prefix_bytes);
    memcpy(host + at_cells, p.cells.data(), prefix_bytes);
    memcpy(host + at_segments, p.segments.data(), prefix_bytes);
    if (blur && j.n_taps) memcpy(host + at_taps, j.taps, (size_t)j.n_taps * 4);
    // from here on work is queued (companion_host.h, queue-then-record)
    const uint8_t* d = s.dev;
    const HeadRow* rows = (const HeadRow*)d;
    const uint32_t *tiles = (const uint32_t*)(d + at_tiles), *cells = (const uint32_t*)(d + at_cells), *segments = (const uint32_t*)(d + at_segments);
    const int32_t* taps = (const int32_t*)(d + at_taps);
    uint8_t* ws = (uint8_t*)workspace_dev;
    int32_t* painted = (int32_t*)ws;
    const int32_t* owner = paint ? painted : j.owner_dev;
    uint32_t* values = (uint32_t*)(ws + p.at_values);
    uint16_t* h = (uint16_t*)(ws + p.at_h);
    Queue q;
    CH_QUEUE(q, hipMemcpyAsync(s.dev, host, total, hipMemcpyHostToDevice, st));
    if (paint) {
        CH_QUEUE(q, hipMemsetAsync(painted, 0xff, (size_t)n_pixels * 4, st));  // -1 everywhere
        if (n_tiles && q.ok())
            hipLaunchKernelGGL(paint_owner_kernel, dim3(n_tiles), dim3(256), 0, st, rows, tiles, n, painted, W, (int)(j.region == VGHAN_REGION_ELLIPSE));
    }
    if (pixelate && n_cells && q.ok()) hipLaunchKernelGGL(cells_kernel, dim3(n_cells), dim3(256), 0, st, rows, cells, n, j.src_dev, j.src_pitch_bytes, values, W, H);
    if (blur && n_segments && q.ok()) {
        hipLaunchKernelGGL(blur_rows_kernel, dim3(n_segments), dim3(256), 0, st, rows, segments, n, taps, j.src_dev, j.src_pitch_bytes, h, W);
        hipLaunchKernelGGL(blur_cols_kernel, dim3(n_tiles), dim3(256), 0, st, rows, tiles, n, taps, owner, (const uint16_t*)h, values, W, H);
    }
    if (q.ok())
        hipLaunchKernelGGL(resolve_kernel, dim3((n_pixels / 4 + 256) / 256), dim3(256), 0, st, rows, n, owner, (const uint32_t*)values, (int)(j.method == VGHAN_METHOD_FILL), (uint32_t)j.color,
                           j.src_dev, j.src_pitch_bytes, j.dst_dev, W, n_pixels);
    return finish(q, s, true, st, "anonymize");
}
