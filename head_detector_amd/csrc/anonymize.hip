// libvghanon.so (include/vgh_anon.h): PredictionResult.anonymize -- every head of an image pixelated, blurred or filled, without a launch per head.
//
// OWNER: which head a pixel belongs to is an i32 plane [H, W], -1 = nobody.  For the box and ellipse regions it is painted by box, every pixel of a head's
// clipped box doing atomicMax(head) (csrc/head_rows.h; the technique of csrc/draw.hip's order keys); for a mesh silhouette or a caller's mask the plane comes
// in as a pointer.
// VALUES: what an owned pixel becomes is looked up in one u32 (three channel bytes) per pixelation cell, or per pixel of a blurred head's clipped box:
//   pixelate   cells_kernel     one workgroup per cell: 64-bit integer sums of the cell's in-image pixels, rounded mean
//   blur       blur_rows_kernel one workgroup per 256-pixel row segment: the source row and its 2 r halo in LDS, h = the u16 horizontal pass
//              blur_cols_kernel one lane per pixel of the clipped box, a wave along a row: the vertical pass over h, rows read coalesced over columns
// RESOLVE: every destination pixel is written once, the source pixel or its owner's value (fill: the colour).
// Heads x tiles, x cells and x row segments are enumerated through prefix sums made on the host; a workgroup finds its head by bisection.  The memset of
// the owner plane, at most three launches and the resolve, whatever the number of heads.  Integer arithmetic only; every effect reads the source alone.
// The head rows, their per-head checks and offsets (in samples: a pixel is one sample of three bytes), the bisection, the owner painter and the staged upload
// are csrc/head_rows.h, shared with csrc/yuv_anonymize.hip; the checks of the job, the workspace layout and every kernel that touches a pixel are here.
#include <map>
#include <mutex>

#include "../../include/vgh_anon.h"
#include "companion_host.h"
#include "head_rows.h"

namespace {

using namespace head_rows;
static_assert(VGHAN_OK == OK && VGHAN_ERR_INVALID == ERR_INVALID && VGHAN_ERR_HIP == ERR_HIP && VGHAN_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");
static_assert(VGHAN_MAX_SIDE == MAX_SIDE && VGHAN_MAX_COORD == MAX_COORD && VGHAN_MAX_HEADS == MAX_HEADS && VGHAN_MAX_CELLS == MAX_CELLS && VGHAN_MAX_RADIUS == MAX_RADIUS &&
                  VGHAN_TAP_SUM == TAP_SUM && VGHAN_METHOD_FILL == METHOD_FILL && VGHAN_METHOD_PIXELATE == METHOD_PIXELATE && VGHAN_METHOD_BLUR == METHOD_BLUR,
              "head_rows.h plans with these caps and methods");

constexpr int LINE_BYTES = (SEGMENT + 2 * VGHAN_MAX_RADIUS) * 3;  // the segment and the widest halo in LDS: 6912 bytes, so r is never chunked
static_assert(LINE_BYTES <= 65536, "static LDS only");

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
    uint16_t* o = h + (r.h_at + (int64_t)row * cw + (sx - r.cx0 + t)) * 3;
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
    if (!tile_sample(r, blockIdx.x - tiles[i], x, y)) return;
    if (owner[(size_t)y * W + x] != i) return;
    const int cw = r.cx1 - r.cx0;
    const int32_t* tap = taps + r.tap_at;
    const uint16_t* col = h + (r.h_at + (int64_t)(x - r.cx0)) * 3;  // row yy of the image is row yy - hy0 of h; clamp(y +- k) stays inside hy0 .. hy1 - 1
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
struct Plan : GroupPlan {
    int64_t at_values = 0, at_h = 0, total = 0;  // byte offsets in the workspace (the owner plane, if painted, is at 0)
};

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
    const bool blur = j.method == VGHAN_METHOD_BLUR;
    CH_REQUIRE(n == 0 || j.heads, "%s: null heads", who);
    CH_REQUIRE(j.n_taps >= 0, "%s: n_taps %d is negative", who, j.n_taps);
    if (blur && n) CH_REQUIRE(j.taps && j.n_taps >= 1, "%s: blur needs a tap table (taps %p, n_taps %d)", who, (const void*)j.taps, j.n_taps);
    {  // source and destination as byte ranges
        const uintptr_t s0 = (uintptr_t)j.src_dev, s1 = s0 + (uintptr_t)((H - 1) * j.src_pitch_bytes + W * 3), d0 = (uintptr_t)j.dst_dev, d1 = d0 + (uintptr_t)(H * W * 3);
        CH_REQUIRE(s1 <= d0 || d1 <= s0, "%s: source and destination overlap (the source is never modified)", who);
    }
    if (int rc = plan_heads(j.heads, n, j.method, j.taps, j.n_taps, W, H, p, who, "head")) return rc;
    p.at_values = up16(j.region == VGHAN_REGION_MAP ? 0 : 4 * H * W);
    p.at_h = up16(p.at_values + 4 * p.n_values);
    p.total = up16(p.at_h + 2 * 3 * p.n_h);
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
    // one upload: [the rows and their prefix sums | taps], each from a 16-byte boundary
    const size_t at_taps = group_bytes(n), total = align16(at_taps + (blur ? (size_t)j.n_taps * 4 : 0));
    if (int rc = reserve(s, total, "anonymize")) return rc;  // also waits for this device's previous call
    const GroupOnDevice g = stage_group(p, s, 0);
    if (blur && j.n_taps) memcpy(s.host + at_taps, j.taps, (size_t)j.n_taps * 4);
    // from here on work is queued (companion_host.h, queue-then-record)
    const int32_t* taps = (const int32_t*)(s.dev + at_taps);
    uint8_t* ws = (uint8_t*)workspace_dev;
    int32_t* painted = (int32_t*)ws;
    const int32_t* owner = paint ? painted : j.owner_dev;
    uint32_t* values = (uint32_t*)(ws + p.at_values);
    uint16_t* h = (uint16_t*)(ws + p.at_h);
    Queue q;
    CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));
    if (paint) {
        CH_QUEUE(q, hipMemsetAsync(painted, 0xff, (size_t)n_pixels * 4, st));  // -1 everywhere
        if (n_tiles && q.ok())
            hipLaunchKernelGGL(paint_owner_kernel, dim3(n_tiles), dim3(256), 0, st, g.rows, g.tiles, n, painted, W, (int)(j.region == VGHAN_REGION_ELLIPSE));
    }
    if (pixelate && n_cells && q.ok()) hipLaunchKernelGGL(cells_kernel, dim3(n_cells), dim3(256), 0, st, g.rows, g.cells, n, j.src_dev, j.src_pitch_bytes, values, W, H);
    if (blur && n_segments && q.ok()) {
        hipLaunchKernelGGL(blur_rows_kernel, dim3(n_segments), dim3(256), 0, st, g.rows, g.segments, n, taps, j.src_dev, j.src_pitch_bytes, h, W);
        hipLaunchKernelGGL(blur_cols_kernel, dim3(n_tiles), dim3(256), 0, st, g.rows, g.tiles, n, taps, owner, (const uint16_t*)h, values, W, H);
    }
    if (q.ok())
        hipLaunchKernelGGL(resolve_kernel, dim3((n_pixels / 4 + 256) / 256), dim3(256), 0, st, g.rows, n, owner, (const uint32_t*)values, (int)(j.method == VGHAN_METHOD_FILL), (uint32_t)j.color,
                           j.src_dev, j.src_pitch_bytes, j.dst_dev, W, n_pixels);
    return finish(q, s, true, st, "anonymize");
}
