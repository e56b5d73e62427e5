// libvghvideo.so (include/vgh_video.h): video.anonymize_frame -- every head of an 8-bit YUV 4:2:0 frame pixelated, blurred or filled directly in the luma and
// chroma planes, in place if wanted, without an RGB image and without a launch per head.
//
// Every plane is a one-channel image under one rule; the kernels are written once for NC channels that share their geometry: NC = 1 is the luma plane, NC = 2
// the U and V planes, which are either two planes (planar) or, where they are the two interleaved views of one NV12 / NV21 plane, a (U, V) pair that a lane
// loads and stores with one 16-bit access.
// OWNER: the luma owner plane, i32 [H, W], -1 = nobody, is painted by box (atomicMax of the head over its clipped box) or comes in as a pointer; a chroma
// sample's owner is the maximum of the (up to) four luma owners it colours, taken where it is needed.
// VALUES: what an owned sample becomes is staged in the workspace from the SOURCE planes before anything is written, NC bytes per pixelation cell or per sample
// of a blurred head's clipped box:
//   pixelate   cells_kernel      one workgroup per cell: 64-bit integer sums of the cell's in-plane samples, rounded mean
//   blur       blur_rows_kernel  one workgroup per 256-sample row segment: the source row and its 2 r halo in LDS, h = the u16 horizontal pass
//              blur_cols_kernel  one lane per sample of the clipped box, a wave along a row: the vertical pass over h, for the samples the head owns
// WRITE: write_kernel, one lane per sample of every head's clipped box, stores the value (fill: the colour) where the head owns the sample: the only pass
// that writes a frame in place.  A plane that is out of place is copied first (planes::copy_kernel, the one pass that walks a whole plane).
// Heads x tiles, x cells and x row segments are enumerated through prefix sums made on the host; a workgroup finds its head by bisection.  Integer arithmetic
// only.  The head rows, their per-head checks and offsets, the bisection, the owner painter and the staged upload are csrc/head_rows.h, shared with
// csrc/anonymize.hip; a plane's checks, the overlap rule, the pair test, the pair access and the copy are csrc/plane_views.h, shared with csrc/osd.hip; the
// other checks of the job, the workspace layout and every other kernel that touches a sample are here.
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_video.h"
#include "companion_host.h"
#include "head_rows.h"
#include "plane_views.h"

namespace {

using namespace head_rows;
static_assert(VGHY_OK == OK && VGHY_ERR_INVALID == ERR_INVALID && VGHY_ERR_HIP == ERR_HIP && VGHY_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");
static_assert(VGHY_MAX_SIDE == MAX_SIDE && VGHY_MAX_COORD == MAX_COORD && VGHY_MAX_HEADS == MAX_HEADS && VGHY_MAX_CELLS == MAX_CELLS && VGHY_MAX_RADIUS == MAX_RADIUS &&
                  VGHY_TAP_SUM == TAP_SUM && VGHY_METHOD_FILL == METHOD_FILL && VGHY_METHOD_PIXELATE == METHOD_PIXELATE && VGHY_METHOD_BLUR == METHOD_BLUR,
              "head_rows.h plans with these caps and methods");

constexpr int LINE_SAMPLES = SEGMENT + 2 * VGHY_MAX_RADIUS;  // the segment and the widest halo in LDS (luma: 256 + 2 * 1024 bytes), so r is never chunked

// A plane group: NC channels (csrc/plane_views.h) of one width and height.
template <int NC>
struct View {
    planes::Chan c[NC];
    int32_t W, H;          // of the plane
    int32_t spair, dpair;  // NC = 2: 0 = two planes; 1 / 2 = c[0] / c[1] is the even, lower byte of interleaved pairs
};

// Does head i own sample (x, y) of this plane group?  Luma: the owner plane itself.  Chroma: the maximum of the owners, -1 for every value outside [0, n), of
// the luma pixels {2 y, 2 y + 1} x {2 x, 2 x + 1} that lie in the frame (LW x LH).
template <int NC>
__device__ __forceinline__ bool owned_by(const int32_t* __restrict__ owner, int LW, int LH, int n, int x, int y, int i) {
    if constexpr (NC == 1) {
        return owner[(size_t)y * LW + x] == i;
    } else {
        int o = -1;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int lx = 2 * x + dx, ly = 2 * y + dy;
                if (lx < LW && ly < LH) {
                    const int32_t k = owner[(size_t)ly * LW + lx];
                    if ((uint32_t)k < (uint32_t)n) o = max(o, k);
                }
            }
        return o == i;
    }
}

// ---- pixelate -------------------------------------------------------------------------------------------------------------------------------
// One workgroup per cell: the four waves take the cell's in-plane rows in turn, the lanes its columns.  64-bit sums: 255 * 32767^2 does not fit 32 bits.
template <int NC>
__global__ __launch_bounds__(256) void cells_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ cells, int n, View<NC> P, uint8_t* __restrict__ values) {
    __shared__ unsigned long long part[NC][256];
    const int i = head_of(cells, n, blockIdx.x);
    const HeadRow r = rows[i];
    const uint32_t q = blockIdx.x - cells[i], cy = q / (uint32_t)r.vstride, cx = q - cy * (uint32_t)r.vstride;
    const int s = r.vdiv, gx = r.x0 + (int)cx * s, gy = r.y0 + (int)cy * s;
    const int ax = max(gx, 0), ay = max(gy, 0), bx = min(min(gx + s, r.x1), P.W), by = min(min(gy + s, r.y1), P.H);  // the cell, in the box, in the plane
    if (bx <= ax || by <= ay) return;  // m = 0: never referenced (the whole workgroup leaves)
    unsigned long long a[NC] = {};
    for (int y = ay + (int)(threadIdx.x >> 6); y < by; y += 4)
        for (int x = ax + (int)(threadIdx.x & 63); x < bx; x += 64) {
            uint32_t v[NC];
            planes::load(P.c, NC, x, y, P.spair, v);
#pragma unroll
            for (int c = 0; c < NC; ++c) a[c] += v[c];
        }
#pragma unroll
    for (int c = 0; c < NC; ++c) part[c][threadIdx.x] = a[c];
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int c = 0; c < NC; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long m = (unsigned long long)(bx - ax) * (unsigned long long)(by - ay);
        for (int c = 0; c < NC; ++c) values[(r.val_at + q) * NC + c] = (uint8_t)((2 * part[c][0] + m) / (2 * m));
    }
}

// ---- blur -----------------------------------------------------------------------------------------------------------------------------------
// Horizontal pass.  One workgroup per (head, row of h, 256-sample segment of the clipped box): the segment's source samples and r either side, columns clamped
// to the plane, staged in LDS; lane t then sums sample t of the segment.  The sum is at most 65536 * 255.  A dense luma row is staged four samples a lane:
// the line starts `lead` bytes early, at the aligned dword below the first sample, and every dword that lies wholly inside the row is one aligned load.
template <int NC>
__global__ __launch_bounds__(256) void blur_rows_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ segments, int n, const int32_t* __restrict__ taps, View<NC> P,
                                                        uint16_t* __restrict__ h) {
    __shared__ __attribute__((aligned(4))) uint8_t line[(LINE_SAMPLES + 4) * NC];
    const int i = head_of(segments, n, blockIdx.x);
    const HeadRow r = rows[i];
    const int cw = r.cx1 - r.cx0;
    const uint32_t q = blockIdx.x - segments[i], across = (uint32_t)(cw + SEGMENT - 1) / SEGMENT, row = q / across, seg = q - row * across;
    const int y = r.hy0 + (int)row, sx = r.cx0 + (int)seg * SEGMENT, samples = min(SEGMENT, r.cx1 - sx), rad = r.radius;
    int lead = 0;
    if (NC == 1 && P.c[0].sstep == 1) {
        const uint8_t* from = P.c[0].src + (int64_t)y * P.c[0].spitch;
        lead = (int)(((uintptr_t)from + (uintptr_t)(intptr_t)(sx - rad)) & 3);  // (sx - rad may be negative: the address is only looked at)
        const int first = sx - rad - lead;                 // the column of line[0]; from + first is 4-byte aligned
        for (int p = 4 * (int)threadIdx.x; p < lead + samples + 2 * rad; p += 1024) {
            const int gx = first + p;
            if (gx >= 0 && gx + 3 < P.W) {
                *reinterpret_cast<uint32_t*>(line + p) = *reinterpret_cast<const uint32_t*>(from + gx);
            } else {
                for (int b = 0; b < 4; ++b) line[p + b] = from[min(max(gx + b, 0), P.W - 1)];
            }
        }
    } else {
        for (int j = threadIdx.x; j < samples + 2 * rad; j += 256) {
            uint32_t v[NC];
            planes::load(P.c, NC, min(max(sx - rad + j, 0), P.W - 1), y, P.spair, v);
#pragma unroll
            for (int c = 0; c < NC; ++c) line[j * NC + c] = (uint8_t)v[c];
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= samples) return;
    const int32_t* tap = taps + r.tap_at;
    const uint8_t* mid = line + (lead + t + rad) * NC;
    uint32_t a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = (uint32_t)tap[0] * mid[c];
    for (int k = 1; k <= rad; ++k) {
        const uint32_t w = (uint32_t)tap[k];
        const uint8_t *l = mid - NC * k, *g = mid + NC * k;
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] += w * ((uint32_t)l[c] + g[c]);
    }
    uint16_t* o = h + (r.h_at + (int64_t)row * cw + (sx - r.cx0 + t)) * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = (uint16_t)((a[c] + 128u) >> 8);
}

// Vertical pass.  One lane per sample of the clipped box, a wave along a row, so that every tap reads a row of h coalesced over the columns.  Only the samples
// the head owns are computed: no other value is ever looked up.  The sum stays below 65536 * 65280 + 2^23 < 2^32.
template <int NC>
__global__ __launch_bounds__(256) void blur_cols_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ tiles, int n, const int32_t* __restrict__ taps,
                                                        const int32_t* __restrict__ owner, int LW, int LH, int PH, const uint16_t* __restrict__ h, uint8_t* __restrict__ values) {
    const int i = head_of(tiles, n, blockIdx.x);
    const HeadRow r = rows[i];
    int x, y;
    if (!tile_sample(r, blockIdx.x - tiles[i], x, y)) return;
    if (!owned_by<NC>(owner, LW, LH, n, x, y, i)) return;
    const int cw = r.cx1 - r.cx0;
    const int32_t* tap = taps + r.tap_at;
    const uint16_t* col = h + (r.h_at + (int64_t)(x - r.cx0)) * NC;  // row yy of the plane is row yy - hy0 of h; clamp(y +- k) stays inside hy0 .. hy1 - 1
    uint32_t a[NC] = {};
    for (int k = -r.radius; k <= r.radius; ++k) {
        const uint32_t w = (uint32_t)tap[abs(k)];
        const uint16_t* p = col + (int64_t)(min(max(y + k, 0), PH - 1) - r.hy0) * cw * NC;
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] += w * p[c];
    }
    uint8_t* o = values + (r.val_at + (int64_t)(y - r.cy0) * cw + (x - r.cx0)) * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = (uint8_t)((a[c] + (1u << 23)) >> 24);
}

// ---- write ----------------------------------------------------------------------------------------------------------------------------------
// One lane per sample of every head's clipped box: the sample is stored if the head owns it (the clipped box is the part of the geometry box in the plane, so
// "inside its owner's box" holds by construction).  Nothing else of the destination is touched.
template <int NC>
__global__ __launch_bounds__(256) void write_kernel(const HeadRow* __restrict__ rows, const uint32_t* __restrict__ tiles, int n, const int32_t* __restrict__ owner, int LW, int LH,
                                                    const uint8_t* __restrict__ values, int fill, uint32_t colour, View<NC> P) {
    const int i = head_of(tiles, n, blockIdx.x);
    const HeadRow r = rows[i];
    int x, y;
    if (!tile_sample(r, blockIdx.x - tiles[i], x, y)) return;
    if (!owned_by<NC>(owner, LW, LH, n, x, y, i)) return;
    uint32_t v[NC];
    if (fill) {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = (colour >> (8 * c)) & 255u;
    } else {
        const uint8_t* p = values + (r.val_at + (int64_t)((y - r.vy0) / r.vdiv) * r.vstride + (x - r.vx0) / r.vdiv) * NC;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = p[c];
    }
    planes::store(P.c, NC, x, y, P.dpair, v);
}

// ---- the host half: every check and every offset, no HIP call -----------------------------------------------------------------------------------
struct Plan {
    GroupPlan luma, chroma;
    int64_t values_l = 0, values_c = 0, h_l = 0, h_c = 0, total = 0;  // byte offsets in the workspace (the owner plane, if painted, is at 0)
    bool in_place[3] = {false, false, false};
    int spair = 0, dpair = 0;
};

const char* const PLANE_NAMES[3] = {"Y", "U", "V"};

// `who` words the messages: the two entry points share every check of the job
int make_plan(const vghy_anonymize_job* job, Plan& p, const char* who) {
    CH_REQUIRE(job, "%s: null job", who);
    const vghy_anonymize_job& j = *job;
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHY_MAX_SIDE && j.width <= VGHY_MAX_SIDE, "%s: frame %d x %d outside 1 .. %d", who, j.height, j.width, VGHY_MAX_SIDE);
    const int64_t H = j.height, W = j.width, CH = (H + 1) / 2, CW = (W + 1) / 2;
    const int64_t pw[3] = {W, CW, CW}, ph[3] = {H, CH, CH};
    char why[400];
    for (int k = 0; k < 3; ++k) CH_REQUIRE(!planes::check_plane(j.planes[k], pw[k], 2, who, PLANE_NAMES[k], why, sizeof(why)), "%s", why);
    CH_REQUIRE(!planes::check_overlap(j.planes, 3, pw, ph, who, PLANE_NAMES, why, sizeof(why)), "%s", why);
    for (int k = 0; k < 3; ++k) p.in_place[k] = planes::in_place(j.planes[k]);
    CH_REQUIRE(j.n_heads >= 0 && j.n_heads <= VGHY_MAX_HEADS, "%s: n_heads %d outside 0 .. %d", who, j.n_heads, VGHY_MAX_HEADS);
    CH_REQUIRE(j.method >= VGHY_METHOD_FILL && j.method <= VGHY_METHOD_BLUR, "%s: unknown method %d", who, j.method);
    CH_REQUIRE(j.region >= VGHY_REGION_BOX && j.region <= VGHY_REGION_MAP, "%s: unknown region %d", who, j.region);
    CH_REQUIRE((j.color & ~0xffffff) == 0, "%s: color 0x%x has more than three bytes", who, (unsigned)j.color);
    CH_REQUIRE(j.reserved == 0, "%s: reserved is %d, not 0", who, j.reserved);
    CH_REQUIRE((j.region == VGHY_REGION_MAP) == (j.owner_dev != nullptr), "%s: owner_dev is %s for region %d (needed by VGHY_REGION_MAP alone)", who, j.owner_dev ? "set" : "null", j.region);
    CH_REQUIRE(((uintptr_t)j.owner_dev & 15) == 0, "%s: owner_dev %p is not 16-byte aligned", who, (const void*)j.owner_dev);
    const int n = j.n_heads;
    const bool blur = j.method == VGHY_METHOD_BLUR;
    CH_REQUIRE(n == 0 || (j.luma_heads && j.chroma_heads), "%s: null heads (luma_heads %p, chroma_heads %p)", who, (const void*)j.luma_heads, (const void*)j.chroma_heads);
    CH_REQUIRE(j.n_taps >= 0, "%s: n_taps %d is negative", who, j.n_taps);
    if (blur && n) CH_REQUIRE(j.taps && j.n_taps >= 1, "%s: blur needs a tap table (taps %p, n_taps %d)", who, (const void*)j.taps, j.n_taps);
    if (int rc = plan_heads(j.luma_heads, n, j.method, j.taps, j.n_taps, W, H, p.luma, who, "luma head")) return rc;
    if (int rc = plan_heads(j.chroma_heads, n, j.method, j.taps, j.n_taps, CW, CH, p.chroma, who, "chroma head")) return rc;
    p.spair = planes::pair_of(j.planes[1].src_dev, j.planes[2].src_dev, j.planes[1].src_pitch, j.planes[2].src_pitch, j.planes[1].src_step, j.planes[2].src_step);
    p.dpair = planes::pair_of(j.planes[1].dst_dev, j.planes[2].dst_dev, j.planes[1].dst_pitch, j.planes[2].dst_pitch, j.planes[1].dst_step, j.planes[2].dst_step);
    p.values_l = up16(j.region == VGHY_REGION_MAP ? 0 : 4 * H * W);
    p.values_c = up16(p.values_l + p.luma.n_values);
    p.h_l = up16(p.values_c + 2 * p.chroma.n_values);
    p.h_c = up16(p.h_l + 2 * p.luma.n_h);
    p.total = up16(p.h_c + 4 * p.chroma.n_h);
    if (p.total < 16) p.total = 16;
    return OK;
}

std::mutex g_mutex;
std::map<int, Staging> g_staging;  // per device: the head rows, the prefix sums and the taps of one call

}  // namespace

extern "C" VGHY_API const char* vghy_version(void) { return "vghvideo 1 (gfx950)"; }
extern "C" VGHY_API const char* vghy_last_error(void) { return last_error(); }

extern "C" VGHY_API int64_t vghy_anonymize_workspace_bytes(const vghy_anonymize_job* job) {
    Plan p;
    return make_plan(job, p, "anonymize_workspace_bytes") == OK ? p.total : 0;
}

extern "C" VGHY_API int vghy_anonymize(const vghy_anonymize_job* job, void* workspace_dev, void* stream) {
    Plan p;
    // everything is checked before anything is allocated, written or queued
    if (int rc = make_plan(job, p, "anonymize")) return rc;
    CH_REQUIRE(workspace_dev, "anonymize: null workspace");
    CH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "anonymize: workspace is not 16-byte aligned");
    const vghy_anonymize_job& j = *job;
    const int n = j.n_heads, W = j.width, H = j.height, CW = (W + 1) / 2, CH = (H + 1) / 2;
    const bool blur = j.method == VGHY_METHOD_BLUR, pixelate = j.method == VGHY_METHOD_PIXELATE, paint = j.region != VGHY_REGION_MAP;
    const int fill = j.method == VGHY_METHOD_FILL;
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    // one upload: [luma: the rows and their prefix sums | chroma: the same | taps], each from a 16-byte boundary
    const size_t at_taps = 2 * group_bytes(n), total = align16(at_taps + (blur ? (size_t)j.n_taps * 4 : 0));
    if (int rc = reserve(s, total, "anonymize")) return rc;  // also waits for this device's previous call
    const GroupOnDevice gl = stage_group(p.luma, s, 0), gc = stage_group(p.chroma, s, group_bytes(n));
    if (blur && j.n_taps) memcpy(s.host + at_taps, j.taps, (size_t)j.n_taps * 4);
    // from here on work is queued (companion_host.h, queue-then-record)
    const int32_t* taps = (const int32_t*)(s.dev + at_taps);
    uint8_t* ws = (uint8_t*)workspace_dev;
    int32_t* painted = (int32_t*)ws;
    const int32_t* owner = paint ? painted : j.owner_dev;
    View<1> luma{{planes::chan_of(j.planes[0])}, W, H, 0, 0};
    View<2> chroma{{planes::chan_of(j.planes[1]), planes::chan_of(j.planes[2])}, CW, CH, p.spair, p.dpair};
    uint8_t *values_l = ws + p.values_l, *values_c = ws + p.values_c;
    uint16_t *h_l = (uint16_t*)(ws + p.h_l), *h_c = (uint16_t*)(ws + p.h_c);
    const uint32_t tiles_l = p.luma.tiles[(size_t)n], tiles_c = p.chroma.tiles[(size_t)n];
    Queue q;
    CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));
    if (paint) {
        CH_QUEUE(q, hipMemsetAsync(painted, 0xff, (size_t)W * (size_t)H * 4, st));  // -1 everywhere
        if (tiles_l && q.ok()) hipLaunchKernelGGL(paint_owner_kernel, dim3(tiles_l), dim3(256), 0, st, gl.rows, gl.tiles, n, painted, W, (int)(j.region == VGHY_REGION_ELLIPSE));
    }
    if (pixelate && q.ok()) {
        if (const uint32_t c = p.luma.cells[(size_t)n]) hipLaunchKernelGGL(cells_kernel<1>, dim3(c), dim3(256), 0, st, gl.rows, gl.cells, n, luma, values_l);
        if (const uint32_t c = p.chroma.cells[(size_t)n]) hipLaunchKernelGGL(cells_kernel<2>, dim3(c), dim3(256), 0, st, gc.rows, gc.cells, n, chroma, values_c);
    }
    if (blur && q.ok()) {
        if (const uint32_t g = p.luma.segments[(size_t)n]) {
            hipLaunchKernelGGL(blur_rows_kernel<1>, dim3(g), dim3(256), 0, st, gl.rows, gl.segments, n, taps, luma, h_l);
            hipLaunchKernelGGL(blur_cols_kernel<1>, dim3(tiles_l), dim3(256), 0, st, gl.rows, gl.tiles, n, taps, owner, W, H, H, (const uint16_t*)h_l, values_l);
        }
        if (const uint32_t g = p.chroma.segments[(size_t)n]) {
            hipLaunchKernelGGL(blur_rows_kernel<2>, dim3(g), dim3(256), 0, st, gc.rows, gc.segments, n, taps, chroma, h_c);
            hipLaunchKernelGGL(blur_cols_kernel<2>, dim3(tiles_c), dim3(256), 0, st, gc.rows, gc.tiles, n, taps, owner, W, H, CH, (const uint16_t*)h_c, values_c);
        }
    }
    if (q.ok()) {  // the planes that are out of place: every sample copied, an interleaved pair that stays one as one plane of 2 CW bytes
        if (!p.in_place[0]) hipLaunchKernelGGL(planes::copy_kernel, dim3((W + 1023) / 1024, H), dim3(256), 0, st, luma.c[0].src, luma.c[0].spitch, 1 * luma.c[0].sstep, luma.c[0].dst, luma.c[0].dpitch, 1 * luma.c[0].dstep, W);
        if (!p.in_place[1] && !p.in_place[2] && p.spair && p.spair == p.dpair) {
            const planes::Chan& lo = chroma.c[p.spair - 1];
            hipLaunchKernelGGL(planes::copy_kernel, dim3((2 * CW + 1023) / 1024, CH), dim3(256), 0, st, lo.src, lo.spitch, 1, lo.dst, lo.dpitch, 1, 2 * CW);
        } else {
            for (int k = 0; k < 2; ++k)
                if (!p.in_place[1 + k]) hipLaunchKernelGGL(planes::copy_kernel, dim3((CW + 1023) / 1024, CH), dim3(256), 0, st, chroma.c[k].src, chroma.c[k].spitch, chroma.c[k].sstep, chroma.c[k].dst, chroma.c[k].dpitch, chroma.c[k].dstep, CW);
        }
    }
    if (q.ok()) {
        if (tiles_l) hipLaunchKernelGGL(write_kernel<1>, dim3(tiles_l), dim3(256), 0, st, gl.rows, gl.tiles, n, owner, W, H, (const uint8_t*)values_l, fill, (uint32_t)j.color & 255u, luma);
        if (tiles_c) hipLaunchKernelGGL(write_kernel<2>, dim3(tiles_c), dim3(256), 0, st, gc.rows, gc.tiles, n, owner, W, H, (const uint8_t*)values_c, fill, (uint32_t)j.color >> 8, chroma);
    }
    return finish(q, s, true, st, "anonymize");
}
