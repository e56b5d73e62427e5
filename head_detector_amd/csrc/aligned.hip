// libvghview.so (include/vgh_view.h): aligned head crops = PredictionResult.get_aligned_heads (head_detector/detection_result.py:56-70,
// head_detector/utils.py:109-117) without the per-head copy and whole-image warp of the reference: ONE launch computes only the pixels of
// every head's crop.
// The arithmetic is OpenCV's 8-bit warpAffine(..., INTER_LINEAR) with the constant-0 border (imgproc/src/imgwarp.cpp, WarpAffineInvoker +
// remapBilinear<FixedPtCast<int, uchar, 15>>): the host supplies the int32 tables adelta / bdelta / X0 / Y0 of the crop's columns and rows
// (head_detector_amd/aligned.py builds them in double as imgwarp.cpp does), the kernel is integer arithmetic only:
//   X = (X0[y] + adelta[x]) >> 5, Y likewise; source pixel (X >> 5, Y >> 5), fractions X & 31, Y & 31; weights 32 * {(32-fx)(32-fy), fx(32-fy),
//   (32-fx)fy, fx fy} (sum 2^15); taps outside the source read 0; (sum + 2^14) >> 15.
// PARITY UNPINNED against cv2 itself (absent from this image); bit-exact against tests/warp_affine_ref.py.
// Self-contained on purpose: no csrc/vgh_internal.h, no object of libvgh.so (csrc/companion_host.h is what the companion libraries' sources share); built with -fvisibility=hidden, only the vghv_* functions are exported.
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_view.h"
#include "companion_host.h"

namespace {

using namespace companion;
static_assert(VGHV_OK == OK && VGHV_ERR_INVALID == ERR_INVALID && VGHV_ERR_HIP == ERR_HIP && VGHV_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

// device-side descriptor of one crop
struct Crop {
    const uint8_t* src;  // [src_h, src_w, 3] u8, rows src_pitch bytes apart
    int64_t src_pitch;
    int64_t dst_off;  // byte offset of the dense [crop_h, crop_w, 3] result
    int32_t src_h, src_w, crop_w, crop_h;
    int32_t tab;  // this crop's [adelta(crop_w) | bdelta(crop_w) | X0(crop_h) | Y0(crop_h)] in the table array
    int32_t pad_;
};

// one 32 x 8 pixel tile of one crop: what blockIdx.x maps to
struct Tile {
    int32_t crop;
    uint32_t xy;  // tile column | tile row << 16
};

constexpr int TILE_W = 32, TILE_H = 8;

// global-address-space views: pointers read from a descriptor in memory would otherwise be accessed with flat instructions
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gmem(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}

// One output pixel per lane, like letterbox_batch_kernel (csrc/letterbox.hip): this class of kernel is bound by its byte gathers, not by its
// stores.  The tile and its crop descriptor are wave-uniform (scalar loads).  The host clipped every crop to the warped canvas, so there is
// no destination-side clipping beyond the tile's ragged edge; source-side taps outside the image get weight 0 and a clamped (in-bounds) address.
__global__ __launch_bounds__(256) void warp_crops_kernel(const Crop* __restrict__ crops, const Tile* __restrict__ tiles, const int32_t* __restrict__ tables,
                                                         uint8_t* __restrict__ dst) {
    const Tile t = tiles[blockIdx.x];
    const Crop& c = crops[t.crop];
    const int x = (t.xy & 0xffff) * TILE_W + (threadIdx.x & (TILE_W - 1)), y = (int)(t.xy >> 16) * TILE_H + (threadIdx.x >> 5);
    const int cw = c.crop_w, ch = c.crop_h;
    if (x >= cw || y >= ch) return;
    const auto tab = gmem(tables) + c.tab;
    // unsigned sums: C's int addition with defined wrap-around (the tables are the caller's)
    const int X = (int)((unsigned)tab[2 * cw + y] + (unsigned)tab[x]) >> 5, Y = (int)((unsigned)tab[2 * cw + ch + y] + (unsigned)tab[cw + x]) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int W = c.src_w, H = c.src_h;
    const bool x0in = (unsigned)sx < (unsigned)W, x1in = (unsigned)(sx + 1) < (unsigned)W;
    const bool y0in = (unsigned)sy < (unsigned)H, y1in = (unsigned)(sy + 1) < (unsigned)H;
    const int w00 = (x0in && y0in) ? 32 * (32 - fx) * (32 - fy) : 0, w01 = (x1in && y0in) ? 32 * fx * (32 - fy) : 0;
    const int w10 = (x0in && y1in) ? 32 * (32 - fx) * fy : 0, w11 = (x1in && y1in) ? 32 * fx * fy : 0;
    const int cx0 = min(max(sx, 0), W - 1) * 3, cx1 = min(max(sx + 1, 0), W - 1) * 3;
    const auto r0 = gmem(c.src) + (size_t)min(max(sy, 0), H - 1) * c.src_pitch, r1 = gmem(c.src) + (size_t)min(max(sy + 1, 0), H - 1) * c.src_pitch;
    uint8_t* o = dst + c.dst_off + ((size_t)y * cw + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = (int)r0[cx0 + k] * w00 + (int)r0[cx1 + k] * w01 + (int)r1[cx0 + k] * w10 + (int)r1[cx1 + k] * w11;  // <= 255 * 2^15
        o[k] = (uint8_t)((v + (1 << 14)) >> 15);
    }
}

// ---- staging: descriptors + tile list + tables of one call (companion_host.h) ----------------------------------------------------------
std::mutex g_mutex;
std::map<int, Staging> g_staging;

}  // namespace

extern "C" VGHV_API const char* vghv_version(void) { return "vghview 2 (gfx950)"; }

extern "C" VGHV_API const char* vghv_last_error(void) { return last_error(); }

extern "C" VGHV_API int vghv_warp_crops(const vghv_crop* crops, int n, const int32_t* tables, int64_t n_tables, uint8_t* dst_dev, int64_t dst_bytes, void* stream) {
    CH_REQUIRE(n >= 0 && n_tables >= 0 && dst_bytes >= 0, "warp_crops: negative count");
    if (n == 0) return OK;
    CH_REQUIRE(crops && tables, "warp_crops: null argument");
    CH_REQUIRE(n_tables <= INT32_MAX, "warp_crops: %lld table entries exceed 2^31 - 1", (long long)n_tables);
    int64_t n_tiles = 0;
    for (int i = 0; i < n; ++i) {  // everything is checked before anything is allocated, written or queued
        const vghv_crop& c = crops[i];
        CH_REQUIRE(c.src_dev, "warp_crops: crop %d: null src_dev", i);
        CH_REQUIRE(c.src_channels == 3, "warp_crops: crop %d: %d channels (needs 3: u8 RGB)", i, c.src_channels);
        CH_REQUIRE(c.src_h >= 1 && c.src_w >= 1 && c.src_h <= VGHV_MAX_SIDE && c.src_w <= VGHV_MAX_SIDE, "warp_crops: crop %d: source %d x %d outside 1 .. %d", i, c.src_h,
                   c.src_w, VGHV_MAX_SIDE);
        CH_REQUIRE(c.src_pitch_bytes >= (int64_t)c.src_w * 3, "warp_crops: crop %d: src_pitch_bytes %lld < src_w * 3 = %lld", i, (long long)c.src_pitch_bytes,
                   (long long)c.src_w * 3);
        CH_REQUIRE(c.crop_w >= 0 && c.crop_h >= 0 && c.crop_w <= 65535 * TILE_W && c.crop_h <= 65535 * TILE_H, "warp_crops: crop %d: bad size %d x %d", i, c.crop_w, c.crop_h);
        if (c.crop_w == 0 || c.crop_h == 0) continue;
        const int64_t need_tab = 2 * (int64_t)c.crop_w + 2 * (int64_t)c.crop_h, need_dst = (int64_t)c.crop_w * c.crop_h * 3;
        CH_REQUIRE(c.table_offset >= 0 && c.table_offset <= n_tables - need_tab, "warp_crops: crop %d: tables [%lld, +%lld) outside the %lld supplied", i,
                   (long long)c.table_offset, (long long)need_tab, (long long)n_tables);
        CH_REQUIRE(dst_dev && c.dst_offset >= 0 && c.dst_offset <= dst_bytes - need_dst, "warp_crops: crop %d: result [%lld, +%lld) outside the %lld destination bytes", i,
                   (long long)c.dst_offset, (long long)need_dst, (long long)dst_bytes);
        n_tiles += (int64_t)((c.crop_w + TILE_W - 1) / TILE_W) * ((c.crop_h + TILE_H - 1) / TILE_H);
    }
    if (n_tiles == 0) return OK;
    CH_REQUIRE(n_tiles <= INT32_MAX, "warp_crops: %lld tiles exceed one launch", (long long)n_tiles);

    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    const size_t at_tiles = align16((size_t)n * sizeof(Crop)), at_tab = align16(at_tiles + (size_t)n_tiles * sizeof(Tile));
    const size_t total = at_tab + (size_t)n_tables * sizeof(int32_t);
    if (int rc = reserve(s, total, "warp_crops")) return rc;
    Crop* hc = (Crop*)s.host;
    Tile* ht = (Tile*)(s.host + at_tiles);
    for (int i = 0; i < n; ++i) {
        const vghv_crop& c = crops[i];
        Crop& d = hc[i];
        d.src = c.src_dev;
        d.src_pitch = c.src_pitch_bytes;
        d.dst_off = c.dst_offset;
        d.src_h = c.src_h;
        d.src_w = c.src_w;
        d.crop_w = c.crop_w;
        d.crop_h = c.crop_h;
        d.tab = (int32_t)c.table_offset;
        d.pad_ = 0;
        if (c.crop_w == 0 || c.crop_h == 0) continue;
        const int tx = (c.crop_w + TILE_W - 1) / TILE_W, ty = (c.crop_h + TILE_H - 1) / TILE_H;
        for (int j = 0; j < ty; ++j)
            for (int k = 0; k < tx; ++k) *ht++ = Tile{i, (uint32_t)k | (uint32_t)j << 16};
    }
    memcpy(s.host + at_tab, tables, (size_t)n_tables * sizeof(int32_t));
    hipStream_t st = (hipStream_t)stream;
    Queue q;  // from here on work is queued (companion_host.h, queue-then-record)
    CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));
    if (q.ok())
        hipLaunchKernelGGL(warp_crops_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, (const Crop*)s.dev, (const Tile*)(s.dev + at_tiles), (const int32_t*)(s.dev + at_tab), dst_dev);
    return finish(q, s, true, st, "warp_crops");
}
