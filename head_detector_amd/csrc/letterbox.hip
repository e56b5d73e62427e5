// GPU letterbox = HeadDetector._transform_image (head_detector/detector.py:40-52) without the host round trip:
//   cv2.resize(image, (new_w, new_h), INTER_LANCZOS4) -> cv2.copyMakeBorder(..., BORDER_CONSTANT, value=127) -> u8 NHWC canvas that the
//   stem kernel consumes directly (its /255 is fused there, detector.py:51).
// The arithmetic is OpenCV's 8-bit fixed-point path (imgproc/src/resize.cpp: HResizeLanczos4<uchar,int,short> then
// VResizeLanczos4<uchar,int,short, FixedPtCast<int,uchar,22>>): 8x8 taps, weights = saturate_cast<short>(w * 2048) supplied by
// the host (head_detector_amd/letterbox.py builds them exactly as resize.cpp does), int32 accumulation, (v + 2^21) >> 22,
// out-of-range taps replicate the edge pixel.  Integer arithmetic => the 2-D sum can be evaluated per output pixel in any order.
// PARITY UNPINNED against cv2 itself (absent from this image); bit-exact against oracle/letterbox_oracle.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <new>
#include <vector>

#include "letterbox_tables.h"
#include "vgh_internal.h"

namespace {

// Where the resized copy of one source image goes on the S x S canvas, and the tables that resample it: common to every source format.
struct LbGeom {
    const int32_t* xofs;   // [new_w]
    const int16_t* alpha;  // [new_w][8]
    const int32_t* yofs;   // [new_h]
    const int16_t* beta;   // [new_h][8]
    int32_t src_h, src_w, new_w, new_h, pad_x, pad_y;
    uint32_t pad;  // border colour r | g << 8 | b << 16
};

// global-address-space views: pointers read from a descriptor in memory would otherwise be accessed with flat instructions
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gmem(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}

typedef const __attribute__((address_space(1))) uint8_t* gbytes;

// A source format is a descriptor that derives from LbGeom and tells letterbox_pixel how to fetch one tap: col(x) prepares the (clamped) source column x once per
// pixel, row(y) the (clamped) source row y once per tap row, tap(row, col, r, g, b) reads the tap as three bytes' worth of int.

// RGB: kernel argument of vgh_letterbox, device-side descriptor of the batched kernel for VGH_IMG_U8_RAW.
struct LbImage : LbGeom {
    const uint8_t* src;  // [src_h, src_w, src_cn >= 3] u8, row stride src_pitch bytes
    int64_t src_pitch;
    int32_t src_cn;
    typedef gbytes Row;
    __device__ __forceinline__ int col(int x) const { return x * src_cn; }
    __device__ __forceinline__ Row row(int y) const { return gmem(src) + (size_t)y * src_pitch; }
    __device__ __forceinline__ void tap(Row p, int c, int& r, int& g, int& b) const {
        r = p[c];
        g = p[c + 1];
        b = p[c + 2];
    }
};

// YUV 4:2:0 (VGH_IMG_YUV420_RAW): the tap is converted by the rule of include/vgh.h (vgh_yuv420_image) and clamped to bytes BEFORE it is weighted.  The chroma
// coordinates derive from the CLAMPED luma coordinates (letterbox_pixel clamps before col() / row()), so (x >> 1, y >> 1) never leaves the ceil-sized chroma planes.
struct LbYuvImage : LbGeom {
    const uint8_t *y, *u, *v;
    int64_t y_pitch, uv_pitch;
    int32_t chroma_step, y_offset, cy, crv, cgu, cgv, cbu;
    struct Row {
        gbytes y, u, v;
    };
    __device__ __forceinline__ int col(int x) const { return x; }
    __device__ __forceinline__ Row row(int yy) const {
        const size_t c = (size_t)(yy >> 1) * uv_pitch;
        return Row{gmem(y) + (size_t)yy * y_pitch, gmem(u) + c, gmem(v) + c};
    }
    __device__ __forceinline__ void tap(const Row& p, int x, int& r, int& g, int& b) const {
        const int cx = (x >> 1) * chroma_step;
        const int l = cy * ((int)p.y[x] - y_offset) + 32768, d = (int)p.u[cx] - 128, e = (int)p.v[cx] - 128;
        // each channel is shifted and clamped into an int of its own and goes straight into a multiply: no clamp-and-pack chain (see the note at the end of letterbox_pixel)
        r = min(max((l + crv * e) >> 16, 0), 255);
        g = min(max((l + cgu * d + cgv * e) >> 16, 0), 255);
        b = min(max((l + cbu * d) >> 16, 0), 255);
    }
};

// Deep YUV 4:2:0 (VGH_IMG_YUV420P16_RAW: 10 or 12 significant bits in 16-bit words): LbYuvImage's fetch with 16-bit loads, a shift and a mask in front of the rule of
// include/vgh.h (vgh_yuv420p16_image); the tap is clamped to BYTES before it is weighted, so everything behind the fetch is the 8-bit path.  The host half
// (set_source) has turned the descriptor's depth into mask / half / round / rshift and its chroma step into words; pointers and pitches are even (check_source), so
// every load is an aligned 16-bit load.  Chroma coordinates derive from the CLAMPED luma coordinates, as above.
typedef const __attribute__((address_space(1))) uint16_t* gwords;

struct LbYuv16Image : LbGeom {
    const uint16_t *y, *u, *v;
    int64_t y_pitch, uv_pitch;  // bytes
    int32_t chroma_step;        // WORDS between chroma samples of a row: 1 or 2
    int32_t shift, mask, half, round, rshift;  // sample = (word >> shift) & mask; half = 2^(D-1), round = 2^(D+7), rshift = D + 8
    int32_t y_offset, cy, crv, cgu, cgv, cbu;
    struct Row {
        gwords y, u, v;
    };
    __device__ __forceinline__ int col(int x) const { return x; }
    __device__ __forceinline__ Row row(int yy) const {
        const size_t c = (size_t)(yy >> 1) * uv_pitch;
        return Row{(gwords)((gbytes)gmem(y) + (size_t)yy * y_pitch), (gwords)((gbytes)gmem(u) + c), (gwords)((gbytes)gmem(v) + c)};
    }
    __device__ __forceinline__ void tap(const Row& p, int x, int& r, int& g, int& b) const {
        const int cx = (x >> 1) * chroma_step;
        const int yv = ((int)p.y[x] >> shift) & mask, uv = ((int)p.u[cx] >> shift) & mask, vv = ((int)p.v[cx] >> shift) & mask;
        const int l = cy * (yv - y_offset) + round, d = uv - half, e = vv - half;
        // as in LbYuvImage: each channel shifted and clamped into an int of its own, no clamp-and-pack chain (see the note at the end of letterbox_pixel)
        r = min(max((l + crv * e) >> rshift, 0), 255);
        g = min(max((l + cgu * d + cgv * e) >> rshift, 0), 255);
        b = min(max((l + cbu * d) >> rshift, 0), 255);
    }
};

// Canvas pixel (x, y) as r | g << 8 | b << 16: the per-pixel arithmetic of ALL letterbox kernels (they cannot drift apart); generic over the tap fetch.
template <typename Img>
__device__ __forceinline__ uint32_t letterbox_pixel(const Img& a, int x, int y) {
    const int dx = x - a.pad_x, dy = y - a.pad_y;
    if ((unsigned)dx >= (unsigned)a.new_w || (unsigned)dy >= (unsigned)a.new_h) return a.pad;
    const int sx = gmem(a.xofs)[dx] - 3, sy = gmem(a.yofs)[dy] - 3;
    int al[8], cx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        al[k] = gmem(a.alpha)[dx * 8 + k];
        cx[k] = a.col(min(max(sx + k, 0), a.src_w - 1));
    }
    unsigned acc[3] = {0u, 0u, 0u};  // unsigned: C's int accumulation with defined wrap-around
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ry = min(max(sy + j, 0), a.src_h - 1);
        const auto row = a.row(ry);
        unsigned h0 = 0u, h1 = 0u, h2 = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int p0, p1, p2;
            a.tap(row, cx[k], p0, p1, p2);
            h0 += (unsigned)(p0 * al[k]);
            h1 += (unsigned)(p1 * al[k]);
            h2 += (unsigned)(p2 * al[k]);
        }
        const int b = gmem(a.beta)[dy * 8 + j];
        acc[0] += (unsigned)((int)h0 * b);
        acc[1] += (unsigned)((int)h1 * b);
        acc[2] += (unsigned)((int)h2 * b);
    }
    // each channel clamped into a byte of its own, then packed: written as one shift / clamp / or chain, hipcc (ROCm 7.0) lowers two channels
    // to v_ashr_pk_u8_i32 on gfx950, and the device then returned wrong red / blue bytes (measured against oracle/letterbox_oracle.py)
    uint8_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = ((int)acc[c] + (1 << 21)) >> 22;  // FixedPtCast<int, uchar, 22>
        o[c] = (uint8_t)min(max(v, 0), 255);
    }
    return (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16;
}

__global__ __launch_bounds__(256) void letterbox_kernel(LbImage a, uint8_t* dst, int S) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= S || y >= S) return;
    uint8_t* o = dst + ((size_t)y * S + x) * 3;
    const uint32_t rgb = letterbox_pixel(a, x, y);
    o[0] = (uint8_t)rgb;
    o[1] = (uint8_t)(rgb >> 8);
    o[2] = (uint8_t)(rgb >> 16);
}

// VGH_IMG_U8_RAW / VGH_IMG_YUV420_RAW / VGH_IMG_YUV420P16_RAW: every image of an arena chunk in one launch, canvas [n, S, S, 3]; one instantiation per source format (a call has ONE format,
// so no lane branches on it).  blockIdx.z = image (its descriptor is wave-uniform: scalar loads); one pixel per lane as in letterbox_kernel.  The RGB kernel is bound
// by the 128 byte gathers per pixel, not by its stores: four pixels per lane with one 3-dword store measured 1.70 ms per 64 mixed photographs against 1.16 ms for this
// form (profiles/raw_letterbox_l64.txt).
template <typename Img>
__global__ __launch_bounds__(256) void letterbox_batch_kernel(const Img* __restrict__ imgs, uint8_t* __restrict__ canvas, int S) {
    const Img& a = imgs[blockIdx.z];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= S || y >= S) return;
    uint8_t* o = canvas + (((size_t)blockIdx.z * S + y) * S + x) * 3;
    const uint32_t rgb = letterbox_pixel(a, x, y);
    o[0] = (uint8_t)rgb;
    o[1] = (uint8_t)(rgb >> 8);
    o[2] = (uint8_t)(rgb >> 16);
}

}  // namespace

extern "C" int vgh_letterbox(const uint8_t* src_dev, int src_h, int src_w, int src_channels, int64_t src_pitch_bytes, const int32_t* xofs_dev,
                             const int16_t* alpha_dev, const int32_t* yofs_dev, const int16_t* beta_dev, int new_w, int new_h, int pad_x, int pad_y,
                             const uint8_t* pad_rgb, uint8_t* dst_dev, int S, void* stream) {
    VGH_REQUIRE(src_dev && xofs_dev && alpha_dev && yofs_dev && beta_dev && dst_dev && pad_rgb, "letterbox: null argument");
    VGH_REQUIRE(src_h > 0 && src_w > 0 && src_channels >= 3 && src_pitch_bytes >= (int64_t)src_w * src_channels, "letterbox: bad source geometry");
    VGH_REQUIRE(new_w > 0 && new_h > 0 && pad_x >= 0 && pad_y >= 0 && pad_x + new_w <= S && pad_y + new_h <= S, "letterbox: the resized image does not fit the %dx%d canvas", S, S);
    LbImage a;
    a.src = src_dev;
    a.src_h = src_h;
    a.src_w = src_w;
    a.src_cn = src_channels;
    a.src_pitch = src_pitch_bytes;
    a.xofs = xofs_dev;
    a.alpha = alpha_dev;
    a.yofs = yofs_dev;
    a.beta = beta_dev;
    a.new_w = new_w;
    a.new_h = new_h;
    a.pad_x = pad_x;
    a.pad_y = pad_y;
    a.pad = pad_rgb[0] | (uint32_t)pad_rgb[1] << 8 | (uint32_t)pad_rgb[2] << 16;
    hipLaunchKernelGGL(letterbox_kernel, dim3((S + 31) / 32, (S + 7) / 8), dim3(256), 0, (hipStream_t)stream, a, dst_dev, S);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

// ---- VGH_IMG_U8_RAW / VGH_IMG_YUV420_RAW / VGH_IMG_YUV420P16_RAW: the detector's batched letterbox (include/vgh.h, vgh_detect) -------------------------------------
// The host validates the B descriptors, builds (or finds in its cache) the per-axis tables and packs, for every arena chunk, the chunk's
// LbImage (or LbYuvImage, or LbYuv16Image) descriptors and tables into a pinned staging slot: ONE async copy and ONE letterbox_batch_kernel launch per chunk.  The first slot
// region also holds the un-pad table [max_batch, 3] of the whole call, so it travels with the first chunk's copy.
//
// Two slots, alternating per call.  A slot is free again once its last device reader has run: the letterbox launches of its call (on the
// detector's stream) and, when the select un-pads the FLAME outputs with its table, that select (on the overlap-mode side stream, possibly
// later).  ev[k] is recorded behind each of them (the latest record wins) and the host waits for it before it rewrites slot k -- two calls
// later, so a pipelined caller is normally not held up.  The canvas needs no such guard: see vgh_detector_candidates.
struct vgh_lb_batch {
    int S = 0, max_batch = 0, arena_batch = 0;
    uint8_t* canvas = nullptr;  // [arena_batch, S, S, 3]
    size_t slot_bytes = 0;
    uint8_t* host[2] = {nullptr, nullptr};  // pinned
    uint8_t* dev[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool recorded[2] = {false, false};
    int slot = 1;                  // slot of the last prepared call
    int fmt = VGH_IMG_U8_RAW;      // source format of the last prepared call: which descriptors its slot holds, which kernel reads them
    std::vector<size_t> chunk_at;  // [chunks + 1] byte offsets of the chunk regions in the slot
    std::map<std::pair<int, int>, vgh_lb::AxisTables> cache;  // (src, dst) length -> tables, like letterbox.py's lru_cache
};

namespace {

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

const vgh_lb::AxisTables& cached_tables(vgh_lb_batch* lb, int src, int dst) {
    auto it = lb->cache.find({src, dst});
    if (it != lb->cache.end()) return it->second;
    if (lb->cache.size() >= 256) lb->cache.clear();  // bounded: a stream of ever-new sizes does not grow it without limit
    return lb->cache.emplace(std::make_pair(src, dst), vgh_lb::axis_tables(src, dst)).first->second;
}

void lb_free(vgh_lb_batch* lb) {
    hipFree(lb->canvas);
    for (int k = 0; k < 2; ++k) {
        hipHostFree(lb->host[k]);
        hipFree(lb->dev[k]);
        if (lb->ev[k]) hipEventDestroy(lb->ev[k]);
    }
    delete lb;
}

int lb_create(int S, int max_batch, int arena_batch, vgh_lb_batch** out) {
    vgh_lb_batch* lb = new (std::nothrow) vgh_lb_batch();
    VGH_REQUIRE(lb, "detector_candidates: out of host memory");
    lb->S = S;
    lb->max_batch = max_batch;
    lb->arena_batch = arena_batch;
    // per image at most one descriptor (the largest of the three source formats') + 16 bytes of descriptor region and two axes of <= S entries (4 + 16 bytes, 16-byte
    // aligned): a slot serves every format, so nothing is allocated when the format changes between calls
    const size_t desc_bytes = std::max({sizeof(LbImage), sizeof(LbYuvImage), sizeof(LbYuv16Image)});
    lb->slot_bytes = align16((size_t)max_batch * 12) + (size_t)max_batch * (desc_bytes + 16 + 2 * (align16((size_t)4 * S) + (size_t)16 * S));
    const size_t canvas_bytes = (size_t)arena_batch * S * S * 3;
    bool ok = hipMalloc((void**)&lb->canvas, canvas_bytes) == hipSuccess;
    for (int k = 0; k < 2 && ok; ++k)
        ok = hipHostMalloc((void**)&lb->host[k], lb->slot_bytes, hipHostMallocDefault) == hipSuccess && hipMalloc((void**)&lb->dev[k], lb->slot_bytes) == hipSuccess &&
             hipEventCreateWithFlags(&lb->ev[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        lb_free(lb);
        vgh_set_error("detector_candidates: allocating the letterbox canvas (%zu bytes) and staging (2 x %zu bytes) failed", canvas_bytes, lb->slot_bytes);
        return VGH_ERR_NOMEM;
    }
    *out = lb;
    return VGH_OK;
}

}  // namespace

namespace {

// the source half of a device descriptor from the caller's; the geometry half is filled by vgh_lb_prepare
void set_source(LbImage& a, const vgh_raw_image& im) {
    a.src = im.data_dev;
    a.src_pitch = im.pitch_bytes;
    a.src_cn = im.channels;
}

void set_source(LbYuvImage& a, const vgh_yuv420_image& im) {
    a.y = im.y_dev;
    a.u = im.u_dev;
    a.v = im.v_dev;
    a.y_pitch = im.y_pitch_bytes;
    a.uv_pitch = im.uv_pitch_bytes;
    a.chroma_step = im.chroma_step;
    a.y_offset = im.y_offset;
    a.cy = im.cy;
    a.crv = im.crv;
    a.cgu = im.cgu;
    a.cgv = im.cgv;
    a.cbu = im.cbu;
}

void set_source(LbYuv16Image& a, const vgh_yuv420p16_image& im) {
    a.y = im.y_dev;
    a.u = im.u_dev;
    a.v = im.v_dev;
    a.y_pitch = im.y_pitch_bytes;
    a.uv_pitch = im.uv_pitch_bytes;
    a.chroma_step = im.chroma_step / 2;  // bytes -> words
    a.shift = im.shift;
    a.mask = (1 << im.bit_depth) - 1;
    a.half = 1 << (im.bit_depth - 1);
    a.round = 1 << (im.bit_depth + 7);
    a.rshift = im.bit_depth + 8;
    a.y_offset = im.y_offset;
    a.cy = im.cy;
    a.crv = im.crv;
    a.cgu = im.cgu;
    a.cgv = im.cgv;
    a.cbu = im.cbu;
}

int check_source(const vgh_raw_image& im, int i) {
    VGH_REQUIRE(im.data_dev, "detector_candidates: image %d: null data_dev", i);
    VGH_REQUIRE(im.h >= 1 && im.w >= 1, "detector_candidates: image %d: empty (%d x %d)", i, im.h, im.w);
    VGH_REQUIRE(im.channels >= 3, "detector_candidates: image %d: %d channels (needs >= 3, the first three RGB)", i, im.channels);
    VGH_REQUIRE(im.pitch_bytes >= (int64_t)im.w * im.channels, "detector_candidates: image %d: pitch_bytes %lld < w * channels = %lld", i, (long long)im.pitch_bytes,
                (long long)im.w * im.channels);
    return VGH_OK;
}

int check_source(const vgh_yuv420_image& im, int i) {
    VGH_REQUIRE(im.y_dev && im.u_dev && im.v_dev, "detector_candidates: image %d: null plane (y_dev, u_dev and v_dev are all needed)", i);
    VGH_REQUIRE(im.h >= 1 && im.w >= 1, "detector_candidates: image %d: empty (%d x %d)", i, im.h, im.w);
    VGH_REQUIRE(im.chroma_step == 1 || im.chroma_step == 2, "detector_candidates: image %d: chroma_step %d (1 = planar, 2 = interleaved)", i, im.chroma_step);
    VGH_REQUIRE(im.y_pitch_bytes >= (int64_t)im.w, "detector_candidates: image %d: y_pitch_bytes %lld < w = %d", i, (long long)im.y_pitch_bytes, im.w);
    const int64_t crow = (int64_t)im.chroma_step * (((int64_t)im.w + 1) / 2);
    VGH_REQUIRE(im.uv_pitch_bytes >= crow, "detector_candidates: image %d: uv_pitch_bytes %lld < chroma_step * ((w + 1) / 2) = %lld", i, (long long)im.uv_pitch_bytes,
                (long long)crow);
    VGH_REQUIRE(im.y_offset >= 0 && im.y_offset <= 255, "detector_candidates: image %d: y_offset %d outside 0..255", i, im.y_offset);
    const int32_t coef[5] = {im.cy, im.crv, im.cgu, im.cgv, im.cbu};
    static const char* const names[5] = {"cy", "crv", "cgu", "cgv", "cbu"};
    for (int k = 0; k < 5; ++k)
        VGH_REQUIRE(coef[k] >= -(1 << 20) && coef[k] <= (1 << 20), "detector_candidates: image %d: coefficient %s = %d outside +-2^20", i, names[k], coef[k]);
    return VGH_OK;
}

int check_source(const vgh_yuv420p16_image& im, int i) {
    VGH_REQUIRE(im.y_dev && im.u_dev && im.v_dev, "detector_candidates: image %d: null plane (y_dev, u_dev and v_dev are all needed)", i);
    VGH_REQUIRE(im.h >= 1 && im.w >= 1, "detector_candidates: image %d: empty (%d x %d)", i, im.h, im.w);
    VGH_REQUIRE((((uintptr_t)im.y_dev | (uintptr_t)im.u_dev | (uintptr_t)im.v_dev) & 1) == 0, "detector_candidates: image %d: odd plane pointer (y_dev, u_dev and v_dev address 16-bit words)", i);
    VGH_REQUIRE(im.chroma_step == 2 || im.chroma_step == 4, "detector_candidates: image %d: chroma_step %d bytes (2 = planar, 4 = interleaved)", i, im.chroma_step);
    VGH_REQUIRE((im.y_pitch_bytes & 1) == 0 && im.y_pitch_bytes >= 2 * (int64_t)im.w, "detector_candidates: image %d: y_pitch_bytes %lld is odd or < 2 * w = %lld", i,
                (long long)im.y_pitch_bytes, 2 * (long long)im.w);
    const int64_t crow = (int64_t)im.chroma_step * (((int64_t)im.w + 1) / 2);
    VGH_REQUIRE((im.uv_pitch_bytes & 1) == 0 && im.uv_pitch_bytes >= crow, "detector_candidates: image %d: uv_pitch_bytes %lld is odd or < chroma_step * ((w + 1) / 2) = %lld", i,
                (long long)im.uv_pitch_bytes, (long long)crow);
    VGH_REQUIRE(im.bit_depth == 10 || im.bit_depth == 12, "detector_candidates: image %d: bit_depth %d (10 or 12)", i, im.bit_depth);
    VGH_REQUIRE(im.shift >= 0 && im.shift <= 16 - im.bit_depth, "detector_candidates: image %d: shift %d outside 0..%d (16 - bit_depth)", i, im.shift, 16 - im.bit_depth);
    VGH_REQUIRE(im.y_offset >= 0 && im.y_offset < (1 << im.bit_depth), "detector_candidates: image %d: y_offset %d outside 0..%d", i, im.y_offset, (1 << im.bit_depth) - 1);
    VGH_REQUIRE(im.cy >= 0 && im.cy <= (1 << 17), "detector_candidates: image %d: coefficient cy = %d outside 0..2^17", i, im.cy);
    const int32_t coef[4] = {im.crv, im.cgu, im.cgv, im.cbu};
    static const char* const names[4] = {"crv", "cgu", "cgv", "cbu"};
    for (int k = 0; k < 4; ++k)
        VGH_REQUIRE(coef[k] >= -(1 << 18) && coef[k] <= (1 << 18), "detector_candidates: image %d: coefficient %s = %d outside +-2^18", i, names[k], coef[k]);
    return VGH_OK;
}

template <typename Desc, typename Src>
int lb_prepare(vgh_lb_batch** plb, int S, int max_batch, int arena_batch, int fmt, const Src* imgs, int B) {
    std::vector<vgh_lb::Geometry> geo(B);
    for (int i = 0; i < B; ++i) {  // everything is checked before anything is allocated, written or queued
        const Src& im = imgs[i];
        if (int rc = check_source(im, i)) return rc;
        geo[i] = vgh_lb::geometry(im.h, im.w, S);
        VGH_REQUIRE(geo[i].new_w >= 1 && geo[i].new_h >= 1, "detector_candidates: image %d (%d x %d) is too elongated for a %dx%d letterbox", i, im.h, im.w, S, S);
    }
    if (!*plb)
        if (int rc = lb_create(S, max_batch, arena_batch, plb)) return rc;
    vgh_lb_batch* lb = *plb;
    const int k = lb->slot ^ 1;
    if (lb->recorded[k]) VGH_HIP(hipEventSynchronize(lb->ev[k]));  // its last call's copies / letterbox / select have run
    uint8_t* h = lb->host[k];
    float* unpad = (float*)h;
    for (int i = 0; i < B; ++i) {
        unpad[3 * i] = (float)geo[i].pad_x;
        unpad[3 * i + 1] = (float)geo[i].pad_y;
        unpad[3 * i + 2] = (float)geo[i].scale;
    }
    size_t at = align16((size_t)lb->max_batch * 12);
    lb->chunk_at.clear();
    for (int c0 = 0; c0 < B; c0 += arena_batch) {
        const int n = B - c0 < arena_batch ? B - c0 : arena_batch;
        lb->chunk_at.push_back(at);
        Desc* desc = (Desc*)(h + at);
        at = align16(at + (size_t)n * sizeof(Desc));
        for (int i = 0; i < n; ++i) {
            const Src& im = imgs[c0 + i];
            const vgh_lb::Geometry& g = geo[c0 + i];
            Desc& a = desc[i];
            set_source(a, im);
            a.src_h = im.h;
            a.src_w = im.w;
            a.new_w = g.new_w;
            a.new_h = g.new_h;
            a.pad_x = g.pad_x;
            a.pad_y = g.pad_y;
            a.pad = 127u;  // letterbox.py PAD_VALUE = (127, 0, 0): cv2.copyMakeBorder(..., value=127) on an RGB image
            const int32_t** ofs[2] = {&a.xofs, &a.yofs};
            const int16_t** coef[2] = {&a.alpha, &a.beta};
            const int src_len[2] = {im.w, im.h}, dst_len[2] = {g.new_w, g.new_h};
            for (int ax = 0; ax < 2; ++ax) {
                const vgh_lb::AxisTables& t = cached_tables(lb, src_len[ax], dst_len[ax]);
                const size_t ob = (size_t)dst_len[ax] * 4, cb = (size_t)dst_len[ax] * 16;
                VGH_REQUIRE(align16(at + ob) + cb <= lb->slot_bytes, "detector_candidates: letterbox staging overflow (internal)");
                memcpy(h + at, t.ofs.data(), ob);
                *ofs[ax] = (const int32_t*)(lb->dev[k] + at);
                at = align16(at + ob);
                memcpy(h + at, t.coef.data(), cb);
                *coef[ax] = (const int16_t*)(lb->dev[k] + at);
                at = align16(at + cb);
            }
        }
    }
    lb->chunk_at.push_back(at);
    lb->slot = k;
    lb->fmt = fmt;
    return VGH_OK;
}

template <typename Desc>
void launch_batch(const vgh_lb_batch* lb, int k, int chunk, int n, hipStream_t stream) {
    const int S = lb->S;
    hipLaunchKernelGGL(letterbox_batch_kernel<Desc>, dim3((S + 31) / 32, (S + 7) / 8, n), dim3(256), 0, stream, (const Desc*)(lb->dev[k] + lb->chunk_at[chunk]), lb->canvas, S);
}

}  // namespace

int vgh_lb_prepare(vgh_lb_batch** plb, int S, int max_batch, int arena_batch, int image_fmt, const void* imgs, int B) {
    if (image_fmt == VGH_IMG_YUV420_RAW) return lb_prepare<LbYuvImage>(plb, S, max_batch, arena_batch, image_fmt, (const vgh_yuv420_image*)imgs, B);
    if (image_fmt == VGH_IMG_YUV420P16_RAW) return lb_prepare<LbYuv16Image>(plb, S, max_batch, arena_batch, image_fmt, (const vgh_yuv420p16_image*)imgs, B);
    VGH_REQUIRE(image_fmt == VGH_IMG_U8_RAW, "letterbox: image format %d is not a raw format", image_fmt);
    return lb_prepare<LbImage>(plb, S, max_batch, arena_batch, image_fmt, (const vgh_raw_image*)imgs, B);
}

int vgh_lb_chunk(vgh_lb_batch* lb, int chunk, int n, hipStream_t stream) {
    VGH_REQUIRE(lb && chunk >= 0 && chunk + 1 < (int)lb->chunk_at.size() && n >= 1 && n <= lb->arena_batch, "letterbox: chunk %d outside the prepared batch", chunk);
    const int k = lb->slot;
    const size_t from = chunk == 0 ? 0 : lb->chunk_at[chunk], to = lb->chunk_at[chunk + 1];  // chunk 0 carries the un-pad table in front
    VGH_HIP(hipMemcpyAsync(lb->dev[k] + from, lb->host[k] + from, to - from, hipMemcpyHostToDevice, stream));
    if (lb->fmt == VGH_IMG_YUV420_RAW)
        launch_batch<LbYuvImage>(lb, k, chunk, n, stream);
    else if (lb->fmt == VGH_IMG_YUV420P16_RAW)
        launch_batch<LbYuv16Image>(lb, k, chunk, n, stream);
    else
        launch_batch<LbImage>(lb, k, chunk, n, stream);
    VGH_HIP(hipGetLastError());
    VGH_HIP(hipEventRecord(lb->ev[k], stream));
    lb->recorded[k] = true;
    return VGH_OK;
}

int vgh_lb_unpad_read(vgh_lb_batch* lb, hipStream_t stream) {
    VGH_HIP(hipEventRecord(lb->ev[lb->slot], stream));
    lb->recorded[lb->slot] = true;
    return VGH_OK;
}

uint8_t* vgh_lb_canvas(const vgh_lb_batch* lb) { return lb ? lb->canvas : nullptr; }
float* vgh_lb_unpad(const vgh_lb_batch* lb) { return lb ? (float*)lb->dev[lb->slot] : nullptr; }

void vgh_lb_destroy(vgh_lb_batch* lb) {
    if (lb) lb_free(lb);
}
