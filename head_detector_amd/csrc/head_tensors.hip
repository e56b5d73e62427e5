// libvghcrop.so (include/vgh_crop.h): head tensors = every head of a call as one dense, normalised S x S crop in the next network's dtype, cut out of u8 RGB
// images or of 8-bit YUV 4:2:0 frames where they lie.  ONE staging upload (sources, heads, tile list) and ONE launch per call, whatever the number of heads or
// sources.  The rule is stated in the public header; its integer functions, the limits, the validation and the tile count are csrc/head_crop_rules.h's and exist
// nowhere else.  Integer arithmetic up to the int32 sum of a pixel's K^2 sub-samples, then two float32 operations in a stated order (-ffp-contract=off): equal bit
// for bit to tests/head_tensors_ref.py.
// Self-contained on purpose: no csrc/vgh_internal.h, no object of libvgh.so or of another companion, no other public header (csrc/companion_host.h is the host
// plumbing the companion libraries' sources share); built with -fvisibility=hidden, only the vghc_* functions are exported.
#include <hip/hip_fp16.h>
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_crop.h"
#include "companion_host.h"
#include "head_crop_rules.h"

namespace {

using namespace companion;
using namespace head_crop;
static_assert(VGHC_OK == OK && VGHC_ERR_INVALID == ERR_INVALID && VGHC_ERR_HIP == ERR_HIP && VGHC_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

// one 16 x 16 tile of one head's crop: what blockIdx.x maps to
struct Tile {
    int32_t head;
    uint32_t xy;  // tile column | tile row << 16
};

// what every block of a call shares: kernel arguments
struct Call {
    int32_t size, dtype, layout, order;
    int32_t fill[3];  // SOURCE channel order
    float b[3];       // output channel order
};

// global-address-space views: pointers read from a descriptor in memory would otherwise be accessed with flat instructions
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gmem(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}

// src(x, y, .) of the rule, in source channel order; a tap outside the source reads the fill
__device__ __forceinline__ void tap(const vghc_source& s, int x, int y, const int32_t (&fill)[3], int32_t (&t)[3]) {
    if ((unsigned)x >= (unsigned)s.w || (unsigned)y >= (unsigned)s.h) {
        t[0] = fill[0], t[1] = fill[1], t[2] = fill[2];
    } else if (s.kind == VGHC_SOURCE_RGB) {  // wave-uniform: a block works on one head, a head has one source
        const auto p = gmem(s.rgb_dev) + (size_t)y * s.rgb_pitch_bytes + 3 * x;
        t[0] = p[0], t[1] = p[1], t[2] = p[2];
    } else {
        const size_t at = (size_t)(y >> 1) * s.uv_pitch_bytes + (size_t)(x >> 1) * s.chroma_step;
        const int32_t Y = gmem(s.y_dev)[(size_t)y * s.y_pitch_bytes + x], U = gmem(s.u_dev)[at], V = gmem(s.v_dev)[at];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = yuv_channel(s, Y, U, V, c);
    }
}

__device__ __forceinline__ uint16_t bf16_bits(float y) {  // round to nearest even; y is never a NaN (finite a and b, a bounded sum)
    uint32_t u = __float_as_uint(y);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// One output pixel per lane, its K^2 sub-samples summed in registers: like warp_crops_kernel (csrc/aligned.hip) this class of kernel is bound by its byte
// gathers.  The tile, its head and the head's source are wave-uniform (scalar loads).  Planar stores are coalesced along j.
__global__ __launch_bounds__(256) void head_tensors_kernel(const vghc_source* __restrict__ sources, const vghc_head* __restrict__ heads, const Tile* __restrict__ tiles,
                                                           const Call call, void* __restrict__ dst) {
    const Tile t = tiles[blockIdx.x];
    const vghc_head& h = heads[t.head];
    const vghc_source& s = sources[h.source];
    const int S = call.size, K = h.supersample;
    const int j = (int)(t.xy & 0xffff) * kTile + (int)(threadIdx.x & (kTile - 1)), i = (int)(t.xy >> 16) * kTile + (int)(threadIdx.x >> 4);
    if (i >= S || j >= S) return;
    int32_t sum[3] = {0, 0, 0};
    int64_t row_x = sub_position(h.x0, h.xp, h.xq, j * K, i * K), row_y = sub_position(h.y0, h.yp, h.yq, j * K, i * K);
    for (int b = 0; b < K; ++b) {  // adding xp / xq step by step is exact in int64: the same positions as sub_position(p, q)
        int64_t px = row_x, py = row_y;
        for (int a = 0; a < K; ++a) {
            const int sx = source_pixel(px), sy = source_pixel(py), fx = fraction(px), fy = fraction(py);
            int32_t t00[3], t01[3], t10[3], t11[3];
            tap(s, sx, sy, call.fill, t00);
            tap(s, sx + 1, sy, call.fill, t01);
            tap(s, sx, sy + 1, call.fill, t10);
            tap(s, sx + 1, sy + 1, call.fill, t11);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += tap4(fx, fy, t00[c], t01[c], t10[c], t11[c]);
            px += h.xp, py += h.yp;
        }
        row_x += h.xq, row_y += h.yq;
    }
    const size_t plane = (size_t)S * S, at = (size_t)i * S + j, base = (size_t)t.head * 3 * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t v = sum[call.order == VGHC_ORDER_BGR ? 2 - c : c];
        const size_t o = call.layout == VGHC_LAYOUT_NCHW ? base + c * plane + at : base + at * 3 + c;
        if (call.dtype == VGHC_DTYPE_U8) {
            ((uint8_t*)dst)[o] = (uint8_t)round_u8(v, K);
            continue;
        }
        float y = (float)v * h.a[c];  // two float32 operations: the library is built with -ffp-contract=off
        y = y + call.b[c];
        if (call.dtype == VGHC_DTYPE_F32)
            ((float*)dst)[o] = y;
        else if (call.dtype == VGHC_DTYPE_F16)
            ((uint16_t*)dst)[o] = __half_as_ushort(__float2half_rn(y));
        else
            ((uint16_t*)dst)[o] = bf16_bits(y);
    }
}

// ---- staging: sources + heads + tile list of one call (companion_host.h) -----------------------------------------------------------------------------------
std::mutex g_mutex;
std::map<int, Staging> g_staging;

}  // namespace

extern "C" VGHC_API const char* vghc_version(void) { return "vghcrop 1 (gfx950)"; }

extern "C" VGHC_API const char* vghc_last_error(void) { return last_error(); }

extern "C" VGHC_API int vghc_head_tensors(const vghc_job* job, void* stream) {
    char why[400];
    const char* refusal = validate(job, why, sizeof(why));  // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(!refusal, "%s", why);
    const int n = job->n_heads, S = job->size;
    if (n == 0) return OK;
    const int64_t n_tiles = tile_count(n, S);

    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& st = g_staging[device];
    const size_t at_heads = align16((size_t)job->n_sources * sizeof(vghc_source)), at_tiles = align16(at_heads + (size_t)n * sizeof(vghc_head));
    const size_t total = at_tiles + (size_t)n_tiles * sizeof(Tile);
    if (int rc = reserve(st, total, "head_tensors")) return rc;
    memcpy(st.host, job->sources, (size_t)job->n_sources * sizeof(vghc_source));
    memcpy(st.host + at_heads, job->heads, (size_t)n * sizeof(vghc_head));
    Tile* ht = (Tile*)(st.host + at_tiles);
    const int side = tiles_per_side(S);
    for (int k = 0; k < n; ++k)
        for (int ty = 0; ty < side; ++ty)
            for (int tx = 0; tx < side; ++tx) *ht++ = Tile{k, (uint32_t)tx | (uint32_t)ty << 16};
    Call call;
    call.size = S, call.dtype = job->dtype, call.layout = job->layout, call.order = job->channel_order;
    for (int c = 0; c < 3; ++c) {
        const int out_c = job->channel_order == VGHC_ORDER_BGR ? 2 - c : c;  // the fill is given in the output's channel order
        call.fill[c] = (job->fill >> (8 * out_c)) & 255;
        call.b[c] = job->b[c];
    }
    hipStream_t s = (hipStream_t)stream;
    Queue q;  // from here on work is queued (companion_host.h, queue-then-record)
    CH_QUEUE(q, hipMemcpyAsync(st.dev, st.host, total, hipMemcpyHostToDevice, s));
    if (q.ok())
        hipLaunchKernelGGL(head_tensors_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, (const vghc_source*)st.dev, (const vghc_head*)(st.dev + at_heads),
                           (const Tile*)(st.dev + at_tiles), call, job->dst_dev);
    return finish(q, st, true, s, "head_tensors");
}
