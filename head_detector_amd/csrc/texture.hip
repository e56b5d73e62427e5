// libvghtex.so (include/vgh_tex.h): Sim3DR's `render_texture` (`_render_texture_core`, head_detector/Sim3DR/lib/rasterize_kernel.cpp:358-463), the
// z-buffered rasteriser that paints a mesh from a texture image through per-vertex texture coordinates, for all heads of an image at once and in both
// directions: onto the photograph (wrap) or, with the UV atlas as the image and the photograph as the texture, into one atlas per head (unwrap).
//
// Per pixel the result is a serial fold over heads (in order) and over the head's triangles (in index order); csrc/mesh_render.hip's tile-major scheme
// reproduces such a fold exactly and is restated here (this library shares no object and no header with the other three):
//   fill     the background of depth, triangle and head (-1e8 is no memset pattern); dst is left alone
//   boxes    one lane per (head, triangle): the triangle's clamped integer bounding box as 4 x int16
//   tiles    one 256-lane workgroup per 16 x 16 tile of a destination that some head touches (the host builds "tile -> heads in order" from the
//            per-head pixel bounds; with one destination per head every (head, tile) pair is a workgroup of its own).  A lane owns one pixel and
//            keeps depth, owner and the winner's clamped texture position in registers.  For every head of the tile the workgroup scans the head's
//            boxes 256 at a time, compacts the ones that overlap the tile IN INDEX ORDER into LDS (ballot + prefix) together with their
//            pixel-independent set-up (88 B a triangle, 22 KB a workgroup, so seven workgroups share a CU's 160 KB of LDS), and
//            every lane walks that list serially with exactly the reference's arithmetic.
// In the reference every win rewrites the pixel's colour and only the last one stays, and the colour depends on nothing but the winner's texture
// position: the lane looks the texture up once, after the fold.  No atomics anywhere.
// The INSIDE RULE is  x < 2 || x > w - 3 || y < 2 || y > h - 3 || is_point_in_tri:  in a frame two pixels wide every pixel of a triangle's box counts.
// All arithmetic is IEEE float32 in the reference's operation order (contraction off, true division): every output is bit-identical to the
// reference's own C++ (tests/test_gpu_texture.py).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/vgh_tex.h"

#pragma clang fp contract(off)

namespace {

// ---- error plumbing: never throw across the C ABI ---------------------------------------------------------------------------------------------
thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define TEX_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return VGHTEX_ERR_HIP;                                                          \
        }                                                                                   \
    } while (0)

#define TEX_REQUIRE(cond, ...)         \
    do {                               \
        if (!(cond)) {                 \
            set_error(__VA_ARGS__);    \
            return VGHTEX_ERR_INVALID; \
        }                              \
    } while (0)

constexpr int TILE = 16;             // 16 x 16 pixels = the 256 lanes of a workgroup
constexpr float BACKGROUND = -1e8f;  // what Sim3DR's callers initialise the depth buffer with (Sim3DR.py:31)

// ---- the background of depth, triangle and head ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_kernel(size_t n_px, float* __restrict__ depth, int32_t* __restrict__ tri, int32_t* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    depth[i] = BACKGROUND;
    if (tri) tri[i] = -1;
    if (head) head[i] = -1;
}

// ---- the triangle's integer box (rasterize_kernel.cpp:406-415) -----------------------------------------------------------------------------------
struct alignas(8) Box {
    int16_t x0, y0, x1, y1;  // inclusive; x1 < x0 = covers nothing
};

__global__ __launch_bounds__(256) void boxes_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tri, int n_total, int V, int T, int h, int w,
                                                    Box* __restrict__ boxes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int head = i / T, t = i - head * T;
    const float* p = verts + (size_t)head * V * 3;
    const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    const float p0x = p[3 * i0], p0y = p[3 * i0 + 1], p1x = p[3 * i1], p1y = p[3 * i1 + 1], p2x = p[3 * i2], p2y = p[3 * i2 + 1];
    const float fx0 = fminf(p0x, fminf(p1x, p2x)), fx1 = fmaxf(p0x, fmaxf(p1x, p2x));
    const float fy0 = fminf(p0y, fminf(p1y, p2y)), fy1 = fmaxf(p0y, fmaxf(p1y, p2y));
    Box b = {1, 1, 0, 0};
    // a triangle with a non-finite corner is skipped ((int)ceil(nan) is undefined in C; fminf / fmaxf would hide a NaN, so look at the corners)
    const bool finite = isfinite(p0x) && isfinite(p0y) && isfinite(p1x) && isfinite(p1y) && isfinite(p2x) && isfinite(p2y);
    if (finite) {
        // clamp in float first: (int)ceil(1e30f) is undefined in C; the clamped result is what any in-range input gives
        const int x_min = max((int)ceilf(fmaxf(fx0, -1.0f)), 0), x_max = min((int)floorf(fminf(fx1, (float)w)), w - 1);
        const int y_min = max((int)ceilf(fmaxf(fy0, -1.0f)), 0), y_max = min((int)floorf(fminf(fy1, (float)h)), h - 1);
        if (x_max >= x_min && y_max >= y_min) b = {(int16_t)x_min, (int16_t)y_min, (int16_t)x_max, (int16_t)y_max};  // w, h <= VGHTEX_MAX_SIDE
    }
    boxes[i] = b;
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------------------------------
// What a lane needs of a triangle that overlaps the tile: the pixel-independent part of get_point_weight (rasterize_kernel.cpp:54-82), the three depths,
// the three texture corners, the box and the triangle's index.  88 B x 256 = 22 KB of LDS a workgroup.
struct Hit {
    float p0x, p0y, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv;
    float d0, d1, d2;
    float q0x, q0y, q1x, q1y, q2x, q2y;
    int32_t t;
    Box box;
};

__device__ __forceinline__ void tri_setup(Hit& t, float p1x, float p1y, float p2x, float p2y) {
    t.v0x = p2x - t.p0x;
    t.v0y = p2y - t.p0y;
    t.v1x = p1x - t.p0x;
    t.v1y = p1y - t.p0y;
    t.dot00 = t.v0x * t.v0x + t.v0y * t.v0y;
    t.dot01 = t.v0x * t.v1x + t.v0y * t.v1y;
    t.dot11 = t.v1x * t.v1x + t.v1y * t.v1y;
    const float den = t.dot00 * t.dot11 - t.dot01 * t.dot01;
    t.inv = (den == 0.0f) ? 0.0f : 1.0f / den;
}
__device__ __forceinline__ void tri_uv(const Hit& t, float px, float py, float& u, float& v) {
    const float v2x = px - t.p0x, v2y = py - t.p0y;
    const float dot02 = t.v0x * v2x + t.v0y * v2y;
    const float dot12 = t.v1x * v2x + t.v1y * v2y;
    u = (t.dot11 * dot02 - t.dot01 * dot12) * t.inv;
    v = (t.dot00 * dot12 - t.dot01 * dot02) * t.inv;
}

// std::min / std::max as the source calls them: min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a (a NaN in `a` stays)
__device__ __forceinline__ float clamp_like_std(float a, float hi) {
    a = hi < a ? hi : a;
    return a < 0.0f ? 0.0f : a;
}
// an index into the texture whatever the float was (a NaN or an infinity converts to something; it is clamped like everything else)
__device__ __forceinline__ int texel_index(float f, int last) { return min(max((int)f, 0), last); }

__device__ __forceinline__ float texel(const void* __restrict__ tex, int is_u8, size_t at) {
    return is_u8 ? (float)((const uint8_t*)tex)[at] : ((const float*)tex)[at];  // u8 -> f32 is exact
}

struct TexArgs {
    const float* coords;  // [n or 1, Vt, 3]
    const void* texture;  // [n or 1, th, tw, tc]
    int Vt, th, tw, tc;
    int coords_per_head, tex_per_head, is_u8, bilinear;
};

// blockIdx.x = an entry of the tile list: tile_xy = tile column | tile row << 16, its heads are tile_heads[tile_first[b] .. tile_first[b + 1]).  With
// per_head destinations an entry has exactly one head and paints that head's slice.  Only pixels that end with an owner are written (fill_kernel wrote the
// background of depth, triangle and head; dst keeps what it holds); tri_out and head_out may be null.
__global__ __launch_bounds__(256) void tiles_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tri, const int32_t* __restrict__ tex_tri,
                                                    const Box* __restrict__ boxes, const uint32_t* __restrict__ tile_xy, const int32_t* __restrict__ tile_first,
                                                    const int32_t* __restrict__ tile_heads, TexArgs ta, int V, int T, int h, int w, int c, int shared_depth, int per_head,
                                                    float zsign, float* __restrict__ dst, float* __restrict__ depth_out, int32_t* __restrict__ tri_out,
                                                    int32_t* __restrict__ head_out) {
    __shared__ Hit hits[256];
    __shared__ int wave_hits[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t xy = tile_xy[blockIdx.x];
    const int tx0 = (int)(xy & 0xffffu) * TILE, ty0 = (int)(xy >> 16) * TILE;
    const int tx1 = min(tx0 + TILE - 1, w - 1), ty1 = min(ty0 + TILE - 1, h - 1);
    const int x = tx0 + (tid & (TILE - 1)), y = ty0 + (tid >> 4);
    const float px = (float)x, py = (float)y;
    const bool frame = x < 2 || x > w - 3 || y < 2 || y > h - 3;  // the source's border rule: here every pixel of a triangle's box is "inside"
    float depth = BACKGROUND;                                     // the depth the next triangle has to beat
    float o_depth = BACKGROUND, o_qx = 0.0f, o_qy = 0.0f;
    int o_head = -1, o_tri = -1;
    const float tex_x_last = (float)(ta.tw - 1), tex_y_last = (float)(ta.th - 1);
    const int e0 = tile_first[blockIdx.x], e1 = tile_first[blockIdx.x + 1];
    for (int e = e0; e < e1; ++e) {
        const int head = tile_heads[e];
        const float* p = verts + (size_t)head * V * 3;
        const float* q = ta.coords + (ta.coords_per_head ? (size_t)head * ta.Vt * 3 : 0);
        const Box* hb = boxes + (size_t)head * T;
        if (!shared_depth) depth = BACKGROUND;  // ORDER: every head's call starts from a fresh depth buffer; whatever it paints replaces the owner
        for (int base = 0; base < T; base += 256) {
            const int t = base + tid;
            Box b = {1, 1, 0, 0};
            if (t < T) b = hb[t];
            const bool hit = b.x1 >= b.x0 && b.x1 >= tx0 && b.x0 <= tx1 && b.y1 >= ty0 && b.y0 <= ty1;
            const unsigned long long mask = __ballot(hit);
            if (lane == 0) wave_hits[wave] = __popcll(mask);
            __syncthreads();
            int slot = __popcll(mask & ((1ull << lane) - 1ull)), count = 0;
            for (int k = 0; k < 4; ++k) {
                const int n = wave_hits[k];
                if (k < wave) slot += n;
                count += n;
            }
            if (hit) {  // index order: waves in order, lanes in order
                const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
                Hit k;
                k.p0x = p[3 * i0];
                k.p0y = p[3 * i0 + 1];
                tri_setup(k, p[3 * i1], p[3 * i1 + 1], p[3 * i2], p[3 * i2 + 1]);
                k.d0 = zsign * p[3 * i0 + 2];
                k.d1 = zsign * p[3 * i1 + 2];
                k.d2 = zsign * p[3 * i2 + 2];
                // texture x through the texture's triangle list, texture y through the mesh's: the source's indexing (rasterize_kernel.cpp:398-403)
                k.q0x = q[3 * tex_tri[3 * t]];
                k.q0y = q[3 * i0 + 1];
                k.q1x = q[3 * tex_tri[3 * t + 1]];
                k.q1y = q[3 * i1 + 1];
                k.q2x = q[3 * tex_tri[3 * t + 2]];
                k.q2y = q[3 * i2 + 1];
                k.t = t;
                k.box = b;
                hits[slot] = k;
            }
            __syncthreads();
            for (int s = 0; s < count; ++s) {
                const Hit& k = hits[s];  // every lane reads the same entry: a broadcast
                if (x < k.box.x0 || x > k.box.x1 || y < k.box.y0 || y > k.box.y1) continue;  // the reference visits the pixels of the triangle's box only
                float u, v;
                tri_uv(k, px, py, u, v);
                if (frame || (u >= 0 && v >= 0 && u + v < 1)) {  // is_point_in_tri is false for NaN
                    const float w0 = 1.0f - u - v;
                    const float pd = w0 * k.d0 + v * k.d1 + u * k.d2;
                    if (pd > depth) {  // false for NaN; -0 and +0 compare equal, as in the reference
                        depth = pd;
                        o_depth = pd;
                        o_head = head;
                        o_tri = k.t;
                        o_qx = clamp_like_std(k.q0x * w0 + k.q1x * v + k.q2x * u, tex_x_last);
                        o_qy = clamp_like_std(k.q0y * w0 + k.q1y * v + k.q2y * u, tex_y_last);
                    }
                }
            }
            // the next chunk's wave_hits are written before, its hits after, a barrier every wave reaches only when it is done with this list
        }
    }
    if (o_head < 0) return;  // no barrier follows
    // inside some triangle's clamped box, hence inside the image; per_head: the entry's only head owns the slice
    const size_t at = (per_head ? (size_t)o_head * (size_t)h * (size_t)w : 0) + (size_t)y * (size_t)w + (size_t)x;
    depth_out[at] = o_depth;
    if (tri_out) tri_out[at] = o_tri;
    if (head_out) head_out[at] = o_head;
    const uint8_t* base = (const uint8_t*)ta.texture;
    const size_t texels = (size_t)ta.th * ta.tw * ta.tc;
    const void* tex = ta.tex_per_head ? (const void*)(base + (size_t)o_head * texels * (ta.is_u8 ? 1 : 4)) : ta.texture;
    float* out = dst + at * (size_t)c;
    const int xl = ta.tw - 1, yl = ta.th - 1;
    if (!ta.bilinear) {
        const size_t a = ((size_t)texel_index(roundf(o_qy), yl) * ta.tw + texel_index(roundf(o_qx), xl)) * ta.tc;  // roundf: halves away from zero
        for (int k = 0; k < c; ++k) out[k] = texel(tex, ta.is_u8, a + k);
    } else {
        const float fx = floorf(o_qx), fy = floorf(o_qy);
        const float xd = o_qx - fx, yd = o_qy - fy;
        const int xf = texel_index(fx, xl), xc = texel_index(ceilf(o_qx), xl), yf = texel_index(fy, yl), yc = texel_index(ceilf(o_qy), yl);
        const size_t a_ul = ((size_t)yf * ta.tw + xf) * ta.tc, a_ur = ((size_t)yf * ta.tw + xc) * ta.tc;
        const size_t a_dl = ((size_t)yc * ta.tw + xf) * ta.tc, a_dr = ((size_t)yc * ta.tw + xc) * ta.tc;
        for (int k = 0; k < c; ++k) {
            const float ul = texel(tex, ta.is_u8, a_ul + k), ur = texel(tex, ta.is_u8, a_ur + k), dl = texel(tex, ta.is_u8, a_dl + k), dr = texel(tex, ta.is_u8, a_dr + k);
            out[k] = ul * (1 - xd) * (1 - yd) + ur * xd * (1 - yd) + dl * (1 - xd) * yd + dr * xd * yd;
        }
    }
}

// ---- per-device state: what one call uploads (one pinned and one device block, guarded by an event) and the boxes -----------------------------------
struct State {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;
    Box* boxes = nullptr;  // library scratch [n, T], grown on demand
    size_t box_bytes = 0;
};

std::mutex g_mutex;
std::map<int, State> g_state;

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// waits for the blocks' previous user (whatever stream it was queued on), then makes room for `need` staging bytes and `need_boxes` bytes of boxes
int reserve(State& s, size_t need, size_t need_boxes) {
    if (s.recorded) TEX_HIP(hipEventSynchronize(s.ev));
    s.recorded = false;
    if (!s.ev) TEX_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (need > s.bytes) {
        hipHostFree(s.host);
        hipFree(s.dev);
        s.host = s.dev = nullptr;
        s.bytes = 0;
        const size_t cap = align16(need + need / 2);
        if (hipHostMalloc((void**)&s.host, cap, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s.dev, cap) != hipSuccess) {
            hipHostFree(s.host);
            s.host = nullptr;
            set_error("render_texture: allocating %zu bytes of staging failed", cap);
            return VGHTEX_ERR_NOMEM;
        }
        s.bytes = cap;
    }
    if (need_boxes > s.box_bytes) {
        hipFree(s.boxes);
        s.boxes = nullptr;
        s.box_bytes = 0;
        if (hipMalloc((void**)&s.boxes, need_boxes) != hipSuccess) {
            set_error("render_texture: allocating %zu bytes of triangle boxes failed", need_boxes);
            return VGHTEX_ERR_NOMEM;
        }
        s.box_bytes = need_boxes;
    }
    return VGHTEX_OK;
}

inline bool is_flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace

extern "C" VGHTEX_API const char* vghtex_version(void) { return "vghtex 1 (gfx950)"; }

extern "C" VGHTEX_API const char* vghtex_last_error(void) { return g_error; }

extern "C" VGHTEX_API int vghtex_render_texture(const vghtex_job* job, void* stream) {
    TEX_REQUIRE(job, "render_texture: null job");
    const vghtex_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    TEX_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHTEX_MAX_SIDE && j.width <= VGHTEX_MAX_SIDE, "render_texture: height x width %d x %d outside 1 .. %d", j.height,
                j.width, VGHTEX_MAX_SIDE);
    const int W = j.width, H = j.height, n = j.n_heads, V = j.n_vertices, T = j.n_triangles, Vt = j.n_tex_vertices, c = j.channels;
    TEX_REQUIRE(c >= 1 && c <= VGHTEX_MAX_CHANNELS, "render_texture: channels %d outside 1 .. %d", c, VGHTEX_MAX_CHANNELS);
    TEX_REQUIRE(n >= 0 && n <= VGHTEX_MAX_HEADS, "render_texture: n_heads %d outside 0 .. %d", n, VGHTEX_MAX_HEADS);
    TEX_REQUIRE(V >= 0, "render_texture: n_vertices %d is negative", V);
    TEX_REQUIRE(T >= 0, "render_texture: n_triangles %d is negative", T);
    TEX_REQUIRE(Vt >= 0, "render_texture: n_tex_vertices %d is negative", Vt);
    TEX_REQUIRE(j.tex_height >= 1 && j.tex_width >= 1 && j.tex_height <= VGHTEX_MAX_SIDE && j.tex_width <= VGHTEX_MAX_SIDE,
                "render_texture: tex_height x tex_width %d x %d outside 1 .. %d", j.tex_height, j.tex_width, VGHTEX_MAX_SIDE);
    TEX_REQUIRE(j.tex_channels >= c, "render_texture: tex_channels %d below channels %d", j.tex_channels, c);
    TEX_REQUIRE(j.tex_dtype == VGHTEX_TEX_F32 || j.tex_dtype == VGHTEX_TEX_U8, "render_texture: tex_dtype %d is neither 0 (f32) nor 1 (u8)", j.tex_dtype);
    TEX_REQUIRE(is_flag(j.tex_per_head), "render_texture: tex_per_head %d is neither 0 nor 1", j.tex_per_head);
    TEX_REQUIRE(is_flag(j.tex_coords_per_head), "render_texture: tex_coords_per_head %d is neither 0 nor 1", j.tex_coords_per_head);
    TEX_REQUIRE(is_flag(j.dst_per_head), "render_texture: dst_per_head %d is neither 0 nor 1", j.dst_per_head);
    TEX_REQUIRE(j.mapping == VGHTEX_MAP_NEAREST || j.mapping == VGHTEX_MAP_BILINEAR, "render_texture: mapping %d is neither 0 (nearest) nor 1 (bilinear)", j.mapping);
    TEX_REQUIRE(j.mode == VGHTEX_MODE_ORDER || j.mode == VGHTEX_MODE_DEPTH, "render_texture: mode %d is neither 0 (order) nor 1 (depth)", j.mode);
    TEX_REQUIRE(j.z_sign == 1.0f || j.z_sign == -1.0f, "render_texture: z_sign %g is neither +1 nor -1", (double)j.z_sign);
    const size_t slices = j.dst_per_head ? (size_t)n : 1;
    const size_t n_px = slices * (size_t)H * (size_t)W;
    TEX_REQUIRE(n_px / 256 < (size_t)INT32_MAX, "render_texture: %zu destination pixels exceed one launch", n_px);
    if (n_px) {
        TEX_REQUIRE(j.dst_dev, "render_texture: null dst_dev");
        TEX_REQUIRE(j.depth_dev, "render_texture: null depth_dev");
    }
    const bool raster = n > 0 && T > 0;
    if (raster) {
        TEX_REQUIRE(V >= 1, "render_texture: n_vertices %d with %d triangles", V, T);
        TEX_REQUIRE(Vt >= 1, "render_texture: n_tex_vertices %d with %d triangles", Vt, T);
        TEX_REQUIRE(j.verts_dev, "render_texture: null verts_dev");
        TEX_REQUIRE(j.triangles, "render_texture: null triangles");
        TEX_REQUIRE(j.tex_coords_dev, "render_texture: null tex_coords_dev");
        TEX_REQUIRE(j.tex_triangles, "render_texture: null tex_triangles");
        TEX_REQUIRE(j.texture_dev, "render_texture: null texture_dev");
        TEX_REQUIRE(j.bounds, "render_texture: null bounds");
        TEX_REQUIRE((int64_t)n * T <= INT32_MAX / 4 && (int64_t)n * V <= INT32_MAX / 4 && (int64_t)n * Vt <= INT32_MAX / 4,
                    "render_texture: n_heads * n_triangles = %lld, n_heads * n_vertices = %lld or n_heads * n_tex_vertices = %lld exceed one launch", (long long)n * T,
                    (long long)n * V, (long long)n * Vt);
        const int both = V < Vt ? V : Vt;  // a mesh index reads a vertex and, for the corner's texture y, a texture coordinate
        for (int64_t i = 0; i < (int64_t)T * 3; ++i) {
            TEX_REQUIRE(j.triangles[i] >= 0 && j.triangles[i] < V, "render_texture: triangles: triangle %lld: index %d outside the %d vertices", (long long)(i / 3), j.triangles[i], V);
            TEX_REQUIRE(j.triangles[i] < both, "render_texture: triangles: triangle %lld: index %d outside the %d texture coordinates (a corner's texture y is read through it)",
                        (long long)(i / 3), j.triangles[i], Vt);
            TEX_REQUIRE(j.tex_triangles[i] >= 0 && j.tex_triangles[i] < Vt, "render_texture: tex_triangles: triangle %lld: index %d outside the %d texture coordinates",
                        (long long)(i / 3), j.tex_triangles[i], Vt);
        }
        for (int i = 0; i < n; ++i) {
            const int32_t* b = j.bounds + 4 * i;
            const bool empty = b[2] < b[0] || b[3] < b[1];
            TEX_REQUIRE(empty || (b[0] >= 0 && b[1] >= 0 && b[2] < W && b[3] < H), "render_texture: bounds: head %d: (%d, %d, %d, %d) outside the image", i, b[0], b[1], b[2], b[3]);
        }
    }
    // "tile -> heads in order" for the tiles some head touches: count, prefix, fill (heads are visited in order, so every list is ascending).  With one
    // destination per head every (head, tile) pair is an entry of its own with that one head.
    const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
    std::vector<int32_t> grid;
    size_t n_tiles = 0, n_pairs = 0;
    if (raster) {
        grid.assign((size_t)tiles_x * tiles_y + 1, 0);
        for (int i = 0; i < n; ++i) {
            const int32_t* b = j.bounds + 4 * i;
            if (b[2] < b[0] || b[3] < b[1]) continue;
            for (int ty = b[1] / TILE; ty <= b[3] / TILE; ++ty)
                for (int tx = b[0] / TILE; tx <= b[2] / TILE; ++tx) grid[(size_t)ty * tiles_x + tx]++;
        }
        for (size_t t = 0; t < (size_t)tiles_x * tiles_y; ++t) {
            n_tiles += grid[t] != 0;
            n_pairs += (size_t)grid[t];
        }
        if (j.dst_per_head) n_tiles = n_pairs;
    }
    TEX_REQUIRE(n_pairs <= (size_t)INT32_MAX, "render_texture: %zu (tile, head) pairs exceed one launch", n_pairs);
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    TEX_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    // one upload: [triangles | tex_triangles | tile_xy | tile_first | tile_heads], each from a 16-byte boundary
    const size_t at_tt = align16((size_t)T * 12), at_xy = at_tt + align16((size_t)T * 12), at_first = at_xy + align16(n_tiles * 4), at_heads = at_first + align16((n_tiles + 1) * 4);
    const size_t total = at_heads + align16(n_pairs * 4);
    if (n_tiles) {
        if (int rc = reserve(s, total, (size_t)n * T * sizeof(Box))) return rc;  // also waits for this device's previous call
        uint8_t* h = s.host;
        memcpy(h, j.triangles, (size_t)T * 12);
        memcpy(h + at_tt, j.tex_triangles, (size_t)T * 12);
        uint32_t* xy = (uint32_t*)(h + at_xy);
        int32_t* first = (int32_t*)(h + at_first);
        int32_t* heads = (int32_t*)(h + at_heads);
        if (j.dst_per_head) {
            size_t k = 0;
            for (int i = 0; i < n; ++i) {
                const int32_t* b = j.bounds + 4 * i;
                if (b[2] < b[0] || b[3] < b[1]) continue;
                for (int ty = b[1] / TILE; ty <= b[3] / TILE; ++ty)
                    for (int tx = b[0] / TILE; tx <= b[2] / TILE; ++tx) {
                        xy[k] = (uint32_t)tx | (uint32_t)ty << 16;
                        first[k] = (int32_t)k;
                        heads[k++] = i;
                    }
            }
            first[k] = (int32_t)k;
        } else {
            size_t k = 0, at = 0;
            for (size_t t = 0; t < (size_t)tiles_x * tiles_y; ++t) {  // grid[t] becomes the position of the tile's next head
                const int32_t cnt = grid[t];
                if (cnt) {
                    xy[k] = (uint32_t)(t % tiles_x) | (uint32_t)(t / tiles_x) << 16;
                    first[k++] = (int32_t)at;
                }
                grid[t] = (int32_t)at;
                at += (size_t)cnt;
            }
            first[k] = (int32_t)at;
            for (int i = 0; i < n; ++i) {
                const int32_t* b = j.bounds + 4 * i;
                if (b[2] < b[0] || b[3] < b[1]) continue;
                for (int ty = b[1] / TILE; ty <= b[3] / TILE; ++ty)
                    for (int tx = b[0] / TILE; tx <= b[2] / TILE; ++tx) heads[grid[(size_t)ty * tiles_x + tx]++] = i;
            }
        }
    }
    // from here on work is queued: the first failure is kept, nothing more is queued after it, and the event is recorded on every path so that the next
    // call never rewrites the staging block or the boxes under work that is still queued
    hipError_t err = hipSuccess;
    const char* failed = "";
#define TEX_QUEUE(expr)                            \
    do {                                           \
        if (err == hipSuccess) {                   \
            err = (expr);                          \
            if (err != hipSuccess) failed = #expr; \
        }                                          \
    } while (0)
    if (n_tiles) TEX_QUEUE(hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event below covers the staging block
    if (n_px && err == hipSuccess) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, n_px, j.depth_dev, j.triangle_dev, j.head_dev);
    if (n_tiles && err == hipSuccess) {
        const uint8_t* d = s.dev;
        TexArgs ta;
        ta.coords = j.tex_coords_dev;
        ta.texture = j.texture_dev;
        ta.Vt = Vt;
        ta.th = j.tex_height;
        ta.tw = j.tex_width;
        ta.tc = j.tex_channels;
        ta.coords_per_head = j.tex_coords_per_head;
        ta.tex_per_head = j.tex_per_head;
        ta.is_u8 = j.tex_dtype == VGHTEX_TEX_U8;
        ta.bilinear = j.mapping != VGHTEX_MAP_NEAREST;
        hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)(n * T + 255) / 256), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, n * T, V, T, H, W, s.boxes);
        hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, (const int32_t*)(d + at_tt), (const Box*)s.boxes,
                           (const uint32_t*)(d + at_xy), (const int32_t*)(d + at_first), (const int32_t*)(d + at_heads), ta, V, T, H, W, c, j.mode == VGHTEX_MODE_DEPTH ? 1 : 0,
                           j.dst_per_head, j.z_sign, j.dst_dev, j.depth_dev, j.triangle_dev, j.head_dev);
    }
    TEX_QUEUE(hipGetLastError());
    if (n_tiles) {
        if (hipEventRecord(s.ev, st) == hipSuccess) {
            s.recorded = true;
        } else {
            hipStreamSynchronize(st);  // no event to wait for next time: wait now
            TEX_QUEUE(hipErrorUnknown);
        }
    }
#undef TEX_QUEUE
    if (err != hipSuccess) {
        set_error("render_texture: %s -> %s", failed, hipGetErrorString(err));
        return VGHTEX_ERR_HIP;
    }
    return VGHTEX_OK;
}
