// libvghvis.so (include/vgh_vis.h): the third function of Sim3DR's binding, `rasterize_triangles` (`_rasterize_triangles`,
// head_detector/Sim3DR/lib/rasterize_kernel.cpp:295-353), for all heads of an image at once: per pixel the head, the triangle, the depth and the
// barycentric weights that show, and per head how many pixels it covers alone, how many of them remain its own, and which of its vertices can be seen.
//
// Per pixel the result is a serial fold over heads (in order) and over the head's triangles (in index order); csrc/mesh_render.hip's tile-major
// scheme reproduces such a fold exactly and is restated here (this library shares no object and no header with libvghview.so):
//   fill     the background of every output (-1e8 is no memset pattern)
//   boxes    one lane per (head, triangle): the triangle's clamped integer bounding box as 4 x int16
//   tiles    one 256-lane workgroup per 16 x 16 image tile that some head touches (the host builds "tile -> heads in order" from the per-head
//            pixel bounds); a lane owns one pixel and keeps depth, owner and weights in registers.  For every head of the tile the workgroup scans
//            the head's boxes 256 at a time, compacts the ones that overlap the tile IN INDEX ORDER into LDS (ballot + prefix) together with their
//            pixel-independent set-up, and every lane walks that list serially with exactly the reference's arithmetic.
// The INSIDE RULE is is_point_in_tri's  u >= 0 && v >= 0 && u + v < 1,  not the  w0 > 0 && w1 > 0 && w2 > 0  of `_rasterize`: an edge or corner on a
// pixel centre belongs to the triangle, and a zero-determinant triangle (inverDeno = 0, so u = v = 0) holds every pixel of its box with weights
// (1, 0, 0).  is_point_in_tri and get_point_weight compute u and v by the same operations, so one evaluation serves the test and the weights.
// No 64-bit keys, no atomics on depth; the pixel counts are integer atomics (order-independent), the vertex flags same-value byte stores.
// All arithmetic is IEEE float32 in the reference's operation order (contraction off, true division): every output is bit-identical to the
// reference's own C++ (tests/test_gpu_visibility.py).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/vgh_vis.h"

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

#define VIS_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return VGHVIS_ERR_HIP;                                                          \
        }                                                                                   \
    } while (0)

#define VIS_REQUIRE(cond, ...)         \
    do {                               \
        if (!(cond)) {                 \
            set_error(__VA_ARGS__);    \
            return VGHVIS_ERR_INVALID; \
        }                              \
    } while (0)

constexpr int TILE = 16;           // 16 x 16 pixels = the 256 lanes of a workgroup
constexpr float BACKGROUND = -1e8f;  // what Sim3DR.rasterize initialises the depth buffer with (Sim3DR.py:31)

// ---- the background of every output ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_kernel(size_t n_px, float* __restrict__ depth, int32_t* __restrict__ tri, int32_t* __restrict__ head, float* __restrict__ bary) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    depth[i] = BACKGROUND;
    tri[i] = -1;
    head[i] = -1;
    if (bary) {  // 3 n_px floats, written as three coalesced planes of the flat array
        bary[i] = 0.0f;
        bary[n_px + i] = 0.0f;
        bary[2 * n_px + i] = 0.0f;
    }
}

// ---- the triangle's integer box (rasterize_kernel.cpp:321-329) -----------------------------------------------------------------------------------
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
        if (x_max >= x_min && y_max >= y_min) b = {(int16_t)x_min, (int16_t)y_min, (int16_t)x_max, (int16_t)y_max};  // w, h <= VGHVIS_MAX_SIDE
    }
    boxes[i] = b;
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------------------------------
// What a lane needs of a triangle that overlaps the tile: the pixel-independent part of is_point_in_tri / get_point_weight (rasterize_kernel.cpp:26-82),
// the three depths, the box and the triangle's index.  64 B x 256 = 16 KB of LDS a workgroup.
struct Hit {
    float p0x, p0y, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv;
    float d0, d1, d2;
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

// blockIdx.x = an entry of the tile list: tile_xy = tile column | tile row << 16, its heads are tile_heads[tile_first[b] .. tile_first[b + 1]).
// Only pixels that end with an owner are written (fill_kernel wrote the background); bary, visible, covered, vertex_visible may be null.
__global__ __launch_bounds__(256) void tiles_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tri, const Box* __restrict__ boxes,
                                                    const uint32_t* __restrict__ tile_xy, const int32_t* __restrict__ tile_first, const int32_t* __restrict__ tile_heads, int V,
                                                    int T, int h, int w, int shared_depth, float zsign, float* __restrict__ depth_out, int32_t* __restrict__ tri_out,
                                                    int32_t* __restrict__ head_out, float* __restrict__ bary_out, int32_t* __restrict__ visible, int32_t* __restrict__ covered,
                                                    uint8_t* __restrict__ vertex_visible) {
    __shared__ Hit hits[256];
    __shared__ int wave_hits[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t xy = tile_xy[blockIdx.x];
    const int tx0 = (int)(xy & 0xffffu) * TILE, ty0 = (int)(xy >> 16) * TILE;
    const int tx1 = min(tx0 + TILE - 1, w - 1), ty1 = min(ty0 + TILE - 1, h - 1);
    const int x = tx0 + (tid & (TILE - 1)), y = ty0 + (tid >> 4);
    const float px = (float)x, py = (float)y;
    float depth = BACKGROUND;  // the depth the next triangle has to beat
    float o_depth = BACKGROUND, o_w0 = 0.0f, o_w1 = 0.0f, o_w2 = 0.0f;
    int o_head = -1, o_tri = -1;
    const int e0 = tile_first[blockIdx.x], e1 = tile_first[blockIdx.x + 1];
    for (int e = e0; e < e1; ++e) {
        const int head = tile_heads[e];
        const float* p = verts + (size_t)head * V * 3;
        const Box* hb = boxes + (size_t)head * T;
        if (!shared_depth) depth = BACKGROUND;  // ORDER: every head's solo pass starts from fresh buffers; whatever it covers replaces the owner
        bool solo = false;                      // the head's solo pass covers this pixel: some inside triangle beats the fresh depth
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
                const int c = wave_hits[k];
                if (k < wave) slot += c;
                count += c;
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
                if (u >= 0 && v >= 0 && u + v < 1) {  // is_point_in_tri; false for NaN
                    const float w0 = 1.0f - u - v;
                    const float pd = w0 * k.d0 + v * k.d1 + u * k.d2;
                    solo = solo || pd > BACKGROUND;
                    if (pd > depth) {  // false for NaN; -0 and +0 compare equal, as in the reference
                        depth = pd;
                        o_depth = pd;
                        o_head = head;
                        o_tri = k.t;
                        o_w0 = w0;
                        o_w1 = v;
                        o_w2 = u;
                    }
                }
            }
            // the next chunk's wave_hits are written before, its hits after, a barrier every wave reaches only when it is done with this list
        }
        if (covered) {
            const int c = __popcll(__ballot(solo));
            if (lane == 0 && c) atomicAdd(covered + head, c);
        }
    }
    if (visible) {
        for (int e = e0; e < e1; ++e) {
            const int head = tile_heads[e];
            const int c = __popcll(__ballot(o_head == head));
            if (lane == 0 && c) atomicAdd(visible + head, c);
        }
    }
    if (o_head >= 0) {  // inside some triangle's clamped box, hence inside the image
        const size_t at = (size_t)y * (size_t)w + (size_t)x;
        depth_out[at] = o_depth;
        tri_out[at] = o_tri;
        head_out[at] = o_head;
        if (bary_out) {
            bary_out[3 * at] = o_w0;
            bary_out[3 * at + 1] = o_w1;
            bary_out[3 * at + 2] = o_w2;
        }
        if (vertex_visible) {  // the same 1 from every pixel of the triangle
            uint8_t* vv = vertex_visible + (size_t)o_head * V;
            vv[tri[3 * o_tri]] = 1;
            vv[tri[3 * o_tri + 1]] = 1;
            vv[tri[3 * o_tri + 2]] = 1;
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
    if (s.recorded) VIS_HIP(hipEventSynchronize(s.ev));
    s.recorded = false;
    if (!s.ev) VIS_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (need > s.bytes) {
        hipHostFree(s.host);
        hipFree(s.dev);
        s.host = s.dev = nullptr;
        s.bytes = 0;
        const size_t cap = align16(need + need / 2);
        if (hipHostMalloc((void**)&s.host, cap, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s.dev, cap) != hipSuccess) {
            hipHostFree(s.host);
            s.host = nullptr;
            set_error("rasterize_triangles: allocating %zu bytes of staging failed", cap);
            return VGHVIS_ERR_NOMEM;
        }
        s.bytes = cap;
    }
    if (need_boxes > s.box_bytes) {
        hipFree(s.boxes);
        s.boxes = nullptr;
        s.box_bytes = 0;
        if (hipMalloc((void**)&s.boxes, need_boxes) != hipSuccess) {
            set_error("rasterize_triangles: allocating %zu bytes of triangle boxes failed", need_boxes);
            return VGHVIS_ERR_NOMEM;
        }
        s.box_bytes = need_boxes;
    }
    return VGHVIS_OK;
}

}  // namespace

extern "C" VGHVIS_API const char* vghvis_version(void) { return "vghvis 1 (gfx950)"; }

extern "C" VGHVIS_API const char* vghvis_last_error(void) { return g_error; }

extern "C" VGHVIS_API int vghvis_rasterize_triangles(const vghvis_job* job, void* stream) {
    VIS_REQUIRE(job, "rasterize_triangles: null job");
    const vghvis_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    VIS_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHVIS_MAX_SIDE && j.width <= VGHVIS_MAX_SIDE, "rasterize_triangles: height x width %d x %d outside 1 .. %d",
                j.height, j.width, VGHVIS_MAX_SIDE);
    const int W = j.width, H = j.height, n = j.n_heads, V = j.n_vertices, T = j.n_triangles;
    VIS_REQUIRE(n >= 0 && n <= VGHVIS_MAX_HEADS, "rasterize_triangles: n_heads %d outside 0 .. %d", n, VGHVIS_MAX_HEADS);
    VIS_REQUIRE(V >= 0, "rasterize_triangles: n_vertices %d is negative", V);
    VIS_REQUIRE(T >= 0, "rasterize_triangles: n_triangles %d is negative", T);
    VIS_REQUIRE(j.mode == VGHVIS_MODE_ORDER || j.mode == VGHVIS_MODE_DEPTH, "rasterize_triangles: mode %d is neither 0 (order) nor 1 (depth)", j.mode);
    VIS_REQUIRE(j.z_sign == 1.0f || j.z_sign == -1.0f, "rasterize_triangles: z_sign %g is neither +1 nor -1", (double)j.z_sign);
    VIS_REQUIRE(j.depth_dev, "rasterize_triangles: null depth_dev");
    VIS_REQUIRE(j.triangle_dev, "rasterize_triangles: null triangle_dev");
    VIS_REQUIRE(j.head_dev, "rasterize_triangles: null head_dev");
    VIS_REQUIRE(!j.vertex_visible_dev || n == 0 || V >= 1, "rasterize_triangles: vertex_visible_dev with n_vertices %d", V);
    const bool raster = n > 0 && T > 0;
    if (raster) {
        VIS_REQUIRE(V >= 1, "rasterize_triangles: n_vertices %d with %d triangles", V, T);
        VIS_REQUIRE(j.verts_dev, "rasterize_triangles: null verts_dev");
        VIS_REQUIRE(j.triangles, "rasterize_triangles: null triangles");
        VIS_REQUIRE(j.bounds, "rasterize_triangles: null bounds");
        VIS_REQUIRE((int64_t)n * T <= INT32_MAX / 4 && (int64_t)n * V <= INT32_MAX / 4, "rasterize_triangles: n_heads * n_triangles = %lld or n_heads * n_vertices = %lld exceed one launch",
                    (long long)n * T, (long long)n * V);
        for (int64_t i = 0; i < (int64_t)T * 3; ++i)
            VIS_REQUIRE(j.triangles[i] >= 0 && j.triangles[i] < V, "rasterize_triangles: triangles: triangle %lld: index %d outside the %d vertices", (long long)(i / 3),
                        j.triangles[i], V);
        for (int i = 0; i < n; ++i) {
            const int32_t* b = j.bounds + 4 * i;
            const bool empty = b[2] < b[0] || b[3] < b[1];
            VIS_REQUIRE(empty || (b[0] >= 0 && b[1] >= 0 && b[2] < W && b[3] < H), "rasterize_triangles: bounds: head %d: (%d, %d, %d, %d) outside the image", i, b[0], b[1], b[2],
                        b[3]);
        }
    }
    // "tile -> heads in order" for the tiles some head touches: count, prefix, fill (heads are visited in order, so every list is ascending)
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
    }
    VIS_REQUIRE(n_pairs <= (size_t)INT32_MAX, "rasterize_triangles: %zu (tile, head) pairs exceed one launch", n_pairs);
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    VIS_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    // one upload: [triangles | tile_xy | tile_first | tile_heads], each from a 16-byte boundary
    const size_t at_xy = align16((size_t)T * 12), at_first = at_xy + align16(n_tiles * 4), at_heads = at_first + align16((n_tiles + 1) * 4);
    const size_t total = at_heads + align16(n_pairs * 4);
    if (n_tiles) {
        if (int rc = reserve(s, total, (size_t)n * T * sizeof(Box))) return rc;  // also waits for this device's previous call
        uint8_t* h = s.host;
        memcpy(h, j.triangles, (size_t)T * 12);
        uint32_t* xy = (uint32_t*)(h + at_xy);
        int32_t* first = (int32_t*)(h + at_first);
        int32_t* heads = (int32_t*)(h + at_heads);
        size_t k = 0, at = 0;
        for (size_t t = 0; t < (size_t)tiles_x * tiles_y; ++t) {  // grid[t] becomes the position of the tile's next head
            const int32_t c = grid[t];
            if (c) {
                xy[k] = (uint32_t)(t % tiles_x) | (uint32_t)(t / tiles_x) << 16;
                first[k++] = (int32_t)at;
            }
            grid[t] = (int32_t)at;
            at += (size_t)c;
        }
        first[k] = (int32_t)at;
        for (int i = 0; i < n; ++i) {
            const int32_t* b = j.bounds + 4 * i;
            if (b[2] < b[0] || b[3] < b[1]) continue;
            for (int ty = b[1] / TILE; ty <= b[3] / TILE; ++ty)
                for (int tx = b[0] / TILE; tx <= b[2] / TILE; ++tx) heads[grid[(size_t)ty * tiles_x + tx]++] = i;
        }
    }
    // from here on work is queued: the first failure is kept, nothing more is queued after it, and the event is recorded on every path so that the next
    // call never rewrites the staging block or the boxes under work that is still queued
    const size_t n_px = (size_t)H * W;
    hipError_t err = hipSuccess;
    const char* failed = "";
#define VIS_QUEUE(expr)                             \
    do {                                            \
        if (err == hipSuccess) {                    \
            err = (expr);                           \
            if (err != hipSuccess) failed = #expr;  \
        }                                           \
    } while (0)
    if (n_tiles) VIS_QUEUE(hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event below covers the staging block
    if (err == hipSuccess) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, n_px, j.depth_dev, j.triangle_dev, j.head_dev, j.bary_dev);
    if (n) {
        if (j.visible_px_dev) VIS_QUEUE(hipMemsetAsync(j.visible_px_dev, 0, (size_t)n * 4, st));
        if (j.covered_px_dev) VIS_QUEUE(hipMemsetAsync(j.covered_px_dev, 0, (size_t)n * 4, st));
        if (j.vertex_visible_dev) VIS_QUEUE(hipMemsetAsync(j.vertex_visible_dev, 0, (size_t)n * V, st));
    }
    if (n_tiles && err == hipSuccess) {
        const uint8_t* d = s.dev;
        hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)(n * T + 255) / 256), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, n * T, V, T, H, W, s.boxes);
        hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, (const Box*)s.boxes, (const uint32_t*)(d + at_xy),
                           (const int32_t*)(d + at_first), (const int32_t*)(d + at_heads), V, T, H, W, j.mode == VGHVIS_MODE_DEPTH ? 1 : 0, j.z_sign, j.depth_dev, j.triangle_dev,
                           j.head_dev, j.bary_dev, j.visible_px_dev, j.covered_px_dev, j.vertex_visible_dev);
    }
    VIS_QUEUE(hipGetLastError());
    if (n_tiles) {
        if (hipEventRecord(s.ev, st) == hipSuccess) {
            s.recorded = true;
        } else {
            hipStreamSynchronize(st);  // no event to wait for next time: wait now
            VIS_QUEUE(hipErrorUnknown);
        }
    }
#undef VIS_QUEUE
    if (err != hipSuccess) {
        set_error("rasterize_triangles: %s -> %s", failed, hipGetErrorString(err));
        return VGHVIS_ERR_HIP;
    }
    return VGHVIS_OK;
}
