// libvghvis.so (include/vgh_vis.h): the third function of Sim3DR's binding, `rasterize_triangles` (`_rasterize_triangles`,
// head_detector/Sim3DR/lib/rasterize_kernel.cpp:295-353), for all heads of an image at once: per pixel the head, the triangle, the depth and the
// barycentric weights that show, and per head how many pixels it covers alone, how many of them remain its own, and which of its vertices can be seen.
//
// Per pixel the result is a serial fold over heads (in order) and over the head's triangles (in index order): the tile-major scheme of csrc/tile_fold.h
// (fill, then boxes, then tiles), with depth, owner and weights in a lane's registers.
// The INSIDE RULE is is_point_in_tri's  u >= 0 && v >= 0 && u + v < 1,  not the  w0 > 0 && w1 > 0 && w2 > 0  of `_rasterize`: an edge or corner on a
// pixel centre belongs to the triangle, and a zero-determinant triangle (inverDeno = 0, so u = v = 0) holds every pixel of its box with weights
// (1, 0, 0).  is_point_in_tri and get_point_weight compute u and v by the same operations, so one evaluation serves the test and the weights.
// No 64-bit keys, no atomics on depth; the pixel counts are integer atomics (order-independent), the vertex flags same-value byte stores.
// All arithmetic is IEEE float32 in the reference's operation order (contraction off, true division): every output is bit-identical to the
// reference's own C++ (tests/test_gpu_visibility.py).
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_vis.h"
#include "tile_fold.h"

#pragma clang fp contract(off)

namespace {

using namespace tile_fold;
static_assert(VGHVIS_OK == OK && VGHVIS_ERR_INVALID == ERR_INVALID && VGHVIS_ERR_HIP == ERR_HIP && VGHVIS_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

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

// ---- tiles ----------------------------------------------------------------------------------------------------------------------------------------
// What a lane needs of a triangle that overlaps the tile: the set-up, the three depths, the triangle's index and the box.  64 B x 256 = 16 KB of LDS a
// workgroup.
struct Hit : TriSetup {
    float d0, d1, d2;
    int32_t t;
    Box box;
};

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
            compact_hits(hit, wave_hits, lane, wave, slot, count);  // declares both
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

std::mutex g_mutex;
std::map<int, State> g_state;

}  // namespace

extern "C" VGHVIS_API const char* vghvis_version(void) { return "vghvis 1 (gfx950)"; }

extern "C" VGHVIS_API const char* vghvis_last_error(void) { return last_error(); }

extern "C" VGHVIS_API int vghvis_rasterize_triangles(const vghvis_job* job, void* stream) {
    CH_REQUIRE(job, "rasterize_triangles: null job");
    const vghvis_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHVIS_MAX_SIDE && j.width <= VGHVIS_MAX_SIDE, "rasterize_triangles: height x width %d x %d outside 1 .. %d",
               j.height, j.width, VGHVIS_MAX_SIDE);
    const int W = j.width, H = j.height, n = j.n_heads, V = j.n_vertices, T = j.n_triangles;
    CH_REQUIRE(n >= 0 && n <= VGHVIS_MAX_HEADS, "rasterize_triangles: n_heads %d outside 0 .. %d", n, VGHVIS_MAX_HEADS);
    CH_REQUIRE(V >= 0, "rasterize_triangles: n_vertices %d is negative", V);
    CH_REQUIRE(T >= 0, "rasterize_triangles: n_triangles %d is negative", T);
    CH_REQUIRE(j.mode == VGHVIS_MODE_ORDER || j.mode == VGHVIS_MODE_DEPTH, "rasterize_triangles: mode %d is neither 0 (order) nor 1 (depth)", j.mode);
    CH_REQUIRE(j.z_sign == 1.0f || j.z_sign == -1.0f, "rasterize_triangles: z_sign %g is neither +1 nor -1", (double)j.z_sign);
    CH_REQUIRE(j.depth_dev, "rasterize_triangles: null depth_dev");
    CH_REQUIRE(j.triangle_dev, "rasterize_triangles: null triangle_dev");
    CH_REQUIRE(j.head_dev, "rasterize_triangles: null head_dev");
    CH_REQUIRE(!j.vertex_visible_dev || n == 0 || V >= 1, "rasterize_triangles: vertex_visible_dev with n_vertices %d", V);
    const bool raster = n > 0 && T > 0;
    if (raster) {
        CH_REQUIRE(V >= 1, "rasterize_triangles: n_vertices %d with %d triangles", V, T);
        CH_REQUIRE(j.verts_dev, "rasterize_triangles: null verts_dev");
        CH_REQUIRE(j.triangles, "rasterize_triangles: null triangles");
        CH_REQUIRE(j.bounds, "rasterize_triangles: null bounds");
        CH_REQUIRE((int64_t)n * T <= INT32_MAX / 4 && (int64_t)n * V <= INT32_MAX / 4, "rasterize_triangles: n_heads * n_triangles = %lld or n_heads * n_vertices = %lld exceed one launch",
                   (long long)n * T, (long long)n * V);
        const int64_t bad = first_bad_index(j.triangles, (int64_t)T * 3, V);
        CH_REQUIRE(bad < 0, "rasterize_triangles: triangles: triangle %lld: index %d outside the %d vertices", (long long)(bad / 3), j.triangles[bad], V);
        if (const int i = first_bad_bound(j.bounds, n, W, H); i >= 0) {
            const int32_t* b = j.bounds + 4 * i;
            CH_REQUIRE(false, "rasterize_triangles: bounds: head %d: (%d, %d, %d, %d) outside the image", i, b[0], b[1], b[2], b[3]);
        }
    }
    TileLists lists;
    if (raster) lists.count(j.bounds, n, W, H);
    const size_t n_tiles = lists.n_tiles, n_pairs = lists.n_pairs;
    CH_REQUIRE(n_pairs <= (size_t)INT32_MAX, "rasterize_triangles: %zu (tile, head) pairs exceed one launch", n_pairs);
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    // one upload: [triangles | tile_xy | tile_first | tile_heads], each from a 16-byte boundary
    const size_t at_xy = align16((size_t)T * 12), at_first = at_xy + align16(n_tiles * 4), at_heads = at_first + align16((n_tiles + 1) * 4);
    const size_t total = at_heads + align16(n_pairs * 4);
    if (n_tiles) {
        if (int rc = reserve(s, total, (size_t)n * T * sizeof(Box), "rasterize_triangles")) return rc;  // also waits for this device's previous call
        uint8_t* h = s.host;
        memcpy(h, j.triangles, (size_t)T * 12);
        lists.fill((uint32_t*)(h + at_xy), (int32_t*)(h + at_first), (int32_t*)(h + at_heads));
    }
    // from here on work is queued (companion_host.h, queue-then-record)
    const size_t n_px = (size_t)H * W;
    Queue q;
    if (n_tiles) CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event covers the staging block
    if (q.ok()) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, n_px, j.depth_dev, j.triangle_dev, j.head_dev, j.bary_dev);
    if (n) {
        if (j.visible_px_dev) CH_QUEUE(q, hipMemsetAsync(j.visible_px_dev, 0, (size_t)n * 4, st));
        if (j.covered_px_dev) CH_QUEUE(q, hipMemsetAsync(j.covered_px_dev, 0, (size_t)n * 4, st));
        if (j.vertex_visible_dev) CH_QUEUE(q, hipMemsetAsync(j.vertex_visible_dev, 0, (size_t)n * V, st));
    }
    if (n_tiles && q.ok()) {
        const uint8_t* d = s.dev;
        hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)(n * T + 255) / 256), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, n * T, V, T, H, W, s.boxes.ptr);
        hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, (const Box*)s.boxes.ptr, (const uint32_t*)(d + at_xy),
                           (const int32_t*)(d + at_first), (const int32_t*)(d + at_heads), V, T, H, W, j.mode == VGHVIS_MODE_DEPTH ? 1 : 0, j.z_sign, j.depth_dev, j.triangle_dev,
                           j.head_dev, j.bary_dev, j.visible_px_dev, j.covered_px_dev, j.vertex_visible_dev);
    }
    return finish(q, s, n_tiles != 0, st, "rasterize_triangles");
}
