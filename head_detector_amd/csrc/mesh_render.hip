// libvghview.so (include/vgh_view.h): the other half of Sim3DR (head_detector/Sim3DR/Sim3DR.py) -- `get_normal` and `_rasterize` with
// alpha < 1 -- and what they exist for: the lit, semi-transparent solid mesh over the photograph (PredictionResult.render_mesh).
//
// NORMALS (`_get_normal`, rasterize_kernel.cpp:158-215).  The reference adds every triangle's un-normalised cross product to its three
// corners, serially over triangles; float sums depend on their order, so each vertex adds its incident triangles in ASCENDING TRIANGLE
// INDEX, corner 0 before 1 before 2 (a vertex named twice by one triangle is added twice).  The host builds that list (a stable counting
// sort of the 3 T corners by vertex) and one lane per (head, vertex) walks it.  No float atomics: the result would depend on arrival order.
//
// BLENDED RASTERISER (`_rasterize`, :219-293).  With alpha < 1 a pixel is blended once for EVERY triangle that beats the running depth, in
// triangle order, and truncated to a byte each time, so the winner alone does not determine the byte: csrc/raster.hip's "atomic max, then
// resolve" cannot express it.  Per pixel the result is a fold over heads (in order, each with a fresh depth) and over the head's
// triangles in index order: the tile-major scheme of csrc/tile_fold.h (boxes, then tiles), with the pixel's bytes and depth in a lane's
// registers and one write per pixel at the end.
// All arithmetic is IEEE float32 in the reference's operation order (contraction off, true division, correctly rounded sqrt): normals
// and images are bit-identical to the reference's own C++ (tests/test_gpu_shaded_mesh.py).
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/vgh_view.h"
#include "tile_fold.h"

#pragma clang fp contract(off)

namespace {

using namespace tile_fold;
static_assert(VGHV_OK == OK && VGHV_ERR_INVALID == ERR_INVALID && VGHV_ERR_HIP == ERR_HIP && VGHV_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

// ---- normals, and the colours of the shaded mesh ----------------------------------------------------------------------------------------
struct Shade {
    float cr, cg, cb, ambient, diffuse, lx, ly, lz;
};

// One lane per (head, vertex).  first[v] .. first[v + 1] are the vertex's entries of `incident` (triangle indices, ascending, a triangle
// once per corner that names the vertex).  shade == 0: out = the normal; shade == 1: out = the colour of the lit vertex:
//   s = |(nx * lx + ny * ly) + nz * lz|,  t = a < 1 ? a : 1 with a = ambient + diffuse * s,  c_k = t * colour_k.
__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tri, const int32_t* __restrict__ first,
                                                      const int32_t* __restrict__ incident, int n_total, int V, float zsign, int shade, Shade sh, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    const int head = i / V, v = i - head * V;
    const float* p = verts + (size_t)head * V * 3;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    for (int e = first[v]; e < first[v + 1]; ++e) {
        const int t = incident[e];
        const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        const float ax = p[3 * i0], ay = p[3 * i0 + 1], az = zsign * p[3 * i0 + 2];
        const float v1x = p[3 * i1] - ax, v1y = p[3 * i1 + 1] - ay, v1z = zsign * p[3 * i1 + 2] - az;
        const float v2x = p[3 * i2] - ax, v2y = p[3 * i2 + 1] - ay, v2z = zsign * p[3 * i2 + 2] - az;
        nx += v1y * v2z - v1z * v2y;
        ny += v1z * v2x - v1x * v2z;
        nz += v1x * v2y - v1y * v2x;
    }
    float det = sqrtf(nx * nx + ny * ny + nz * nz);
    if (det <= 0) det = 1e-6f;
    nx = nx / det;
    ny = ny / det;
    nz = nz / det;
    float* o = out + (size_t)i * 3;
    if (shade) {
        const float s = fabsf((nx * sh.lx + ny * sh.ly) + nz * sh.lz);
        const float a = sh.ambient + sh.diffuse * s;
        const float t = a < 1.0f ? a : 1.0f;
        o[0] = t * sh.cr;
        o[1] = t * sh.cg;
        o[2] = t * sh.cb;
    } else {
        o[0] = nx;
        o[1] = ny;
        o[2] = nz;
    }
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------------------------
// What a lane needs of a triangle that overlaps the tile: the set-up, the three depths, the nine colour values and the box.  96 B x 256 = 24 KB
// of LDS a workgroup.
struct Hit : TriSetup {
    float d0, d1, d2;
    float c0[3], c1[3], c2[3];
    Box box;
};

// (unsigned char)((1 - alpha) * byte + alpha * 255 * p_color): truncation, the low 8 bits for in-range values (as csrc/raster.hip)
__device__ __forceinline__ uint32_t blend(uint32_t byte, float pc, float one_minus_alpha, float alpha255) {
    const float val = one_minus_alpha * (float)byte + alpha255 * pc;
    return (uint32_t)((int)val & 0xFF);
}

// blockIdx.x = an entry of the tile list: tile_xy = tile column | tile row << 16, its heads are tile_heads[tile_first[b] .. tile_first[b + 1]).
// colours: [V, 3] shared by all heads (colour_stride 0) or [n, V, 3] (colour_stride V * 3).
__global__ __launch_bounds__(256) void tiles_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tri, const float* __restrict__ colours, size_t colour_stride,
                                                    const Box* __restrict__ boxes, const uint32_t* __restrict__ tile_xy, const int32_t* __restrict__ tile_first,
                                                    const int32_t* __restrict__ tile_heads, int V, int T, int h, int w, int reverse, float zsign, float alpha,
                                                    const uint8_t* __restrict__ src, int64_t src_pitch, uint8_t* __restrict__ dst) {
    __shared__ Hit hits[256];
    __shared__ int wave_hits[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t xy = tile_xy[blockIdx.x];
    const int tx0 = (int)(xy & 0xffffu) * TILE, ty0 = (int)(xy >> 16) * TILE;
    const int tx1 = min(tx0 + TILE - 1, w - 1), ty1 = min(ty0 + TILE - 1, h - 1);
    const int x = tx0 + (tid & (TILE - 1)), y = ty0 + (tid >> 4);
    const bool live = x < w && y < h;
    const size_t row = (size_t)(reverse ? h - 1 - y : y);  // `reverse` flips the row that is read and written, not the geometry's
    uint32_t q0 = 0, q1 = 0, q2 = 0;
    if (live) {
        const uint8_t* s = src + row * (size_t)src_pitch + (size_t)x * 3;
        q0 = s[0];
        q1 = s[1];
        q2 = s[2];
    }
    const float px = (float)x, py = (float)y;
    const float one_minus_alpha = 1.0f - alpha, alpha255 = alpha * 255.0f;
    for (int e = tile_first[blockIdx.x]; e < tile_first[blockIdx.x + 1]; ++e) {
        const int head = tile_heads[e];
        const float* p = verts + (size_t)head * V * 3;
        const float* col = colours + (size_t)head * colour_stride;
        const Box* hb = boxes + (size_t)head * T;
        float depth = BACKGROUND;  // a fresh depth buffer for every head (Sim3DR.py:30)
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
                for (int c = 0; c < 3; ++c) {
                    k.c0[c] = col[3 * i0 + c];
                    k.c1[c] = col[3 * i1 + c];
                    k.c2[c] = col[3 * i2 + c];
                }
                k.box = b;
                hits[slot] = k;
            }
            __syncthreads();
            for (int s = 0; s < count; ++s) {
                const Hit& k = hits[s];  // every lane reads the same entry: a broadcast
                // the triangle's own box, per pixel: in float arithmetic all three weights can be positive one pixel outside it
                if (x < k.box.x0 || x > k.box.x1 || y < k.box.y0 || y > k.box.y1) continue;
                float u, v;
                tri_uv(k, px, py, u, v);
                const float w0 = 1.0f - u - v, w1 = v, w2 = u;  // get_point_weight
                if (w2 > 0 && w1 > 0 && w0 > 0) {
                    const float pd = w0 * k.d0 + w1 * k.d1 + w2 * k.d2;
                    if (pd > depth) {  // false for NaN; -0 and +0 compare equal, as in the reference
                        q0 = blend(q0, w0 * k.c0[0] + w1 * k.c1[0] + w2 * k.c2[0], one_minus_alpha, alpha255);
                        q1 = blend(q1, w0 * k.c0[1] + w1 * k.c1[1] + w2 * k.c2[1], one_minus_alpha, alpha255);
                        q2 = blend(q2, w0 * k.c0[2] + w1 * k.c1[2] + w2 * k.c2[2], one_minus_alpha, alpha255);
                        depth = pd;
                    }
                }
            }
        }
    }
    if (live) {
        uint8_t* o = dst + (row * (size_t)w + (size_t)x) * 3;
        o[0] = (uint8_t)q0;
        o[1] = (uint8_t)q1;
        o[2] = (uint8_t)q2;
    }
}

std::mutex g_mutex;
std::map<int, State> g_state;

// every triangle index against V
int check_triangles(const char* who, const int32_t* triangles, int T, int V) {
    const int64_t bad = first_bad_index(triangles, (int64_t)T * 3, V);
    CH_REQUIRE(bad < 0, "%s: triangle %lld: index %d outside the %d vertices", who, (long long)(bad / 3), triangles[bad], V);
    return OK;
}

// [first (V + 1) | incident (3 T)]: a stable counting sort of the 3 T corners by vertex, so that a vertex's triangles come in ascending index
void build_incidence(const int32_t* triangles, int T, int V, int32_t* first, int32_t* incident) {
    memset(first, 0, ((size_t)V + 1) * sizeof(int32_t));
    for (int64_t i = 0; i < (int64_t)T * 3; ++i) first[triangles[i] + 1]++;
    for (int v = 0; v < V; ++v) first[v + 1] += first[v];
    std::vector<int32_t> at(first, first + V);
    for (int64_t i = 0; i < (int64_t)T * 3; ++i) incident[at[triangles[i]]++] = (int32_t)(i / 3);
}

size_t incidence_bytes(int T, int V) { return align16(((size_t)V + 1) * 4) + align16((size_t)T * 12); }

void launch_normals(const float* verts, const uint8_t* d_tri, const uint8_t* d_inc, int n, int V, float zsign, int shade, const Shade& sh, float* out, hipStream_t st) {
    const int total = n * V;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)(total + 255) / 256), dim3(256), 0, st, verts, (const int32_t*)d_tri, (const int32_t*)d_inc,
                       (const int32_t*)(d_inc + align16(((size_t)V + 1) * 4)), total, V, zsign, shade, sh, out);
}

}  // namespace

extern "C" VGHV_API int vghv_vertex_normals(const float* verts_dev, int n, int V, const int32_t* triangles, int T, float* normals_dev, void* stream) {
    CH_REQUIRE(n >= 0 && V >= 1 && T >= 0, "vertex_normals: bad sizes (n %d, V %d, T %d)", n, V, T);
    CH_REQUIRE((int64_t)n * V <= INT32_MAX / 4 && T <= INT32_MAX / 4, "vertex_normals: %lld vertices or %d triangles exceed one launch", (long long)n * V, T);
    if (n == 0) return OK;
    CH_REQUIRE(verts_dev && normals_dev, "vertex_normals: null vertices or normals (verts_dev %p, normals_dev %p)", (const void*)verts_dev, (void*)normals_dev);
    CH_REQUIRE(triangles || T == 0, "vertex_normals: null triangles");
    CH_REQUIRE(verts_dev != normals_dev, "vertex_normals: normals_dev overlaps verts_dev");
    if (int rc = check_triangles("vertex_normals", triangles, T, V)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    const size_t at_inc = align16((size_t)T * 12), total = at_inc + incidence_bytes(T, V);
    if (int rc = reserve(s, total, 0, "vertex_normals")) return rc;
    uint8_t* h = s.host;
    if (T) memcpy(h, triangles, (size_t)T * 12);
    build_incidence(triangles, T, V, (int32_t*)(h + at_inc), (int32_t*)(h + at_inc + align16(((size_t)V + 1) * 4)));
    Queue q;  // from here on work is queued (companion_host.h, queue-then-record)
    CH_QUEUE(q, hipMemcpyAsync(s.dev, h, total, hipMemcpyHostToDevice, st));
    if (q.ok()) launch_normals(verts_dev, s.dev, s.dev + at_inc, n, V, 1.0f, 0, Shade{}, normals_dev, st);
    return finish(q, s, true, st, "vertex_normals");
}

extern "C" VGHV_API int vghv_render_meshes(const vghv_mesh_job* job, void* stream) {
    CH_REQUIRE(job, "render_meshes: null job");
    const vghv_mesh_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.src_dev && j.dst_dev, "render_meshes: null image (src_dev %p, dst_dev %p)", (const void*)j.src_dev, (void*)j.dst_dev);
    CH_REQUIRE(j.channels == 3, "render_meshes: %d channels (needs 3: u8 RGB)", j.channels);
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHV_MAX_SIDE && j.width <= VGHV_MAX_SIDE, "render_meshes: image %d x %d outside 1 .. %d", j.height, j.width,
               VGHV_MAX_SIDE);
    CH_REQUIRE(j.src_pitch_bytes >= (int64_t)j.width * 3, "render_meshes: src_pitch_bytes %lld < width * 3 = %lld", (long long)j.src_pitch_bytes, (long long)j.width * 3);
    const int W = j.width, H = j.height, n = j.n_heads, V = j.n_vertices, T = j.n_triangles;
    {
        const uintptr_t s0 = (uintptr_t)j.src_dev, s1 = s0 + (size_t)(H - 1) * (size_t)j.src_pitch_bytes + (size_t)W * 3, d0 = (uintptr_t)j.dst_dev, d1 = d0 + (size_t)H * W * 3;
        CH_REQUIRE(s1 <= d0 || d1 <= s0, "render_meshes: dst_dev overlaps src_dev");
    }
    CH_REQUIRE(n >= 0 && n <= VGHV_MAX_DRAW_HEADS, "render_meshes: %d heads outside 0 .. %d", n, VGHV_MAX_DRAW_HEADS);
    CH_REQUIRE(V >= 0 && T >= 0, "render_meshes: negative count");
    CH_REQUIRE(j.alpha >= 0.0f && j.alpha <= 1.0f, "render_meshes: alpha %g outside 0 .. 1", (double)j.alpha);
    CH_REQUIRE(j.z_sign == 1.0f || j.z_sign == -1.0f, "render_meshes: z_sign %g is neither +1 nor -1", (double)j.z_sign);
    CH_REQUIRE(j.shade == 0 || j.shade == 1, "render_meshes: shade %d is neither 0 nor 1", j.shade);
    CH_REQUIRE(j.colors_per_head == 0 || j.colors_per_head == 1, "render_meshes: colors_per_head %d is neither 0 nor 1", j.colors_per_head);
    const bool paint = n > 0 && T > 0;
    if (paint) {
        CH_REQUIRE(V >= 1 && j.verts_dev && j.triangles && j.bounds && j.colors_dev, "render_meshes: null vertices, triangles, bounds or colours (n_vertices %d)", V);
        CH_REQUIRE((int64_t)n * T <= INT32_MAX / 4 && (int64_t)n * V <= INT32_MAX / 4, "render_meshes: %lld triangles or %lld vertices exceed one launch", (long long)n * T,
                   (long long)n * V);
        CH_REQUIRE(!j.shade || j.colors_per_head, "render_meshes: shading writes one colour table per head (colors_per_head must be 1)");
        if (j.shade) {
            const float c[8] = {j.color[0], j.color[1], j.color[2], j.ambient, j.diffuse, j.light[0], j.light[1], j.light[2]};
            for (int i = 0; i < 8; ++i) CH_REQUIRE(c[i] == c[i] && c[i] - c[i] == 0.0f, "render_meshes: a shading constant is not finite");
            CH_REQUIRE(j.color[0] >= 0 && j.color[0] <= 1 && j.color[1] >= 0 && j.color[1] <= 1 && j.color[2] >= 0 && j.color[2] <= 1 && j.ambient >= 0 && j.diffuse >= 0,
                       "render_meshes: colour outside 0 .. 1 or negative ambient / diffuse");
        }
        if (int rc = check_triangles("render_meshes", j.triangles, T, V)) return rc;
        if (const int i = first_bad_bound(j.bounds, n, W, H); i >= 0) {
            const int32_t* b = j.bounds + 4 * i;
            CH_REQUIRE(false, "render_meshes: head %d: bounds (%d, %d, %d, %d) outside the image", i, b[0], b[1], b[2], b[3]);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    TileLists lists;
    if (paint) lists.count(j.bounds, n, W, H);
    const size_t n_tiles = lists.n_tiles, n_pairs = lists.n_pairs;
    CH_REQUIRE(n_pairs <= (size_t)INT32_MAX, "render_meshes: %zu (tile, head) pairs exceed one launch", n_pairs);
    const bool tiles = n_tiles > 0, work = tiles || (paint && j.shade);  // with shade the colours are written even when no head touches the image
    // one upload: [triangles | first, incident (shading only) | tile_xy | tile_first | tile_heads], each from a 16-byte boundary
    const size_t at_inc = align16((size_t)T * 12), at_xy = at_inc + (work && j.shade ? incidence_bytes(T, V) : 0), at_first = at_xy + align16(n_tiles * 4);
    const size_t at_heads = at_first + align16((n_tiles + 1) * 4), total = at_heads + align16(n_pairs * 4);
    if (work) {
        if (int rc = reserve(s, total, tiles ? (size_t)n * T * sizeof(Box) : 0, "render_meshes")) return rc;  // also waits for this device's previous call
        uint8_t* h = s.host;
        memcpy(h, j.triangles, (size_t)T * 12);
        if (j.shade) build_incidence(j.triangles, T, V, (int32_t*)(h + at_inc), (int32_t*)(h + at_inc + align16(((size_t)V + 1) * 4)));
        lists.fill((uint32_t*)(h + at_xy), (int32_t*)(h + at_first), (int32_t*)(h + at_heads));
    }
    // from here on work is queued (companion_host.h, queue-then-record).  dst = src everywhere; the tiles that some head touches are then rewritten from src
    Queue q;
    CH_QUEUE(q, hipMemcpy2DAsync(j.dst_dev, (size_t)W * 3, j.src_dev, (size_t)j.src_pitch_bytes, (size_t)W * 3, (size_t)H, hipMemcpyDeviceToDevice, st));
    const uint8_t* d = s.dev;
    if (work) CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));
    if (work && j.shade && q.ok()) {
        const Shade sh = {j.color[0], j.color[1], j.color[2], j.ambient, j.diffuse, j.light[0], j.light[1], j.light[2]};
        launch_normals(j.verts_dev, d, d + at_inc, n, V, j.z_sign, 1, sh, j.colors_dev, st);
    }
    if (tiles && q.ok()) {
        hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)(n * T + 255) / 256), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, n * T, V, T, H, W, s.boxes.ptr);
        hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, (const float*)j.colors_dev,
                           j.colors_per_head ? (size_t)V * 3 : (size_t)0, (const Box*)s.boxes.ptr, (const uint32_t*)(d + at_xy), (const int32_t*)(d + at_first),
                           (const int32_t*)(d + at_heads), V, T, H, W, j.reverse ? 1 : 0, j.z_sign, j.alpha, j.src_dev, j.src_pitch_bytes, j.dst_dev);
    }
    return finish(q, s, work, st, "render_meshes");
}
