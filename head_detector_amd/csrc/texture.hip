// libvghtex.so (include/vgh_tex.h): Sim3DR's `render_texture` (`_render_texture_core`, head_detector/Sim3DR/lib/rasterize_kernel.cpp:358-463), the
// z-buffered rasteriser that paints a mesh from a texture image through per-vertex texture coordinates, for all heads of an image at once and in both
// directions: onto the photograph (wrap) or, with the UV atlas as the image and the photograph as the texture, into one atlas per head (unwrap).
//
// Per pixel the result is a serial fold over heads (in order) and over the head's triangles (in index order): the tile-major scheme of csrc/tile_fold.h
// (fill, then boxes, then tiles; with one destination per head every (head, tile) pair is a workgroup of its own), with depth, owner and the winner's
// clamped texture position in a lane's registers.  88 B a triangle, 22 KB of LDS a workgroup, so seven workgroups share a CU's 160 KB.
// In the reference every win rewrites the pixel's colour and only the last one stays, and the colour depends on nothing but the winner's texture
// position: the lane looks the texture up once, after the fold.  No atomics anywhere.
// The INSIDE RULE is  x < 2 || x > w - 3 || y < 2 || y > h - 3 || is_point_in_tri:  in a frame two pixels wide every pixel of a triangle's box counts.
// All arithmetic is IEEE float32 in the reference's operation order (contraction off, true division): every output is bit-identical to the
// reference's own C++ (tests/test_gpu_texture.py).
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_tex.h"
#include "tile_fold.h"

#pragma clang fp contract(off)

namespace {

using namespace tile_fold;
static_assert(VGHTEX_OK == OK && VGHTEX_ERR_INVALID == ERR_INVALID && VGHTEX_ERR_HIP == ERR_HIP && VGHTEX_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

// ---- the background of depth, triangle and head ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_kernel(size_t n_px, float* __restrict__ depth, int32_t* __restrict__ tri, int32_t* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    depth[i] = BACKGROUND;
    if (tri) tri[i] = -1;
    if (head) head[i] = -1;
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------------------------------
// What a lane needs of a triangle that overlaps the tile: the set-up, the three depths, the three texture corners, the triangle's index and the box.
// 88 B x 256 = 22 KB of LDS a workgroup.
struct Hit : TriSetup {
    float d0, d1, d2;
    float q0x, q0y, q1x, q1y, q2x, q2y;
    int32_t t;
    Box box;
};

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

std::mutex g_mutex;
std::map<int, State> g_state;

inline bool is_flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace

extern "C" VGHTEX_API const char* vghtex_version(void) { return "vghtex 1 (gfx950)"; }

extern "C" VGHTEX_API const char* vghtex_last_error(void) { return last_error(); }

extern "C" VGHTEX_API int vghtex_render_texture(const vghtex_job* job, void* stream) {
    CH_REQUIRE(job, "render_texture: null job");
    const vghtex_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHTEX_MAX_SIDE && j.width <= VGHTEX_MAX_SIDE, "render_texture: height x width %d x %d outside 1 .. %d", j.height,
               j.width, VGHTEX_MAX_SIDE);
    const int W = j.width, H = j.height, n = j.n_heads, V = j.n_vertices, T = j.n_triangles, Vt = j.n_tex_vertices, c = j.channels;
    CH_REQUIRE(c >= 1 && c <= VGHTEX_MAX_CHANNELS, "render_texture: channels %d outside 1 .. %d", c, VGHTEX_MAX_CHANNELS);
    CH_REQUIRE(n >= 0 && n <= VGHTEX_MAX_HEADS, "render_texture: n_heads %d outside 0 .. %d", n, VGHTEX_MAX_HEADS);
    CH_REQUIRE(V >= 0, "render_texture: n_vertices %d is negative", V);
    CH_REQUIRE(T >= 0, "render_texture: n_triangles %d is negative", T);
    CH_REQUIRE(Vt >= 0, "render_texture: n_tex_vertices %d is negative", Vt);
    CH_REQUIRE(j.tex_height >= 1 && j.tex_width >= 1 && j.tex_height <= VGHTEX_MAX_SIDE && j.tex_width <= VGHTEX_MAX_SIDE,
               "render_texture: tex_height x tex_width %d x %d outside 1 .. %d", j.tex_height, j.tex_width, VGHTEX_MAX_SIDE);
    CH_REQUIRE(j.tex_channels >= c, "render_texture: tex_channels %d below channels %d", j.tex_channels, c);
    CH_REQUIRE(j.tex_dtype == VGHTEX_TEX_F32 || j.tex_dtype == VGHTEX_TEX_U8, "render_texture: tex_dtype %d is neither 0 (f32) nor 1 (u8)", j.tex_dtype);
    CH_REQUIRE(is_flag(j.tex_per_head), "render_texture: tex_per_head %d is neither 0 nor 1", j.tex_per_head);
    CH_REQUIRE(is_flag(j.tex_coords_per_head), "render_texture: tex_coords_per_head %d is neither 0 nor 1", j.tex_coords_per_head);
    CH_REQUIRE(is_flag(j.dst_per_head), "render_texture: dst_per_head %d is neither 0 nor 1", j.dst_per_head);
    CH_REQUIRE(j.mapping == VGHTEX_MAP_NEAREST || j.mapping == VGHTEX_MAP_BILINEAR, "render_texture: mapping %d is neither 0 (nearest) nor 1 (bilinear)", j.mapping);
    CH_REQUIRE(j.mode == VGHTEX_MODE_ORDER || j.mode == VGHTEX_MODE_DEPTH, "render_texture: mode %d is neither 0 (order) nor 1 (depth)", j.mode);
    CH_REQUIRE(j.z_sign == 1.0f || j.z_sign == -1.0f, "render_texture: z_sign %g is neither +1 nor -1", (double)j.z_sign);
    const size_t slices = j.dst_per_head ? (size_t)n : 1;
    const size_t n_px = slices * (size_t)H * (size_t)W;
    CH_REQUIRE(n_px / 256 < (size_t)INT32_MAX, "render_texture: %zu destination pixels exceed one launch", n_px);
    if (n_px) {
        CH_REQUIRE(j.dst_dev, "render_texture: null dst_dev");
        CH_REQUIRE(j.depth_dev, "render_texture: null depth_dev");
    }
    const bool raster = n > 0 && T > 0;
    if (raster) {
        CH_REQUIRE(V >= 1, "render_texture: n_vertices %d with %d triangles", V, T);
        CH_REQUIRE(Vt >= 1, "render_texture: n_tex_vertices %d with %d triangles", Vt, T);
        CH_REQUIRE(j.verts_dev, "render_texture: null verts_dev");
        CH_REQUIRE(j.triangles, "render_texture: null triangles");
        CH_REQUIRE(j.tex_coords_dev, "render_texture: null tex_coords_dev");
        CH_REQUIRE(j.tex_triangles, "render_texture: null tex_triangles");
        CH_REQUIRE(j.texture_dev, "render_texture: null texture_dev");
        CH_REQUIRE(j.bounds, "render_texture: null bounds");
        CH_REQUIRE((int64_t)n * T <= INT32_MAX / 4 && (int64_t)n * V <= INT32_MAX / 4 && (int64_t)n * Vt <= INT32_MAX / 4,
                   "render_texture: n_heads * n_triangles = %lld, n_heads * n_vertices = %lld or n_heads * n_tex_vertices = %lld exceed one launch", (long long)n * T,
                   (long long)n * V, (long long)n * Vt);
        // a mesh index reads a vertex and, for the corner's texture y, a texture coordinate
        const int64_t bad = first_bad_index(j.triangles, (int64_t)T * 3, V < Vt ? V : Vt), bad_tex = first_bad_index(j.tex_triangles, (int64_t)T * 3, Vt);
        // what is reported is what one pass over the corners, looking at triangles[i] before tex_triangles[i], meets first: the earlier corner, the mesh's on a tie
        if (bad >= 0 && (bad_tex < 0 || bad <= bad_tex)) {
            const int32_t v = j.triangles[bad];
            CH_REQUIRE(v >= 0 && v < V, "render_texture: triangles: triangle %lld: index %d outside the %d vertices", (long long)(bad / 3), v, V);
            CH_REQUIRE(false, "render_texture: triangles: triangle %lld: index %d outside the %d texture coordinates (a corner's texture y is read through it)", (long long)(bad / 3), v, Vt);
        }
        CH_REQUIRE(bad_tex < 0, "render_texture: tex_triangles: triangle %lld: index %d outside the %d texture coordinates", (long long)(bad_tex / 3), j.tex_triangles[bad_tex], Vt);
        if (const int i = first_bad_bound(j.bounds, n, W, H); i >= 0) {
            const int32_t* b = j.bounds + 4 * i;
            CH_REQUIRE(false, "render_texture: bounds: head %d: (%d, %d, %d, %d) outside the image", i, b[0], b[1], b[2], b[3]);
        }
    }
    TileLists lists;
    if (raster) lists.count(j.bounds, n, W, H, j.dst_per_head != 0);
    const size_t n_tiles = lists.n_tiles, n_pairs = lists.n_pairs;
    CH_REQUIRE(n_pairs <= (size_t)INT32_MAX, "render_texture: %zu (tile, head) pairs exceed one launch", n_pairs);
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    State& s = g_state[device];
    // one upload: [triangles | tex_triangles | tile_xy | tile_first | tile_heads], each from a 16-byte boundary
    const size_t at_tt = align16((size_t)T * 12), at_xy = at_tt + align16((size_t)T * 12), at_first = at_xy + align16(n_tiles * 4), at_heads = at_first + align16((n_tiles + 1) * 4);
    const size_t total = at_heads + align16(n_pairs * 4);
    if (n_tiles) {
        if (int rc = reserve(s, total, (size_t)n * T * sizeof(Box), "render_texture")) return rc;  // also waits for this device's previous call
        uint8_t* h = s.host;
        memcpy(h, j.triangles, (size_t)T * 12);
        memcpy(h + at_tt, j.tex_triangles, (size_t)T * 12);
        lists.fill((uint32_t*)(h + at_xy), (int32_t*)(h + at_first), (int32_t*)(h + at_heads));
    }
    // from here on work is queued (companion_host.h, queue-then-record)
    Queue q;
    if (n_tiles) CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event covers the staging block
    if (n_px && q.ok()) hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, n_px, j.depth_dev, j.triangle_dev, j.head_dev);
    if (n_tiles && q.ok()) {
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
        hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)(n * T + 255) / 256), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, n * T, V, T, H, W, s.boxes.ptr);
        hipLaunchKernelGGL(tiles_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, j.verts_dev, (const int32_t*)d, (const int32_t*)(d + at_tt), (const Box*)s.boxes.ptr,
                           (const uint32_t*)(d + at_xy), (const int32_t*)(d + at_first), (const int32_t*)(d + at_heads), ta, V, T, H, W, c, j.mode == VGHTEX_MODE_DEPTH ? 1 : 0,
                           j.dst_per_head, j.z_sign, j.dst_dev, j.depth_dev, j.triangle_dev, j.head_dev);
    }
    return finish(q, s, n_tiles != 0, st, "render_texture");
}
