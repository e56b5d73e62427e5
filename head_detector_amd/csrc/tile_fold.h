// The tile-major triangle fold that csrc/mesh_render.hip (libvghview.so), csrc/visibility.hip (libvghvis.so) and csrc/texture.hip (libvghtex.so) share,
// and the host half of it (argument scans, TileLists, the per-device State); the plumbing every companion library needs is csrc/companion_host.h.
// Header-only and internal: every definition has internal linkage or is inline, so each library compiles its own copy
// and stays a library of its own (no shared object, no exported symbol, no link dependency).
//
// A pixel of Sim3DR's rasterisers is a serial fold over heads (in order) and over the head's triangles (in index order).  Tile-major:
//   boxes    one lane per (head, triangle): the triangle's clamped integer bounding box as 4 x int16 (8 B a triangle for the scans below)
//   tiles    one 256-lane workgroup per 16 x 16 tile that some head touches (TileLists builds "tile -> heads in order" from the per-head pixel
//            bounds); a lane owns one pixel and keeps its state in registers.  For every head of the tile the workgroup scans the head's boxes 256
//            at a time, compacts the ones that overlap the tile IN INDEX ORDER into LDS (compact_hits) together with their pixel-independent set-up
//            (TriSetup), and every lane then walks that list serially with exactly the reference's arithmetic.  Deterministic, no float atomics,
//            launches independent of the head count.
// What a library does with a triangle (its Hit payload, its inside rule, what a win changes, the write-back) is the library's; so is its fold loop.
// All arithmetic is IEEE float32 in the reference's operation order: contraction is off here and in every includer.
#pragma once
#include <vector>

#include "companion_host.h"

#pragma clang fp contract(off)

namespace tile_fold {
using namespace companion;
namespace {

constexpr int TILE = 16;             // 16 x 16 pixels = the 256 lanes of a workgroup
constexpr float BACKGROUND = -1e8f;  // what Sim3DR's callers initialise the depth buffer with (Sim3DR.py:31)

// ---- the triangle's integer box (rasterize_kernel.cpp:245-253, :321-329, :406-415) -----------------------------------------------------------------
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
        if (x_max >= x_min && y_max >= y_min) b = {(int16_t)x_min, (int16_t)y_min, (int16_t)x_max, (int16_t)y_max};  // w, h <= the library's MAX_SIDE = 32767
    }
    boxes[i] = b;
}

// ---- the pixel-independent part of is_point_in_tri / get_point_weight (rasterize_kernel.cpp:26-82); a library's Hit derives from it ----------------
struct TriSetup {
    float p0x, p0y, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv;
};

// p0x, p0y are set by the caller
__device__ __forceinline__ void tri_setup(TriSetup& t, float p1x, float p1y, float p2x, float p2y) {
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
// the weights of the pixel are (1 - u - v, v, u)
__device__ __forceinline__ void tri_uv(const TriSetup& t, float px, float py, float& u, float& v) {
    const float v2x = px - t.p0x, v2y = py - t.p0y;
    const float dot02 = t.v0x * v2x + t.v0y * v2y;
    const float dot12 = t.v1x * v2x + t.v1y * v2y;
    u = (t.dot11 * dot02 - t.dot01 * dot12) * t.inv;
    v = (t.dot00 * dot12 - t.dot01 * dot02) * t.inv;
}

// ---- the top of every 256-triangle chunk ---------------------------------------------------------------------------------------------------------------
// compact_hits(hit, wave_hits, lane, wave, slot, count): all 256 lanes reach it with `hit` = the lane's triangle overlaps the tile; it declares
// `int slot`, the lane's place in the chunk's list (index order: waves in order, lanes in order), and `int count`, the length of that list.
// BARRIERS: a chunk has two, the one in here (wave_hits written -> read) and the caller's after the hitting lanes have stored hits[slot] (hits written
// -> walked).  No third one is needed at the end of the walk: the next chunk's wave_hits are written before, its hits after, the barrier in here, which
// every wave reaches only when it is done with this chunk's list, and its wave_hits were last read before the caller's barrier.
// A macro, not a function: an inlined function changes the instruction schedule of all three tiles_kernels; this text compiles to exactly the code it
// did when each kernel spelled it out.
#define compact_hits(hit, wave_hits, lane, wave, slot, count)                   \
    const unsigned long long hit_mask_ = __ballot(hit);                         \
    if ((lane) == 0) (wave_hits)[wave] = __popcll(hit_mask_);                   \
    __syncthreads();                                                            \
    int slot = __popcll(hit_mask_ & ((1ull << (lane)) - 1ull)), count = 0;      \
    for (int k_ = 0; k_ < 4; ++k_) {                                            \
        const int c_ = (wave_hits)[k_];                                         \
        if (k_ < (wave)) slot += c_;                                            \
        count += c_;                                                            \
    }

// ---- host: argument scans; the caller words the message ----------------------------------------------------------------------------------------------
// bounds: [n, 4] = x0, y0, x1, y1 inclusive, x1 < x0 or y1 < y0 = empty.  The first head whose non-empty bounds leave the W x H image, or -1.
inline int first_bad_bound(const int32_t* bounds, int n, int W, int H) {
    for (int i = 0; i < n; ++i) {
        const int32_t* b = bounds + 4 * i;
        const bool empty = b[2] < b[0] || b[3] < b[1];
        if (!empty && !(b[0] >= 0 && b[1] >= 0 && b[2] < W && b[3] < H)) return i;
    }
    return -1;
}
// the first position of `indices` that is not in 0 .. limit - 1, or -1
inline int64_t first_bad_index(const int32_t* indices, int64_t count, int limit) {
    for (int64_t i = 0; i < count; ++i)
        if (indices[i] < 0 || indices[i] >= limit) return i;
    return -1;
}

// ---- host: "tile -> heads in order" for the tiles some head touches ------------------------------------------------------------------------------------
// count, prefix, fill: heads are visited in order, so every tile's list is ascending.  The bounds must have passed first_bad_bound.  per_head (one
// destination per head): every (head, tile) pair is an entry of its own with that one head, heads in order and a head's tiles row by row.
// An entry is xy = tile column | tile row << 16 and the heads heads[first[k]] .. heads[first[k + 1] - 1].
struct TileLists {
    size_t n_tiles = 0, n_pairs = 0;

    void count(const int32_t* bounds_, int n_, int W, int H, bool per_head_ = false) {
        bounds = bounds_, n = n_, per_head = per_head_;
        tiles_x = (W + TILE - 1) / TILE;
        grid.assign((size_t)tiles_x * ((H + TILE - 1) / TILE), 0);
        each_tile([&](int, int tx, int ty) { grid[(size_t)ty * tiles_x + tx]++; });
        n_tiles = n_pairs = 0;
        for (size_t t = 0; t < grid.size(); ++t) {
            n_tiles += grid[t] != 0;
            n_pairs += (size_t)grid[t];
        }
        if (per_head) n_tiles = n_pairs;
    }
    // xy: n_tiles, first: n_tiles + 1, heads: n_pairs entries; n_pairs <= INT32_MAX is the caller's to check
    void fill(uint32_t* xy, int32_t* first, int32_t* heads) {
        size_t k = 0, at = 0;
        if (per_head) {
            each_tile([&](int i, int tx, int ty) {
                xy[k] = (uint32_t)tx | (uint32_t)ty << 16;
                first[k] = (int32_t)k;
                heads[k++] = i;
            });
            first[k] = (int32_t)k;
            return;
        }
        for (size_t t = 0; t < grid.size(); ++t) {  // grid[t] becomes the position of the tile's next head
            const int32_t c = grid[t];
            if (c) {
                xy[k] = (uint32_t)(t % tiles_x) | (uint32_t)(t / tiles_x) << 16;
                first[k++] = (int32_t)at;
            }
            grid[t] = (int32_t)at;
            at += (size_t)c;
        }
        first[k] = (int32_t)at;
        each_tile([&](int i, int tx, int ty) { heads[grid[(size_t)ty * tiles_x + tx]++] = i; });
    }

   private:
    const int32_t* bounds = nullptr;
    int n = 0, tiles_x = 0;
    bool per_head = false;
    std::vector<int32_t> grid;

    template <typename F>
    void each_tile(F f) const {  // f(head, tile column, tile row) for every tile of every non-empty head, heads in order
        for (int i = 0; i < n; ++i) {
            const int32_t* b = bounds + 4 * i;
            if (b[2] < b[0] || b[3] < b[1]) continue;
            for (int ty = b[1] / TILE; ty <= b[3] / TILE; ++ty)
                for (int tx = b[0] / TILE; tx <= b[2] / TILE; ++tx) f(i, tx, ty);
        }
    }
};

// ---- host: per-device state: the staging block of what one call uploads and the boxes, both guarded by the block's event (companion_host.h) ----------
struct State : Staging {
    Scratch<Box> boxes;  // library scratch [n, T]
};

// waits for the blocks' previous user, then makes room for `need` staging bytes and `need_boxes` bytes of boxes; `who` names the caller in the message
inline int reserve(State& s, size_t need, size_t need_boxes, const char* who) {
    if (int rc = companion::reserve(s, need, who)) return rc;
    if (!grow(s.boxes, need_boxes)) {
        set_error("%s: allocating %zu bytes of triangle boxes failed", who, need_boxes);
        return ERR_NOMEM;
    }
    return OK;
}

}  // namespace
}  // namespace tile_fold
