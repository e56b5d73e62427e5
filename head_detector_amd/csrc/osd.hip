// libvghosd.so (include/vgh_osd.h): overlay.render -- bars, boxes and bitmap text written into the planes a frame already lies in (the Y, U and V planes of a
// YUV 4:2:0 frame, or the three byte planes of an RGB image), in place if wanted, without an RGB copy of a frame and without a launch per item.
//
// KEY: the key plane K, u32 [H, W] in the caller's workspace, holds 1 + the latest item that covers a position.  The workspace arrives holding anything, and no
// pass walks it whole: clear_kernel zeroes the keys of every item's box GROWN TO EVEN BOUNDS (a sample of a plane of shift 1 reads the keys of a row or column
// outside an odd edge), paint_kernel raises the keys of the covered positions (atomicMax of i + 1), and write_kernel, one lane per plane sample of every item's
// grown box, takes the maximum of the sample's 1 or 4 keys and blends the item's colour over the SOURCE sample if that maximum is its own item: each sample is
// written by exactly one lane of exactly one item.  A plane that is out of place is copied first.
// The (item, 16 x 16 tile) pairs are listed on the host and uploaded with the items, the codes and the font in ONE staging block; a workgroup is one tile of
// one item, so the item's row is wave-uniform and no lane branches on its kind apart from its wave.  Integer arithmetic only.  The font, the coverage, the
// blend, the grown box, the tile count, the workspace size and every check of a job are csrc/osd_rules.h's and exist nowhere else; a plane's checks, the pair
// test, the pair access and the strided copy kernel are csrc/plane_views.h's, shared with libvghvideo.so (header-only: nothing is linked).
// Self-contained on purpose: no csrc/vgh_internal.h, no object of libvgh.so or of another companion, no other public header (csrc/companion_host.h is the host
// plumbing the companion libraries' sources share); built with -fvisibility=hidden, only the vgho_* functions are exported.
#include <string.h>

#include <map>
#include <mutex>

#include "../../include/vgh_osd.h"
#include "companion_host.h"
#include "osd_rules.h"
#include "plane_views.h"

namespace {

using namespace companion;
using namespace osd;
static_assert(VGHO_OK == OK && VGHO_ERR_INVALID == ERR_INVALID && VGHO_ERR_HIP == ERR_HIP && VGHO_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");
static_assert(sizeof(vgho_item) == 44 && sizeof(vgho_plane) == 48 && sizeof(vgho_job) == 184, "the layout the binding mirrors");

// one 16 x 16 tile of one item's grown, clipped box: what blockIdx.x maps to
struct Tile {
    int32_t item;
    uint32_t xy;  // tile column | tile row << 16, counted from the grown box's corner
};

// One plane as the write pass sees it (csrc/plane_views.h), and the planes of one shift: they share their geometry.
struct Member : planes::Chan {
    int32_t plane;  // its index in the job: which colour byte of an item it takes
};
struct Group {
    Member c[VGHO_MAX_PLANES];
    int32_t n;
    int32_t spair, dpair;  // n = 2: 0 = two planes; 1 / 2 = c[0] / c[1] is the even, lower byte of interleaved pairs that one 16-bit access reaches
};

// what the three passes share: the tile's item (a wave-uniform row: scalar loads), its grown box and the tile's corner
struct Where {
    int32_t i;
    Box g;
    int32_t ox, oy;
};

__device__ __forceinline__ Where locate(const vgho_item* __restrict__ items, const Tile* __restrict__ tiles, int W, int H, vgho_item& it) {
    const Tile t = tiles[blockIdx.x];
    it = items[t.item];
    Where w;
    w.i = t.item;
    w.g = grown_clipped(it, W, H);
    w.ox = w.g.x0 + (int32_t)(t.xy & 0xffff) * kTile;
    w.oy = w.g.y0 + (int32_t)(t.xy >> 16) * kTile;
    return w;
}

// ---- clear: the keys of the item's GROWN box --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clear_kernel(const vgho_item* __restrict__ items, const Tile* __restrict__ tiles, uint32_t* __restrict__ key, int W, int H) {
    vgho_item it;
    const Where w = locate(items, tiles, W, H, it);
    const int x = w.ox + (int)(threadIdx.x & (kTile - 1)), y = w.oy + (int)(threadIdx.x >> 4);
    if (x < w.g.x1 && y < w.g.y1) key[(size_t)y * W + x] = 0u;
}

// ---- paint: the covered positions of the item's TRUE box, in the target ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paint_kernel(const vgho_item* __restrict__ items, const Tile* __restrict__ tiles, const uint8_t* __restrict__ codes,
                                                    const uint8_t* __restrict__ font, uint32_t* __restrict__ key, int W, int H) {
    vgho_item it;
    const Where w = locate(items, tiles, W, H, it);
    const int x = w.ox + (int)(threadIdx.x & (kTile - 1)), y = w.oy + (int)(threadIdx.x >> 4);
    const Box t = clipped(Box{it.x0, it.y0, it.x1, it.y1}, W, H);
    if (x < t.x0 || x >= t.x1 || y < t.y0 || y >= t.y1) return;
    if (covers(it, x, y, codes, font)) atomicMax(&key[(size_t)y * W + x], (uint32_t)w.i + 1u);
}

// ---- write: one lane per sample of the planes of shift S ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void blend_sample(const Group& G, const vgho_item& it, int x, int y) {
    uint32_t v[VGHO_MAX_PLANES];
    planes::load(G.c, G.n, x, y, G.spair, v);  // (a pair is set for n = 2 alone)
    const uint32_t colour = (uint32_t)it.color[0] | (uint32_t)it.color[1] << 8 | (uint32_t)it.color[2] << 16;
    for (int c = 0; c < G.n; ++c) v[c] = blend(v[c], (colour >> (8 * G.c[c].plane)) & 255u, (uint32_t)it.alpha);
    planes::store(G.c, G.n, x, y, G.dpair, v);
}

// S = 0: 256 lanes, the tile's 16 x 16 positions.  S = 1: 64 lanes, its 8 x 8 samples (the tile's corner is even); a sample's keys are the positions
// {2 y, 2 y + 1} x {2 x, 2 x + 1} that lie in the target -- all of them inside the grown box, so all of them cleared.
template <int S>
__global__ __launch_bounds__(256) void write_kernel(const vgho_item* __restrict__ items, const Tile* __restrict__ tiles, const uint32_t* __restrict__ key, int W, int H, const Group G) {
    vgho_item it;
    const Where w = locate(items, tiles, W, H, it);
    constexpr int side = kTile >> S;
    const int x = (w.ox >> S) + (int)(threadIdx.x & (side - 1)), y = (w.oy >> S) + (int)(threadIdx.x / side);
    if ((x << S) >= w.g.x1 || (y << S) >= w.g.y1) return;
    uint32_t k = 0u;
#pragma unroll
    for (int dy = 0; dy < (1 << S); ++dy)
#pragma unroll
        for (int dx = 0; dx < (1 << S); ++dx) {
            const int lx = (x << S) + dx, ly = (y << S) + dy;
            if (lx < W && ly < H) k = max(k, key[(size_t)ly * W + lx]);
        }
    if (k == (uint32_t)w.i + 1u) blend_sample(G, it, x, y);
}

// The planes idx[0 .. n) (one shift, all out of place) as ONE dense copy: n >= 2 planes, n bytes between samples on both sides, their pointers the n
// consecutive bytes of a sample in the same order on both sides, one pitch a side that holds a whole row.  `lo`: the plane at the lowest address.
bool interleaved_whole(const vgho_job& j, const int* idx, int n, int64_t pw, int& lo) {
    if (n < 2) return false;
    lo = idx[0];
    for (int k = 1; k < n; ++k)
        if (j.planes[idx[k]].src_dev < j.planes[lo].src_dev) lo = idx[k];
    const vgho_plane& base = j.planes[lo];
    if (base.src_pitch < pw * n || base.dst_pitch < pw * n) return false;
    unsigned seen = 0;
    for (int k = 0; k < n; ++k) {
        const vgho_plane& q = j.planes[idx[k]];
        const ptrdiff_t ds = q.src_dev - base.src_dev, dd = q.dst_dev - base.dst_dev;
        if (q.src_step != n || q.dst_step != n || q.src_pitch != base.src_pitch || q.dst_pitch != base.dst_pitch || ds != dd || ds < 0 || ds >= n) return false;
        seen |= 1u << ds;
    }
    return seen == (1u << n) - 1u;
}

std::mutex g_mutex;
std::map<int, Staging> g_staging;  // per device: the items, the codes, the font and the tile list of one call

}  // namespace

extern "C" VGHO_API const char* vgho_version(void) { return "vghosd 1 (gfx950)"; }
extern "C" VGHO_API const char* vgho_last_error(void) { return last_error(); }

extern "C" VGHO_API int64_t vgho_workspace_bytes(const vgho_job* job) {
    char why[400];
    if (validate(job, "workspace_bytes", why, sizeof(why))) {
        set_error("%s", why);
        return 0;
    }
    return workspace_bytes(job->width, job->height);
}

extern "C" VGHO_API int vgho_font(int32_t code, uint8_t rows_out[7]) {
    CH_REQUIRE(rows_out, "font: null rows_out");
    const uint8_t* rows = font_rows(code);
    CH_REQUIRE(rows, "font: code %d outside the font of %d glyphs", code, VGHO_GLYPHS);
    memcpy(rows_out, rows, VGHO_GLYPH_ROWS);
    return OK;
}

extern "C" VGHO_API int vgho_draw(const vgho_job* job, void* workspace_dev, void* stream) {
    char why[400];
    const char* refusal = validate(job, "draw", why, sizeof(why));  // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(!refusal, "%s", why);
    CH_REQUIRE(workspace_dev, "draw: null workspace");
    CH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "draw: workspace is not 16-byte aligned");
    const vgho_job& j = *job;
    const int n = j.n_items, W = j.width, H = j.height;
    const int64_t n_tiles = n ? tile_count(j.items, n, W, H) : 0;
    bool any_copy = false;
    for (int k = 0; k < j.n_planes; ++k) any_copy |= !in_place(j.planes[k]);
    if (!n_tiles && !any_copy) return OK;  // nothing to draw, nothing to copy: nothing is queued

    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    // one upload: [items | codes | font | tiles], each from a 16-byte boundary
    const size_t at_codes = align16((size_t)n * sizeof(vgho_item)), at_font = align16(at_codes + (size_t)j.n_codes), at_tiles = align16(at_font + kFontBytes);
    const size_t total = at_tiles + (size_t)n_tiles * sizeof(Tile);
    if (n_tiles) {
        if (int rc = reserve(s, total, "draw")) return rc;  // also waits for this device's previous call
        memcpy(s.host, j.items, (size_t)n * sizeof(vgho_item));
        if (j.n_codes && j.codes) memcpy(s.host + at_codes, j.codes, (size_t)j.n_codes);
        memcpy(s.host + at_font, kFont, kFontBytes);
        Tile* ht = (Tile*)(s.host + at_tiles);
        for (int i = 0; i < n; ++i) {
            const Box g = grown_clipped(j.items[i], W, H);
            const int across = tiles_across(g), down = tiles_down(g);
            for (int ty = 0; ty < down; ++ty)
                for (int tx = 0; tx < across; ++tx) *ht++ = Tile{i, (uint32_t)tx | (uint32_t)ty << 16};
        }
    }
    // the planes of each shift, in the job's order
    Group groups[2] = {};
    int members[2][VGHO_MAX_PLANES];
    for (int k = 0; k < j.n_planes; ++k) {
        const vgho_plane& q = j.planes[k];
        Group& G = groups[q.shift];
        members[q.shift][G.n] = k;
        G.c[G.n++] = Member{planes::chan_of(q), k};
    }
    for (Group& G : groups)
        if (G.n == 2) {
            G.spair = planes::pair_of(G.c[0].src, G.c[1].src, G.c[0].spitch, G.c[1].spitch, G.c[0].sstep, G.c[1].sstep);
            G.dpair = planes::pair_of(G.c[0].dst, G.c[1].dst, G.c[0].dpitch, G.c[1].dpitch, G.c[0].dstep, G.c[1].dstep);
        }
    // from here on work is queued (companion_host.h, queue-then-record)
    Queue q;
    if (n_tiles) CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));
    for (int shift = 0; shift < 2; ++shift) {  // the planes that are out of place: every sample copied
        const Group& G = groups[shift];
        const int64_t pw = plane_side(W, shift), ph = plane_side(H, shift);
        bool all_out = G.n > 0;
        for (int c = 0; c < G.n; ++c) all_out &= !in_place(j.planes[members[shift][c]]);
        int lo = 0;
        if (all_out && interleaved_whole(j, members[shift], G.n, pw, lo)) {
            const vgho_plane& p = j.planes[lo];
            CH_QUEUE(q, hipMemcpy2DAsync(p.dst_dev, (size_t)p.dst_pitch, p.src_dev, (size_t)p.src_pitch, (size_t)(pw * G.n), (size_t)ph, hipMemcpyDeviceToDevice, st));
            continue;
        }
        for (int c = 0; c < G.n; ++c) {
            const vgho_plane& p = j.planes[members[shift][c]];
            if (in_place(p)) continue;
            if (p.src_step == 1 && p.dst_step == 1)
                CH_QUEUE(q, hipMemcpy2DAsync(p.dst_dev, (size_t)p.dst_pitch, p.src_dev, (size_t)p.src_pitch, (size_t)pw, (size_t)ph, hipMemcpyDeviceToDevice, st));
            else if (q.ok())
                hipLaunchKernelGGL(planes::copy_kernel,dim3((unsigned)((pw + 1023) / 1024), (unsigned)ph), dim3(256), 0, st, p.src_dev, p.src_pitch, p.src_step, p.dst_dev, p.dst_pitch, p.dst_step, (int)pw);
        }
    }
    if (n_tiles && q.ok()) {
        const vgho_item* items = (const vgho_item*)s.dev;
        const Tile* tiles = (const Tile*)(s.dev + at_tiles);
        uint32_t* key = (uint32_t*)workspace_dev;
        const dim3 grid((unsigned)n_tiles);
        hipLaunchKernelGGL(clear_kernel, grid, dim3(256), 0, st, items, tiles, key, W, H);
        hipLaunchKernelGGL(paint_kernel, grid, dim3(256), 0, st, items, tiles, (const uint8_t*)(s.dev + at_codes), (const uint8_t*)(s.dev + at_font), key, W, H);
        if (groups[0].n) hipLaunchKernelGGL(write_kernel<0>, grid, dim3(256), 0, st, items, tiles, (const uint32_t*)key, W, H, groups[0]);
        if (groups[1].n) hipLaunchKernelGGL(write_kernel<1>, grid, dim3(64), 0, st, items, tiles, (const uint32_t*)key, W, H, groups[1]);
    }
    return finish(q, s, n_tiles != 0, st, "draw");
}
