// What the host half and the kernels of csrc/osd.hip (libvghosd.so, include/vgh_osd.h) must not hold twice: the font table, the coverage of an item, the
// blend, the box-growing rules, the tile count, the workspace size and the validation of a job (the checks of a plane and the overlap rule inside it are
// csrc/plane_views.h's host part, shared with libvghvideo.so).
// HIP-free: plain C++ that tests/osd_host.hip compiles for the host alone under the sanitizers; under hipcc the functions are host and device functions.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vgh_osd.h"
#include "plane_views.h"

#if defined(__HIPCC__)
#define OSD_HD __host__ __device__ inline
#else
#define OSD_HD inline
#endif

namespace osd {

constexpr int kTile = 16;  // a workgroup is one 16 x 16 tile of luma positions of one item's grown box (8 x 8 samples of a plane of shift 1)

// ---- the font: 5 x 7, authored here and nowhere else.  One row byte per glyph row, top first; bit 0 is the LEFT column.  ---------------------------------
// Order: space, 0-9, A-Z, # % . : - + /
constexpr uint8_t kFont[VGHO_GLYPHS][VGHO_GLYPH_ROWS] = {
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00},  // space
    {0x0e, 0x11, 0x19, 0x15, 0x13, 0x11, 0x0e},  // 0
    {0x04, 0x06, 0x04, 0x04, 0x04, 0x04, 0x0e},  // 1
    {0x0e, 0x11, 0x10, 0x08, 0x04, 0x02, 0x1f},  // 2
    {0x0f, 0x10, 0x10, 0x0e, 0x10, 0x10, 0x0f},  // 3
    {0x08, 0x0c, 0x0a, 0x09, 0x1f, 0x08, 0x08},  // 4
    {0x1f, 0x01, 0x0f, 0x10, 0x10, 0x11, 0x0e},  // 5
    {0x0c, 0x02, 0x01, 0x0f, 0x11, 0x11, 0x0e},  // 6
    {0x1f, 0x10, 0x08, 0x04, 0x04, 0x02, 0x02},  // 7
    {0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e},  // 8
    {0x0e, 0x11, 0x11, 0x1e, 0x10, 0x08, 0x06},  // 9
    {0x04, 0x0a, 0x11, 0x11, 0x1f, 0x11, 0x11},  // A
    {0x0f, 0x11, 0x11, 0x0f, 0x11, 0x11, 0x0f},  // B
    {0x0e, 0x11, 0x01, 0x01, 0x01, 0x11, 0x0e},  // C
    {0x07, 0x09, 0x11, 0x11, 0x11, 0x09, 0x07},  // D
    {0x1f, 0x01, 0x01, 0x0f, 0x01, 0x01, 0x1f},  // E
    {0x1f, 0x01, 0x01, 0x0f, 0x01, 0x01, 0x01},  // F
    {0x0e, 0x11, 0x01, 0x1d, 0x11, 0x11, 0x1e},  // G
    {0x11, 0x11, 0x11, 0x1f, 0x11, 0x11, 0x11},  // H
    {0x0e, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0e},  // I
    {0x1c, 0x08, 0x08, 0x08, 0x08, 0x09, 0x06},  // J
    {0x11, 0x09, 0x05, 0x03, 0x05, 0x09, 0x11},  // K
    {0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x1f},  // L
    {0x11, 0x1b, 0x15, 0x15, 0x11, 0x11, 0x11},  // M
    {0x11, 0x13, 0x13, 0x15, 0x19, 0x19, 0x11},  // N
    {0x0e, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e},  // O
    {0x0f, 0x11, 0x11, 0x0f, 0x01, 0x01, 0x01},  // P
    {0x0e, 0x11, 0x11, 0x11, 0x15, 0x09, 0x16},  // Q
    {0x0f, 0x11, 0x11, 0x0f, 0x05, 0x09, 0x11},  // R
    {0x1e, 0x01, 0x01, 0x0e, 0x10, 0x10, 0x0f},  // S
    {0x1f, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04},  // T
    {0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e},  // U
    {0x11, 0x11, 0x11, 0x11, 0x0a, 0x0a, 0x04},  // V
    {0x11, 0x11, 0x11, 0x15, 0x15, 0x1b, 0x11},  // W
    {0x11, 0x11, 0x0a, 0x04, 0x0a, 0x11, 0x11},  // X
    {0x11, 0x11, 0x0a, 0x04, 0x04, 0x04, 0x04},  // Y
    {0x1f, 0x10, 0x08, 0x04, 0x02, 0x01, 0x1f},  // Z
    {0x0a, 0x0a, 0x1f, 0x0a, 0x1f, 0x0a, 0x0a},  // #
    {0x13, 0x13, 0x08, 0x04, 0x02, 0x19, 0x19},  // %
    {0x00, 0x00, 0x00, 0x00, 0x00, 0x06, 0x06},  // .
    {0x00, 0x06, 0x06, 0x00, 0x06, 0x06, 0x00},  // :
    {0x00, 0x00, 0x00, 0x1f, 0x00, 0x00, 0x00},  // -
    {0x00, 0x04, 0x04, 0x1f, 0x04, 0x04, 0x00},  // +
    {0x10, 0x10, 0x08, 0x04, 0x02, 0x01, 0x01},  // /
};
constexpr size_t kFontBytes = sizeof(kFont);
static_assert(kFontBytes == 308, "44 glyphs of 7 row bytes");

// the rows of glyph `code`, or NULL for a code outside the table
inline const uint8_t* font_rows(int32_t code) { return code >= 0 && code < VGHO_GLYPHS ? kFont[code] : nullptr; }

// ---- the rule ------------------------------------------------------------------------------------------------------------------------------------------------
struct Box {
    int32_t x0, y0, x1, y1;
};

OSD_HD bool empty(const Box& b) { return b.x1 <= b.x0 || b.y1 <= b.y0; }

OSD_HD Box clipped(const Box& b, int32_t W, int32_t H) {
    return Box{b.x0 < 0 ? 0 : b.x0, b.y0 < 0 ? 0 : b.y0, b.x1 > W ? W : b.x1, b.y1 > H ? H : b.y1};
}

// The box the key clear and the tile enumeration work on: the part of the item's box in the target, grown to even bounds, then clipped to the target again.
// A sample of a plane of shift 1 inside the item's box of that plane reads the keys of positions one row or column OUTSIDE the item's own box where an edge
// is odd; those keys have to be cleared as well.  An item with nothing in the target (a zero side, a box outside) grows to nothing.
OSD_HD Box grown_clipped(const vgho_item& it, int32_t W, int32_t H) {
    const Box t = clipped(Box{it.x0, it.y0, it.x1, it.y1}, W, H);
    if (empty(t)) return Box{0, 0, 0, 0};
    return clipped(Box{t.x0 & ~1, t.y0 & ~1, (t.x1 + 1) & ~1, (t.y1 + 1) & ~1}, W, H);
}

// Does the item cover position (x, y)?  (x, y) must lie in the item's box; `codes` and `font` are the job's codes and the font table.
OSD_HD bool covers(const vgho_item& it, int32_t x, int32_t y, const uint8_t* codes, const uint8_t* font) {
    const int32_t dx = x - it.x0, dy = y - it.y0;
    if (it.kind == VGHO_BAR) return true;
    if (it.kind == VGHO_RECT) {
        const int32_t ex = it.x1 - 1 - x, ey = it.y1 - 1 - y;
        const int32_t mx = dx < ex ? dx : ex, my = dy < ey ? dy : ey;
        return (mx < my ? mx : my) < it.thickness;
    }
    const int32_t u = dx / it.scale, v = dy / it.scale, g = u / VGHO_GLYPH_PITCH, col = u - g * VGHO_GLYPH_PITCH;
    if (col >= VGHO_GLYPH_COLS) return false;
    return (font[(int32_t)codes[it.code_offset + g] * VGHO_GLYPH_ROWS + v] >> col) & 1;
}

// dst of the rule: the owner's colour over the SOURCE sample
OSD_HD uint32_t blend(uint32_t src, uint32_t c, uint32_t a) { return (src * (256u - a) + c * a + 128u) >> 8; }

// ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------------
OSD_HD int32_t plane_side(int32_t side, int32_t shift) { return (side + (1 << shift) - 1) >> shift; }

inline int32_t tiles_across(const Box& g) { return empty(g) ? 0 : (g.x1 - g.x0 + kTile - 1) / kTile; }
inline int32_t tiles_down(const Box& g) { return empty(g) ? 0 : (g.y1 - g.y0 + kTile - 1) / kTile; }

// the (item, tile) pairs of one item: the 16 x 16 tiles of its grown, clipped box, counted from that box's (even) corner
inline int64_t item_tiles(const vgho_item& it, int32_t W, int32_t H) {
    const Box g = grown_clipped(it, W, H);
    return (int64_t)tiles_across(g) * tiles_down(g);
}

inline int64_t tile_count(const vgho_item* items, int32_t n, int32_t W, int32_t H) {
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) total += item_tiles(items[i], W, H);  // <= 65536 * 2048 * 2048 < 2^63
    return total;
}

// the key plane: uint32 [H, W], a multiple of 16 bytes
inline int64_t workspace_bytes(int32_t W, int32_t H) { return ((int64_t)4 * W * H + 15) & ~(int64_t)15; }

// ---- validation ----------------------------------------------------------------------------------------------------------------------------------------------
#define OSD_REFUSE(...) PLANES_REFUSE(__VA_ARGS__)  // the message into msg, and returned

using planes::in_place;
constexpr const char* PLANE_LABELS[VGHO_MAX_PLANES] = {"0", "1", "2"};

// NULL for a job vgho_draw takes, otherwise the message of its first refusal (written to msg).  Reads host memory only; `who` words the message.
inline const char* validate(const vgho_job* job, const char* who, char* msg, size_t msg_bytes) {
    OSD_REFUSE(job, "%s: null job", who);
    const vgho_job& j = *job;
    OSD_REFUSE(j.height >= 1 && j.width >= 1 && j.height <= VGHO_MAX_SIDE && j.width <= VGHO_MAX_SIDE, "%s: target %d x %d outside 1 .. %d", who, j.height, j.width, VGHO_MAX_SIDE);
    OSD_REFUSE(j.n_planes >= 1 && j.n_planes <= VGHO_MAX_PLANES, "%s: n_planes %d outside 1 .. %d", who, j.n_planes, VGHO_MAX_PLANES);
    OSD_REFUSE(j.n_items >= 0 && j.n_items <= VGHO_MAX_ITEMS, "%s: n_items %d outside 0 .. %d", who, j.n_items, VGHO_MAX_ITEMS);
    OSD_REFUSE(j.n_codes >= 0, "%s: n_codes %d is negative", who, j.n_codes);
    OSD_REFUSE(j.reserved == 0, "%s: reserved is %d, not 0", who, j.reserved);
    int64_t pw[VGHO_MAX_PLANES], ph[VGHO_MAX_PLANES];
    for (int k = 0; k < j.n_planes; ++k) {
        const vgho_plane& q = j.planes[k];
        OSD_REFUSE(q.shift == 0 || q.shift == 1, "%s: plane %d: shift %d is not 0 or 1", who, k, q.shift);
        OSD_REFUSE(q.reserved == 0, "%s: plane %d: reserved is %d, not 0", who, k, q.reserved);
        pw[k] = plane_side(j.width, q.shift), ph[k] = plane_side(j.height, q.shift);
        if (const char* m = planes::check_plane(q, pw[k], 3, who, PLANE_LABELS[k], msg, msg_bytes)) return m;
    }
    if (const char* m = planes::check_overlap(j.planes, j.n_planes, pw, ph, who, PLANE_LABELS, msg, msg_bytes)) return m;
    if (j.n_items == 0) return nullptr;
    OSD_REFUSE(j.items, "%s: null items", who);
    for (int32_t i = 0; i < j.n_items; ++i) {
        const vgho_item& it = j.items[i];
        OSD_REFUSE(it.kind >= VGHO_BAR && it.kind <= VGHO_TEXT, "%s: item %d: unknown kind %d", who, i, it.kind);
        const int32_t c[4] = {it.x0, it.y0, it.x1, it.y1};
        for (int k = 0; k < 4; ++k)
            OSD_REFUSE(c[k] >= -VGHO_MAX_COORD && c[k] <= VGHO_MAX_COORD, "%s: item %d: box coordinate %d outside +-%d", who, i, c[k], VGHO_MAX_COORD);
        const int32_t w = it.x1 - it.x0, h = it.y1 - it.y0;
        OSD_REFUSE(w >= 0 && h >= 0 && w <= VGHO_MAX_SIDE && h <= VGHO_MAX_SIDE, "%s: item %d: box sides %d x %d outside 0 .. %d", who, i, w, h, VGHO_MAX_SIDE);
        OSD_REFUSE(it.alpha >= 0 && it.alpha <= VGHO_MAX_ALPHA, "%s: item %d: alpha %d outside 0 .. %d", who, i, it.alpha, VGHO_MAX_ALPHA);
        OSD_REFUSE(it.reserved == 0, "%s: item %d: reserved is %d, not 0", who, i, it.reserved);
        if (it.kind == VGHO_RECT) OSD_REFUSE(it.thickness >= 1, "%s: item %d: thickness %d of a RECT is below 1", who, i, it.thickness);
        if (it.kind != VGHO_TEXT) continue;
        OSD_REFUSE(it.scale >= 1 && it.scale <= VGHO_MAX_SCALE, "%s: item %d: scale %d outside 1 .. %d", who, i, it.scale, VGHO_MAX_SCALE);
        OSD_REFUSE(it.length >= 1 && it.length <= VGHO_MAX_TEXT, "%s: item %d: length %d outside 1 .. %d", who, i, it.length, VGHO_MAX_TEXT);
        OSD_REFUSE(j.codes, "%s: item %d: null codes", who, i);
        OSD_REFUSE(it.code_offset >= 0 && (int64_t)it.code_offset + it.length <= j.n_codes, "%s: item %d: code_offset %d + length %d outside the %d codes", who, i, it.code_offset,
                   it.length, j.n_codes);
        for (int32_t k = 0; k < it.length; ++k)
            OSD_REFUSE(font_rows(j.codes[it.code_offset + k]), "%s: item %d: code %d (at %d) outside the font of %d glyphs", who, i, j.codes[it.code_offset + k], it.code_offset + k, VGHO_GLYPHS);
        const int32_t tw = VGHO_GLYPH_PITCH * it.scale * it.length - it.scale, th = VGHO_GLYPH_ROWS * it.scale;
        OSD_REFUSE(w == tw && h == th, "%s: item %d: box %d x %d of a TEXT is not its run's size %d x %d (length %d, scale %d)", who, i, w, h, tw, th, it.length, it.scale);
    }
    const int64_t tiles = tile_count(j.items, j.n_items, j.width, j.height);
    OSD_REFUSE(tiles <= VGHO_MAX_TILES, "%s: %lld tiles exceed one launch (%d)", who, (long long)tiles, VGHO_MAX_TILES);
    return nullptr;
}

}  // namespace osd
