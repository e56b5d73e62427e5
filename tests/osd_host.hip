// csrc/osd_rules.h (the font, the coverage of an item, the blend, the grown box, the tile count, the workspace size and the validation of a job) under the host
// sanitizers.  A program of its own: built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU.  It
// includes the rule header alone and makes no HIP call: every job here is only validated, and every pointer of a plane is only compared.
#include <stdlib.h>
#include <string.h>

#include "../head_detector_amd/csrc/osd_rules.h"

using namespace osd;

static int failures = 0;
static char msg[400];

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s (message: %s)\n", __LINE__, #cond, msg); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static bool refused(const vgho_job& j, const char* words) {
    msg[0] = 0;
    const char* m = validate(&j, "draw", msg, sizeof(msg));
    return m == msg && strstr(msg, words);
}

static bool accepted(const vgho_job& j) {
    msg[0] = 0;
    return validate(&j, "draw", msg, sizeof(msg)) == nullptr;
}

static vgho_item bar(int x0, int y0, int x1, int y1) {
    vgho_item it = {};
    it.kind = VGHO_BAR, it.x0 = x0, it.y0 = y0, it.x1 = x1, it.y1 = y1, it.alpha = 256;
    return it;
}

static int count(const vgho_item& it, const uint8_t* codes) {  // covered positions of the whole box
    int n = 0;
    for (int y = it.y0; y < it.y1; ++y)
        for (int x = it.x0; x < it.x1; ++x) n += covers(it, x, y, codes, &kFont[0][0]);
    return n;
}

int main() {
    // ---- the font: every glyph fits 5 x 7, the lookup refuses what lies outside ----
    EXPECT(sizeof(vgho_item) == 44 && sizeof(vgho_plane) == 48 && sizeof(vgho_job) == 184);
    for (int c = 0; c < VGHO_GLYPHS; ++c)
        for (int r = 0; r < VGHO_GLYPH_ROWS; ++r) EXPECT(font_rows(c) && font_rows(c)[r] < (1 << VGHO_GLYPH_COLS));
    EXPECT(!font_rows(-1) && !font_rows(VGHO_GLYPHS) && !font_rows(255) && !font_rows(INT32_MAX) && !font_rows(INT32_MIN));
    EXPECT(font_rows(0)[3] == 0 && font_rows(2)[0] == 0x04 && font_rows(2)[1] == 0x06 && font_rows(2)[6] == 0x0e);  // space; "1": ..#.. / .##.. / ... / .###.

    // ---- the blend ----
    EXPECT(blend(10, 200, 128) == 105 && blend(10, 200, 256) == 200 && blend(10, 200, 0) == 10 && blend(255, 255, 255) == 255 && blend(0, 0, 1) == 0);
    for (uint32_t s = 0; s < 256; ++s)
        for (uint32_t a = 0; a <= 256; a += 64) EXPECT(blend(s, s, a) == s && blend(s, 255 - s, 256) == 255 - s && blend(s, 7, 0) == s);

    // ---- coverage at the edges of a box ----
    const uint8_t codes[4] = {2, 0, 43, 11};  // "1", space, "/", "A"
    vgho_item r = bar(10, 20, 15, 24);
    r.kind = VGHO_RECT, r.thickness = 1;
    EXPECT(count(r, codes) == 5 * 4 - 3 * 2);  // a 5 x 4 box: the ring
    EXPECT(covers(r, 10, 20, codes, &kFont[0][0]) && covers(r, 14, 23, codes, &kFont[0][0]) && !covers(r, 11, 21, codes, &kFont[0][0]) && !covers(r, 13, 22, codes, &kFont[0][0]));
    r.thickness = 2;
    EXPECT(count(r, codes) == 20);  // half the shorter side: the box is full
    r.thickness = 1 << 30;
    EXPECT(count(r, codes) == 20);
    vgho_item far = bar(-VGHO_MAX_COORD, VGHO_MAX_COORD - 3, -VGHO_MAX_COORD + 3, VGHO_MAX_COORD);
    far.kind = VGHO_RECT, far.thickness = 1;
    EXPECT(count(far, codes) == 8);  // nothing overflows at the largest coordinates
    vgho_item t = bar(-3, 5, -3 + 6 * 2 * 3 - 2, 5 + 14);
    t.kind = VGHO_TEXT, t.scale = 2, t.length = 3, t.code_offset = 0;
    int ones = 0;
    for (int k = 0; k < 7; ++k) ones += __builtin_popcount(kFont[2][k]) + __builtin_popcount(kFont[43][k]);
    EXPECT(count(t, codes) == 4 * ones);  // "1 /" at scale 2: every set bit is a 2 x 2 block, the sixth column and the space are blank
    EXPECT(covers(t, -3 + 2 * 2, 5, codes, &kFont[0][0]) && covers(t, -3 + 2 * 2 + 1, 5 + 1, codes, &kFont[0][0]) && !covers(t, -3, 5, codes, &kFont[0][0]));  // the top of "1" is column 2
    EXPECT(!covers(t, -3 + 5 * 2, 5 + 13, codes, &kFont[0][0]) && covers(t, t.x1 - 1 - 5 * 2 + 1, t.y1 - 1, codes, &kFont[0][0]));  // the gap column; the foot of "/" is its column 0
    t.code_offset = 1, t.length = 3, t.scale = 16, t.x1 = t.x0 + 6 * 16 * 3 - 16, t.y1 = t.y0 + 7 * 16;
    EXPECT(count(t, codes) > 0);  // reads codes[1 .. 3] and no further: the sanitizer watches the array's end

    // ---- the grown box, the tile counts, the workspace ----
    Box g = grown_clipped(bar(3, 5, 8, 9), 100, 100);
    EXPECT(g.x0 == 2 && g.y0 == 4 && g.x1 == 8 && g.y1 == 10);
    g = grown_clipped(bar(4, 6, 9, 11), 100, 100);
    EXPECT(g.x0 == 4 && g.y0 == 6 && g.x1 == 10 && g.y1 == 12);
    g = grown_clipped(bar(-5, -3, 99, 97), 97, 95);  // negative odd corners grow downwards, then everything is clipped
    EXPECT(g.x0 == 0 && g.y0 == 0 && g.x1 == 97 && g.y1 == 95);
    EXPECT((-5 & ~1) == -6 && (-3 & ~1) == -4);
    EXPECT(empty(grown_clipped(bar(7, 7, 7, 20), 100, 100)) && empty(grown_clipped(bar(7, 7, 20, 7), 100, 100)) && empty(grown_clipped(bar(100, 0, 120, 50), 100, 100)));
    EXPECT(empty(grown_clipped(bar(-20, -20, -1, -1), 100, 100)) && !empty(grown_clipped(bar(-20, -20, 1, 1), 100, 100)));
    EXPECT(item_tiles(bar(0, 0, 16, 16), 100, 100) == 1 && item_tiles(bar(0, 0, 17, 16), 100, 100) == 2 && item_tiles(bar(1, 1, 17, 17), 100, 100) == 4);  // (0, 0, 18, 18)
    EXPECT(item_tiles(bar(15, 15, 16, 16), 100, 100) == 1 && item_tiles(bar(15, 15, 16, 16), 15, 100) == 0 && item_tiles(bar(0, 0, 0, 0), 100, 100) == 0);
    EXPECT(item_tiles(bar(-VGHO_MAX_COORD, -VGHO_MAX_COORD, -VGHO_MAX_COORD + VGHO_MAX_SIDE, -VGHO_MAX_COORD + VGHO_MAX_SIDE), VGHO_MAX_SIDE, VGHO_MAX_SIDE) == 0);
    EXPECT(item_tiles(bar(0, 0, VGHO_MAX_SIDE, VGHO_MAX_SIDE), VGHO_MAX_SIDE, VGHO_MAX_SIDE) == 2048 * 2048);
    EXPECT(workspace_bytes(1, 1) == 16 && workspace_bytes(131, 97) == ((4 * 131 * 97 + 15) / 16) * 16 && workspace_bytes(VGHO_MAX_SIDE, VGHO_MAX_SIDE) == (4ll * 32767 * 32767 + 15) / 16 * 16);
    EXPECT(plane_side(97, 0) == 97 && plane_side(97, 1) == 49 && plane_side(96, 1) == 48 && plane_side(1, 1) == 1);

    // ---- validate() ----
    uint8_t* mem = (uint8_t*)malloc(1 << 16);  // only its addresses are used
    vgho_item items[3] = {bar(1, 1, 30, 20), r, bar(0, 0, 6 * 2 * 2 - 2, 14)};
    items[2].kind = VGHO_TEXT, items[2].scale = 2, items[2].length = 2, items[2].code_offset = 2;
    vgho_job ok = {};
    ok.height = 20, ok.width = 30, ok.n_planes = 3, ok.n_items = 3, ok.items = items, ok.codes = codes, ok.n_codes = 4;
    for (int k = 0; k < 3; ++k) {
        vgho_plane& q = ok.planes[k];
        q.src_dev = q.dst_dev = mem + (k ? 1024 + (k - 1) : 0), q.src_pitch = q.dst_pitch = k ? 32 : 32, q.src_step = q.dst_step = k ? 2 : 1, q.shift = k ? 1 : 0;
    }
    EXPECT(accepted(ok));
    msg[0] = 0;
    EXPECT(validate(nullptr, "draw", msg, sizeof(msg)) == msg && strstr(msg, "null job"));
    vgho_job j = ok;
    j.height = 0;
    EXPECT(refused(j, "target 0 x 30"));
    j = ok, j.width = VGHO_MAX_SIDE + 1;
    EXPECT(refused(j, "target 20 x 32768"));
    j = ok, j.n_planes = 0;
    EXPECT(refused(j, "n_planes 0"));
    j = ok, j.n_planes = 4;
    EXPECT(refused(j, "n_planes 4"));
    j = ok, j.n_items = VGHO_MAX_ITEMS + 1;
    EXPECT(refused(j, "n_items 65537"));
    j = ok, j.n_items = -1;
    EXPECT(refused(j, "n_items -1"));
    j = ok, j.items = nullptr;
    EXPECT(refused(j, "null items"));
    j.n_items = 0;
    EXPECT(accepted(j));  // nothing to draw needs no items
    j = ok, j.codes = nullptr;
    EXPECT(refused(j, "item 2: null codes"));
    j = ok, j.n_codes = 3;
    EXPECT(refused(j, "item 2: code_offset 2 + length 2 outside the 3 codes"));
    j = ok, j.reserved = 1;
    EXPECT(refused(j, "reserved"));
    j = ok, j.planes[1].shift = 2;
    EXPECT(refused(j, "plane 1: shift 2"));
    j = ok, j.planes[2].src_step = 4;
    EXPECT(refused(j, "plane 2: steps 4 and 2"));
    j = ok, j.planes[0].dst_step = 0;
    EXPECT(refused(j, "plane 0: steps 1 and 0"));
    j = ok, j.planes[0].src_pitch = 29;
    EXPECT(refused(j, "plane 0: src_pitch 29 outside 30"));
    j = ok, j.planes[1].dst_pitch = 28;
    EXPECT(refused(j, "plane 1: dst_pitch 28 outside 29"));
    j = ok, j.planes[2].src_dev = nullptr;
    EXPECT(refused(j, "plane 2: null plane"));
    j = ok, j.planes[0].dst_pitch = 40;
    EXPECT(refused(j, "plane 0: the destination starts where the source does"));
    j = ok, j.planes[0].dst_dev = mem + 8;
    EXPECT(refused(j, "plane 0: the destination overlaps source plane 0"));
    j = ok, j.planes[2].dst_dev = mem + 1024 - (32 * 9 + 2 * 14);  // 10 rows of 15 samples: its last sample is the first of source plane 1
    EXPECT(refused(j, "plane 2: the destination overlaps source plane 1"));
    j.planes[2].dst_dev = mem + 1024 - (32 * 9 + 2 * 14) - 1;
    EXPECT(accepted(j));  // ... and one byte lower it touches nothing (source plane 0 ends at byte 638)
    j = ok, j.planes[1].dst_dev = mem + 4096, j.planes[2].dst_dev = mem + 8192, j.planes[1].dst_step = j.planes[2].dst_step = 1, j.planes[1].dst_pitch = j.planes[2].dst_pitch = 15;
    EXPECT(accepted(j));  // interleaved in, planar out
    vgho_item bad[3];
    auto with = [&](int k, auto change) {
        memcpy(bad, items, sizeof(bad));
        change(bad[k]);
        vgho_job b = ok;
        b.items = bad;
        return b;
    };
    EXPECT(refused(with(0, [](vgho_item& i) { i.kind = 3; }), "item 0: unknown kind 3"));
    EXPECT(refused(with(1, [](vgho_item& i) { i.thickness = 0; }), "item 1: thickness 0"));
    EXPECT(refused(with(0, [](vgho_item& i) { i.alpha = 257; }), "item 0: alpha 257"));
    EXPECT(refused(with(1, [](vgho_item& i) { i.alpha = -1; }), "item 1: alpha -1"));
    EXPECT(refused(with(0, [](vgho_item& i) { i.x1 = i.x0 - 1; }), "item 0: box sides -1 x 19"));
    EXPECT(refused(with(0, [](vgho_item& i) { i.y1 = i.y0 + VGHO_MAX_SIDE + 1; }), "item 0: box sides 29 x 32768"));
    EXPECT(refused(with(0, [](vgho_item& i) { i.x0 = -VGHO_MAX_COORD - 1; }), "item 0: box coordinate -16777216"));
    EXPECT(refused(with(0, [](vgho_item& i) { i.x0 = INT32_MIN, i.x1 = INT32_MAX; }), "item 0: box coordinate"));  // (x1 - x0 is never formed)
    EXPECT(refused(with(0, [](vgho_item& i) { i.reserved = 1; }), "item 0: reserved"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.scale = 0; }), "item 2: scale 0"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.scale = 17; }), "item 2: scale 17"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.length = 0; }), "item 2: length 0"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.length = 65; }), "item 2: length 65"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.code_offset = -1; }), "item 2: code_offset -1"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.code_offset = INT32_MAX; }), "item 2: code_offset 2147483647"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.x1 += 1; }), "item 2: box 23 x 14 of a TEXT is not its run's size 22 x 14"));
    EXPECT(refused(with(2, [](vgho_item& i) { i.y1 -= 1; }), "item 2: box 22 x 13 of a TEXT"));
    EXPECT(accepted(with(2, [](vgho_item& i) { i.x0 -= 1000, i.x1 -= 1000; })));  // anywhere, as long as it has its size
    const uint8_t wrong[4] = {2, 0, 44, 11};
    j = ok, j.codes = wrong;
    EXPECT(refused(j, "item 2: code 44 (at 2) outside the font of 44 glyphs"));
    // the tile cap: 65536 items of 17 x 17 tiles each
    vgho_item* many = (vgho_item*)malloc(sizeof(vgho_item) * VGHO_MAX_ITEMS);
    for (int k = 0; k < VGHO_MAX_ITEMS; ++k) many[k] = bar(0, 0, 272, 272);
    j = ok, j.items = many, j.n_items = VGHO_MAX_ITEMS, j.height = j.width = 272;
    for (int k = 0; k < 3; ++k) j.planes[k].src_pitch = j.planes[k].dst_pitch = 272;
    j.planes[1].src_dev = j.planes[1].dst_dev = mem + 2;  // (only compared: in place)
    EXPECT(tile_count(many, VGHO_MAX_ITEMS, 272, 272) == 65536ll * 289 && refused(j, "tiles exceed one launch"));
    j.n_items = 58052;  // 58052 * 289 = 16 777 028 <= 2^24 < 58053 * 289
    EXPECT(accepted(j));
    j.n_items = 58053;
    EXPECT(refused(j, "16777317 tiles"));
    free(many);
    free(mem);
    if (failures) {
        printf("%d osd host checks FAILED\n", failures);
        return 1;
    }
    printf("osd host checks passed\n");
    return 0;
}
