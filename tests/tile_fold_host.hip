// Stand-alone check of the host half of csrc/tile_fold.h: TileLists (shared and per-head), first_bad_bound and first_bad_index against brute force; and of
// what csrc/companion_host.h does without the runtime: align16, the require macro and the message, the queue macro (reserve and finish call the runtime:
// tests/test_gpu_*.py).  tests/test_tile_fold_host.py builds it with the host sanitizers (address, undefined) and runs it on its own.  It makes no HIP call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../head_detector_amd/csrc/tile_fold.h"

using namespace tile_fold;

static int failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            ++failures;                        \
            printf("FAILED %s: ", #cond);      \
            printf(__VA_ARGS__);               \
            printf("\n");                      \
            if (failures > 20) exit(1);        \
        }                                      \
    } while (0)

struct Entry {
    uint32_t xy;
    std::vector<int32_t> heads;
    bool operator==(const Entry& o) const { return xy == o.xy && heads == o.heads; }
};

// does head b touch tile (tx, ty)?  Pixel by pixel would be the same: a tile is touched iff some pixel of the (in-image) bounds lies in it
static bool touches(const int32_t* b, int tx, int ty) {
    if (b[2] < b[0] || b[3] < b[1]) return false;
    return b[0] <= tx * TILE + TILE - 1 && b[2] >= tx * TILE && b[1] <= ty * TILE + TILE - 1 && b[3] >= ty * TILE;
}

static std::vector<Entry> brute(const std::vector<int32_t>& bounds, int W, int H, bool per_head) {
    const int n = (int)bounds.size() / 4, tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
    std::vector<Entry> out;
    if (per_head) {  // heads in order, a head's tiles row by row
        for (int i = 0; i < n; ++i)
            for (int ty = 0; ty < tiles_y; ++ty)
                for (int tx = 0; tx < tiles_x; ++tx)
                    if (touches(&bounds[4 * i], tx, ty)) out.push_back({(uint32_t)tx | (uint32_t)ty << 16, {i}});
        return out;
    }
    for (int ty = 0; ty < tiles_y; ++ty)  // for every tile, which heads touch it, ascending
        for (int tx = 0; tx < tiles_x; ++tx) {
            Entry e{(uint32_t)tx | (uint32_t)ty << 16, {}};
            for (int i = 0; i < n; ++i)
                if (touches(&bounds[4 * i], tx, ty)) e.heads.push_back(i);
            if (!e.heads.empty()) out.push_back(e);
        }
    return out;
}

static void check_lists(const char* what, const std::vector<int32_t>& bounds, int W, int H, bool per_head) {
    const int n = (int)bounds.size() / 4;
    EXPECT(first_bad_bound(bounds.data(), n, W, H) == -1, "%s %d x %d: the case's own bounds", what, W, H);
    const std::vector<Entry> want = brute(bounds, W, H, per_head);
    size_t want_pairs = 0;
    for (const Entry& e : want) want_pairs += e.heads.size();
    TileLists lists;
    lists.count(bounds.data(), n, W, H, per_head);
    EXPECT(lists.n_tiles == want.size() && lists.n_pairs == want_pairs, "%s %d x %d per_head %d: %zu tiles, %zu pairs, brute force %zu, %zu", what, W, H, (int)per_head,
           lists.n_tiles, lists.n_pairs, want.size(), want_pairs);
    if (lists.n_tiles != want.size() || lists.n_pairs != want_pairs) return;
    // exactly the sizes the libraries reserve: the sanitizer sees a write past any of them
    std::vector<uint32_t> xy(lists.n_tiles);
    std::vector<int32_t> first(lists.n_tiles + 1), heads(lists.n_pairs);
    lists.fill(xy.data(), first.data(), heads.data());
    std::vector<Entry> got;
    bool sane = first[0] == 0 && first[lists.n_tiles] == (int32_t)lists.n_pairs;
    for (size_t k = 0; sane && k < lists.n_tiles; ++k) {
        sane = first[k] <= first[k + 1];
        if (sane) got.push_back({xy[k], std::vector<int32_t>(heads.begin() + first[k], heads.begin() + first[k + 1])});
    }
    EXPECT(sane && got == want, "%s %d x %d per_head %d: lists differ from brute force", what, W, H, (int)per_head);
}

// ---- csrc/companion_host.h ----------------------------------------------------------------------------------------------------------------------------
static int needs_small(int v) {
    CH_REQUIRE(v < 10, "needs_small: %d is not below %d (%s)", v, 10, "text");
    return OK;
}

static int evaluated = 0;
static hipError_t step(hipError_t e) {  // a plain value, no runtime call
    ++evaluated;
    return e;
}

static void check_plumbing() {
    const size_t in[] = {0, 1, 15, 16, 17, 31, 32, 4097}, out[] = {0, 16, 16, 16, 32, 32, 32, 4112};
    for (int i = 0; i < 8; ++i) EXPECT(align16(in[i]) == out[i], "align16(%zu) = %zu", in[i], align16(in[i]));
    EXPECT(align16(SIZE_MAX - 15) == SIZE_MAX - 15, "align16 of the last multiple of 16");

    EXPECT(strcmp(last_error(), "") == 0, "a thread starts with no message");
    EXPECT(needs_small(9) == OK && strcmp(last_error(), "") == 0, "a check that holds writes nothing");
    EXPECT(needs_small(12) == ERR_INVALID, "a check that fails returns ERR_INVALID");
    EXPECT(strcmp(last_error(), "needs_small: 12 is not below 10 (text)") == 0, "message '%s'", last_error());
    const std::string big(2000, 'x');  // longer than the buffer: truncated, terminated
    set_error("%s", big.c_str());
    EXPECT(strlen(last_error()) == 511 && last_error()[0] == 'x', "a long message is cut to %zu", strlen(last_error()));

    Queue q;
    EXPECT(q.ok() && q.err == hipSuccess && strcmp(q.failed, "") == 0, "a fresh queue");
    CH_QUEUE(q, step(hipSuccess));
    EXPECT(q.ok() && evaluated == 1, "a success keeps the queue going");
    CH_QUEUE(q, step(hipErrorInvalidValue));
    EXPECT(!q.ok() && q.err == hipErrorInvalidValue && evaluated == 2, "the first failure is kept");
    EXPECT(strcmp(q.failed, "step(hipErrorInvalidValue)") == 0, "its text: '%s'", q.failed);
    CH_QUEUE(q, step(hipErrorOutOfMemory));
    CH_QUEUE(q, step(hipSuccess));
    EXPECT(evaluated == 2, "nothing is evaluated after the first failure (%d evaluations)", evaluated);
    EXPECT(q.err == hipErrorInvalidValue && strcmp(q.failed, "step(hipErrorInvalidValue)") == 0, "and it stays the first: '%s'", q.failed);
    static_assert(OK == 0 && ERR_INVALID == -1 && ERR_HIP == -2 && ERR_NOMEM == -3, "the codes of the public headers");
}

int main() {
    check_plumbing();
    const int sizes[4][2] = {{1, 1}, {16, 16}, {17, 33}, {4000, 3000}};
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        const int xe = (W - 1) / TILE * TILE - 1, ye = (H - 1) / TILE * TILE - 1;  // the last pixel before the last tile column / row, or -1
        std::vector<int32_t> b;
        auto head = [&](int x0, int y0, int x1, int y1) { b.insert(b.end(), {x0, y0, x1, y1}); };
        head(0, 0, W - 1, H - 1);                                 // the full image
        head(5, 5, 4, 9);                                         // empty (x1 < x0), nowhere near the image's limits
        head(W - 1, H - 1, W - 1, H - 1);                         // one pixel, the last
        head(0, 0, 0, 0);                                         // one pixel, the first
        head(0, 0, W < TILE ? W - 1 : TILE - 1, H < TILE ? H - 1 : TILE - 1);  // ends exactly on the first tile's edge
        if (xe >= 0) head(0, 0, xe, H - 1);                       // ends exactly on a later tile edge, in x
        if (ye >= 0) head(0, 0, W - 1, ye);                       // and in y
        if (xe >= 0 && ye >= 0) head(xe, ye, xe + 1, ye + 1);     // straddles a tile corner: four tiles
        head(W / 2, H / 2, W / 2 - 1, H / 2);                     // empty again, so that an empty head is not only the second
        head(W / 3, H / 3, W - 1 - W / 5, H - 1 - H / 7);         // general position
        for (int per_head = 0; per_head < 2; ++per_head) {
            check_lists("all heads", b, W, H, per_head != 0);
            check_lists("no head", {}, W, H, per_head != 0);
            check_lists("only empty heads", {3, 0, 2, 0, 0, 3, 0, 2}, W, H, per_head != 0);
        }
        // first_bad_bound: every way out of the image, after good and empty heads; an empty head may hold anything
        const int n_good = (int)b.size() / 4;
        const int bad[4][4] = {{-1, 0, 0, 0}, {0, -1, 0, 0}, {0, 0, W, 0}, {0, 0, 0, H}};
        for (const auto& q : bad) {
            std::vector<int32_t> c = b;
            c.insert(c.end(), {7, -9, 6, 1 << 30});  // empty: not looked at
            c.insert(c.end(), q, q + 4);
            c.insert(c.end(), {-5, -5, W + 5, H + 5});  // also bad, but later
            EXPECT(first_bad_bound(c.data(), n_good + 3, W, H) == n_good + 1, "first_bad_bound (%d, %d, %d, %d) in %d x %d", q[0], q[1], q[2], q[3], W, H);
            EXPECT(first_bad_bound(c.data(), n_good + 1, W, H) == -1, "first_bad_bound stops at n");
        }
    }
    // first_bad_index: 0 .. limit - 1 is good
    const std::vector<int32_t> idx = {0, 4, 2, 4, 0, 1};
    EXPECT(first_bad_index(idx.data(), 6, 5) == -1, "all inside");
    EXPECT(first_bad_index(idx.data(), 6, 4) == 1, "the first of two too large");
    EXPECT(first_bad_index(idx.data(), 1, 4) == -1, "stops at count");
    EXPECT(first_bad_index(idx.data(), 0, 0) == -1 && first_bad_index(nullptr, 0, 5) == -1, "nothing to look at");
    const std::vector<int32_t> neg = {3, 2, -1, 9};
    EXPECT(first_bad_index(neg.data(), 4, 4) == 2, "negative before too large");
    EXPECT(first_bad_index(neg.data(), 4, 3) == 0, "limit itself is outside");
    if (failures) return 1;
    printf("tile_fold host checks passed\n");
    return 0;
}
