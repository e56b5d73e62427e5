// The host half of csrc/anonymize.hip (every argument check, the per-head offsets, the workspace size) under the host sanitizers.  A program of its own:
// built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU.  It makes no call that reaches a device:
// every job here is either refused before anything is queued or only sized.
#include <stdlib.h>

#include "../head_detector_amd/csrc/anonymize.hip"

static int failures = 0;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            printf("line %d: %s (message: %s)\n", __LINE__, #cond, vghan_last_error()); \
            ++failures;                                                                \
        }                                                                              \
    } while (0)

static bool refused(const vghan_job& j, void* ws, const char* words) {
    const int rc = vghan_anonymize(&j, ws, nullptr);
    return rc == VGHAN_ERR_INVALID && strstr(vghan_last_error(), words);
}

int main() {
    alignas(16) static uint8_t memory[1 << 16];  // stands for device memory: never touched
    uint8_t* src = memory;
    uint8_t* dst = memory + 32768;
    void* ws = memory + 16;
    // exactly as many rows and taps as the job names: a read past either is a sanitizer report
    vghan_head* heads = (vghan_head*)malloc(3 * sizeof(vghan_head));
    int32_t* taps = (int32_t*)malloc(4 * sizeof(int32_t));
    heads[0] = {10, 10, 60, 50, 7, 1, 0, 0};
    heads[1] = {-20, -5, 30, 40, 8, 0, 2, 0};
    heads[2] = {90, 80, 90, 95, 1, 1, 0, 0};  // a zero side
    taps[0] = 65534, taps[1] = 1, taps[2] = 65536, taps[3] = 0;
    vghan_job good = {};
    good.src_dev = src, good.dst_dev = dst, good.src_pitch_bytes = 100 * 3, good.height = 97, good.width = 100, good.n_heads = 3, good.method = VGHAN_METHOD_BLUR;
    good.region = VGHAN_REGION_ELLIPSE, good.heads = heads, good.taps = taps, good.n_taps = 4;

    // sizes: the owner plane, one u32 per pixel of the clipped boxes, the u16 h rows extended by r
    const int64_t owner = 4 * 97 * 100, values = 4 * (50 * 40 + 30 * 40), h = 2 * 3 * ((40 + 2) * 50 + 40 * 30);
    EXPECT(vghan_workspace_bytes(&good) == up16(up16(owner + values) + h));
    vghan_job j = good;
    j.method = VGHAN_METHOD_FILL;
    EXPECT(vghan_workspace_bytes(&j) == up16(owner));
    j.method = VGHAN_METHOD_PIXELATE;  // 8 x 6 and 7 x 6 cells
    EXPECT(vghan_workspace_bytes(&j) == up16(owner + 4 * (48 + 42)));
    j.region = VGHAN_REGION_MAP, j.owner_dev = (const int32_t*)(memory + 64);
    EXPECT(vghan_workspace_bytes(&j) == up16(4 * (48 + 42)));
    j.n_heads = 0, j.heads = nullptr;
    EXPECT(vghan_workspace_bytes(&j) == 16);
    {
        Plan p;
        EXPECT(make_plan(&good, p, "t") == OK && p.rows.size() == 3 && p.tiles[3] == 1 * 10 + 1 * 10 && p.segments[3] == 42 + 40 && p.rows[1].cx0 == 0 && p.rows[1].cy0 == 0 && p.rows[1].hy0 == 0 &&
               p.rows[1].hy1 == 40 && p.rows[0].hy0 == 9 && p.rows[0].hy1 == 51 && p.rows[2].cx1 == 0 && p.rows[1].h_at == 42 * 50 && p.rows[1].val_at == 2000);
    }

    // refusals, each with its message, before anything is queued
    EXPECT(vghan_anonymize(nullptr, ws, nullptr) == VGHAN_ERR_INVALID && strstr(vghan_last_error(), "null job") && vghan_workspace_bytes(nullptr) == 0);
    EXPECT(refused(good, nullptr, "null workspace") && refused(good, memory + 8, "workspace is not 16-byte aligned"));
#define REFUSED(change, words) \
    do {                       \
        vghan_job b = good;    \
        change;                \
        EXPECT(refused(b, ws, words) && vghan_workspace_bytes(&b) == 0); \
    } while (0)
    REFUSED(b.src_dev = nullptr, "null image");
    REFUSED(b.dst_dev = nullptr, "null image");
    REFUSED(b.dst_dev = dst + 2, "not 4-byte aligned");
    REFUSED(b.height = 0, "image 0 x 100 outside 1 .. 32767");
    REFUSED(b.width = 32768, "outside 1 .. 32767");
    REFUSED(b.src_pitch_bytes = 299, "src_pitch_bytes 299 < width * 3");
    REFUSED(b.n_heads = -1, "n_heads -1 outside 0 .. 65536");
    REFUSED(b.n_heads = 65537, "n_heads 65537 outside 0 .. 65536");
    REFUSED(b.method = 3, "unknown method 3");
    REFUSED(b.region = -1, "unknown region -1");
    REFUSED(b.color = 1 << 24, "color");
    REFUSED(b.reserved = 1, "reserved");
    REFUSED(b.region = VGHAN_REGION_MAP, "owner_dev is null");
    REFUSED(b.owner_dev = (const int32_t*)(memory + 64), "owner_dev is set");
    REFUSED((b.region = VGHAN_REGION_MAP, b.owner_dev = (const int32_t*)(memory + 68)), "owner_dev");
    REFUSED(b.heads = nullptr, "null heads");
    REFUSED(b.taps = nullptr, "blur needs a tap table");
    REFUSED(b.n_taps = 0, "blur needs a tap table");
    REFUSED(b.n_taps = -1, "n_taps -1");
    REFUSED(b.dst_dev = src + 96 * 300, "overlap");
    REFUSED(b.src_dev = dst + 97 * 300 - 4, "overlap");
    REFUSED(b.n_taps = 2, "head 1: taps 2 .. 2 outside the table of 2");
#undef REFUSED
    // per-head refusals name the head
    struct Bad {
        int head;
        vghan_head row;
        int method;
        const char* words;
    } bad[] = {
        {1, {1 << 24, 0, (1 << 24) + 5, 5, 1, 0, 2, 0}, VGHAN_METHOD_BLUR, "head 1: corner"},
        {0, {0, 0, 32768, 5, 1, 0, 2, 0}, VGHAN_METHOD_BLUR, "head 0: box sides 32768 x 5"},
        {2, {5, 5, 4, 9, 1, 0, 2, 0}, VGHAN_METHOD_FILL, "head 2: box sides -1 x 4"},
        {1, {0, 0, 5, 5, 1, 0, 2, 3}, VGHAN_METHOD_FILL, "head 1: reserved"},
        {1, {0, 0, 50, 50, 0, 0, 2, 0}, VGHAN_METHOD_PIXELATE, "head 1: cell side 0"},
        {2, {0, 0, 130, 50, 2, 0, 2, 0}, VGHAN_METHOD_PIXELATE, "head 2: 65 x 25 cells of side 2 exceed 64"},
        {0, {0, 0, 50, 50, 1, 1025, 0, 0}, VGHAN_METHOD_BLUR, "head 0: radius 1025 outside 0 .. 1024"},
        {1, {0, 0, 50, 50, 1, -1, 0, 0}, VGHAN_METHOD_BLUR, "head 1: radius -1"},
        {1, {0, 0, 50, 50, 1, 1, 3, 0}, VGHAN_METHOD_BLUR, "head 1: taps 3 .. 4 outside the table of 4"},
        {2, {0, 0, 50, 50, 1, 0, -1, 0}, VGHAN_METHOD_BLUR, "head 2: taps -1"},
        {1, {0, 0, 50, 50, 1, 1, 1, 0}, VGHAN_METHOD_BLUR, "head 1: tap sum 131073 is not 65536"},
        {2, {0, 0, 50, 50, 1, 0, 3, 0}, VGHAN_METHOD_BLUR, "head 2: tap sum 0 is not 65536"},
    };
    for (const Bad& c : bad) {
        vghan_head keep = heads[c.head];
        heads[c.head] = c.row;
        vghan_job b = good;
        b.method = c.method;
        EXPECT(refused(b, ws, c.words) && vghan_workspace_bytes(&b) == 0);
        heads[c.head] = keep;
    }
    taps[3] = -1;
    {
        vghan_head keep = heads[2];
        heads[2] = {0, 0, 50, 50, 1, 1, 2, 0};
        EXPECT(refused(good, ws, "head 2: tap 1 is -1"));
        heads[2] = keep;
    }
    for (size_t i = 0; i < sizeof(memory); ++i) failures += memory[i] != 0;  // nothing was written anywhere
    free(heads);
    free(taps);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("anonymize host checks passed\n");
    return 0;
}
