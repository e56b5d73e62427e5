// The host half of csrc/yuv_anonymize.hip and csrc/yuv_pack.hip (every argument check, the per-head offsets of both plane groups, the workspace size, the
// packer's arguments) under the host sanitizers.  A program of its own: built with -fsanitize=address,undefined on the host side and run directly -- never
// through Python, never on a GPU.  It makes no call that reaches a device: every job here is either refused before anything is queued or only sized.
#include <stdlib.h>

#include "../head_detector_amd/csrc/yuv_anonymize.hip"
#include "../head_detector_amd/csrc/yuv_pack.hip"

static int failures = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            printf("line %d: %s (message: %s)\n", __LINE__, #cond, vghy_last_error()); \
            ++failures;                                                               \
        }                                                                             \
    } while (0)

static bool refused(const vghy_anonymize_job& j, void* ws, const char* words) {
    const int rc = vghy_anonymize(&j, ws, nullptr);
    return rc == VGHY_ERR_INVALID && strstr(vghy_last_error(), words);
}

static bool pack_refused(const vghy_pack_job& j, const char* words) {
    const int rc = vghy_pack_rgb(&j, nullptr);
    return rc == VGHY_ERR_INVALID && strstr(vghy_last_error(), words);
}

int main() {
    alignas(16) static uint8_t memory[1 << 17];  // stands for device memory: never touched
    uint8_t* y = memory;                         // 97 rows of 100 samples, 104 bytes apart
    uint8_t* uv = memory + 10240;                // 49 rows of 50 (U, V) pairs, 104 bytes apart
    uint8_t* out = memory + 65536;               // a destination elsewhere
    void* ws = memory + 32768;
    // exactly as many rows and taps as the job names: a read past either is a sanitizer report
    vghy_head* luma = (vghy_head*)malloc(3 * sizeof(vghy_head));
    vghy_head* chroma = (vghy_head*)malloc(3 * sizeof(vghy_head));
    int32_t* taps = (int32_t*)malloc(4 * sizeof(int32_t));
    luma[0] = {10, 10, 60, 50, 7, 1, 0, 0};
    luma[1] = {-20, -5, 30, 40, 8, 0, 2, 0};
    luma[2] = {90, 80, 90, 95, 1, 1, 0, 0};  // a zero side
    chroma[0] = {5, 5, 30, 25, 4, 1, 0, 0};
    chroma[1] = {-10, -3, 15, 20, 4, 0, 2, 0};
    chroma[2] = {45, 40, 45, 48, 1, 1, 0, 0};
    taps[0] = 65534, taps[1] = 1, taps[2] = 65536, taps[3] = 0;
    vghy_anonymize_job good = {};  // NV12, in place
    good.planes[0] = {y, y, 104, 104, 1, 1};
    good.planes[1] = {uv, uv, 104, 104, 2, 2};
    good.planes[2] = {uv + 1, uv + 1, 104, 104, 2, 2};
    good.height = 97, good.width = 100, good.n_heads = 3, good.method = VGHY_METHOD_BLUR, good.region = VGHY_REGION_ELLIPSE;
    good.luma_heads = luma, good.chroma_heads = chroma, good.taps = taps, good.n_taps = 4;

    // sizes: the owner plane; one byte a luma and two a chroma sample of the clipped boxes; the u16 h rows extended by r
    const int64_t owner = 4 * 97 * 100, vl = 50 * 40 + 30 * 40, vc = 2 * (25 * 20 + 15 * 20), hl = 2 * ((40 + 2) * 50 + 40 * 30), hc = 4 * ((20 + 2) * 25 + 20 * 15);
    EXPECT(vghy_anonymize_workspace_bytes(&good) == up16(up16(up16(up16(owner) + vl) + vc) + hl) + up16(hc));
    vghy_anonymize_job j = good;
    j.method = VGHY_METHOD_FILL;
    EXPECT(vghy_anonymize_workspace_bytes(&j) == up16(owner));
    j.method = VGHY_METHOD_PIXELATE;  // luma 8 x 6 and 7 x 6 cells, chroma 7 x 5 and 7 x 6
    EXPECT(vghy_anonymize_workspace_bytes(&j) == up16(up16(owner + 48 + 42) + 2 * (35 + 42)));
    j.region = VGHY_REGION_MAP, j.owner_dev = (const int32_t*)(memory + 64);
    EXPECT(vghy_anonymize_workspace_bytes(&j) == up16(up16(48 + 42) + 2 * (35 + 42)));
    j.n_heads = 0, j.luma_heads = nullptr, j.chroma_heads = nullptr;
    EXPECT(vghy_anonymize_workspace_bytes(&j) == 16);
    {
        Plan p;
        EXPECT(make_plan(&good, p, "t") == OK && p.in_place[0] && p.in_place[1] && p.in_place[2] && p.spair == 1 && p.dpair == 1);
        EXPECT(p.luma.rows.size() == 3 && p.luma.tiles[3] == 1 * 10 + 1 * 10 && p.luma.segments[3] == 42 + 40 && p.luma.rows[1].cx0 == 0 && p.luma.rows[1].hy1 == 40 &&
               p.luma.rows[0].hy0 == 9 && p.luma.rows[0].hy1 == 51 && p.luma.rows[2].cx1 == 0 && p.luma.rows[1].h_at == 42 * 50 && p.luma.rows[1].val_at == 2000);
        EXPECT(p.chroma.tiles[3] == 5 + 5 && p.chroma.segments[3] == 22 + 20 && p.chroma.rows[1].cx1 == 15 && p.chroma.rows[1].cy1 == 20 && p.chroma.rows[0].hy0 == 4 &&
               p.chroma.rows[0].hy1 == 26 && p.chroma.rows[1].h_at == 22 * 25 && p.chroma.rows[1].val_at == 500 && p.chroma.rows[2].cy1 == 0);
        vghy_anonymize_job o = good;  // out of place into planar chroma (NV12 -> I420); NV21 source
        o.planes[0].dst_dev = out, o.planes[0].dst_pitch = 100;
        o.planes[1].dst_dev = out + 9700, o.planes[1].dst_pitch = 50, o.planes[1].dst_step = 1;
        o.planes[2].dst_dev = out + 9700 + 2450, o.planes[2].dst_pitch = 50, o.planes[2].dst_step = 1;
        o.planes[1].src_dev = uv + 1, o.planes[2].src_dev = uv;
        EXPECT(make_plan(&o, p, "t") == OK && !p.in_place[0] && !p.in_place[1] && !p.in_place[2] && p.spair == 2 && p.dpair == 0);
        o.planes[1].src_dev = uv + 2, o.planes[2].src_dev = uv + 1;  // pairs that start at an odd byte are handled as two planes
        EXPECT(make_plan(&o, p, "t") == OK && p.spair == 0);
    }

    // refusals, each with its message, before anything is queued
    EXPECT(vghy_anonymize(nullptr, ws, nullptr) == VGHY_ERR_INVALID && strstr(vghy_last_error(), "null job") && vghy_anonymize_workspace_bytes(nullptr) == 0);
    EXPECT(refused(good, nullptr, "null workspace") && refused(good, memory + 8, "workspace is not 16-byte aligned"));
#define REFUSED(change, words)                                                    \
    do {                                                                          \
        vghy_anonymize_job b = good;                                              \
        change;                                                                   \
        EXPECT(refused(b, ws, words) && vghy_anonymize_workspace_bytes(&b) == 0); \
    } while (0)
    REFUSED(b.planes[0].src_dev = nullptr, "plane Y: null plane");
    REFUSED(b.planes[2].dst_dev = nullptr, "plane V: null plane");
    REFUSED(b.planes[1].src_step = 3, "plane U: steps 3 and 2 are not 1 or 2");
    REFUSED(b.planes[0].dst_step = 0, "plane Y: steps 1 and 0");
    REFUSED(b.planes[0].src_pitch = 99, "plane Y: src_pitch 99 outside 100");
    REFUSED(b.planes[1].dst_pitch = 98, "plane U: dst_pitch 98 outside 99");
    REFUSED(b.height = 0, "frame 0 x 100 outside 1 .. 32767");
    REFUSED(b.width = 32768, "outside 1 .. 32767");
    REFUSED(b.planes[0].dst_pitch = 105, "plane Y: the destination starts where the source does with another pitch or step");
    REFUSED(b.planes[1].dst_step = 1, "plane U: the destination starts where the source does");
    REFUSED(b.planes[0].dst_dev = y + 104, "plane Y: the destination overlaps source plane Y");
    REFUSED(b.planes[0].dst_dev = uv - 104, "plane Y: the destination overlaps source plane U");
    REFUSED(b.planes[2].dst_dev = uv + 3, "plane V: the destination overlaps source plane U");
    REFUSED((b.planes[1].dst_dev = y + 96 * 104 + 99, b.planes[1].dst_pitch = 50, b.planes[1].dst_step = 1), "plane U: the destination overlaps source plane Y");
    REFUSED(b.n_heads = -1, "n_heads -1 outside 0 .. 65536");
    REFUSED(b.n_heads = 65537, "n_heads 65537 outside 0 .. 65536");
    REFUSED(b.method = 3, "unknown method 3");
    REFUSED(b.region = -1, "unknown region -1");
    REFUSED(b.color = 1 << 24, "color");
    REFUSED(b.reserved = 1, "reserved");
    REFUSED(b.region = VGHY_REGION_MAP, "owner_dev is null");
    REFUSED(b.owner_dev = (const int32_t*)(memory + 64), "owner_dev is set");
    REFUSED((b.region = VGHY_REGION_MAP, b.owner_dev = (const int32_t*)(memory + 68)), "owner_dev");
    REFUSED(b.luma_heads = nullptr, "null heads");
    REFUSED(b.chroma_heads = nullptr, "null heads");
    REFUSED(b.taps = nullptr, "blur needs a tap table");
    REFUSED(b.n_taps = 0, "blur needs a tap table");
    REFUSED(b.n_taps = -1, "n_taps -1");
    REFUSED(b.n_taps = 2, "luma head 1: taps 2 .. 2 outside the table of 2");
#undef REFUSED
    // per-head refusals name the plane group and the head
    struct Bad {
        bool in_chroma;
        int head;
        vghy_head row;
        int method;
        const char* words;
    } bad[] = {
        {false, 1, {1 << 24, 0, (1 << 24) + 5, 5, 1, 0, 2, 0}, VGHY_METHOD_BLUR, "luma head 1: corner"},
        {true, 0, {0, 0, 32768, 5, 1, 0, 2, 0}, VGHY_METHOD_BLUR, "chroma head 0: box sides 32768 x 5"},
        {false, 2, {5, 5, 4, 9, 1, 0, 2, 0}, VGHY_METHOD_FILL, "luma head 2: box sides -1 x 4"},
        {true, 1, {0, 0, 5, 5, 1, 0, 2, 3}, VGHY_METHOD_FILL, "chroma head 1: reserved"},
        {true, 1, {0, 0, 50, 50, 0, 0, 2, 0}, VGHY_METHOD_PIXELATE, "chroma head 1: cell side 0"},
        {false, 2, {0, 0, 130, 50, 2, 0, 2, 0}, VGHY_METHOD_PIXELATE, "luma head 2: 65 x 25 cells of side 2 exceed 64"},
        {true, 0, {0, 0, 50, 50, 1, 1025, 0, 0}, VGHY_METHOD_BLUR, "chroma head 0: radius 1025 outside 0 .. 1024"},
        {false, 1, {0, 0, 50, 50, 1, -1, 0, 0}, VGHY_METHOD_BLUR, "luma head 1: radius -1"},
        {true, 1, {0, 0, 50, 50, 1, 1, 3, 0}, VGHY_METHOD_BLUR, "chroma head 1: taps 3 .. 4 outside the table of 4"},
        {false, 2, {0, 0, 50, 50, 1, 0, -1, 0}, VGHY_METHOD_BLUR, "luma head 2: taps -1"},
        {true, 1, {0, 0, 50, 50, 1, 1, 1, 0}, VGHY_METHOD_BLUR, "chroma head 1: tap sum 131073 is not 65536"},
        {false, 2, {0, 0, 50, 50, 1, 0, 3, 0}, VGHY_METHOD_BLUR, "luma head 2: tap sum 0 is not 65536"},
    };
    for (const Bad& c : bad) {
        vghy_head* rows = c.in_chroma ? chroma : luma;
        vghy_head keep = rows[c.head];
        rows[c.head] = c.row;
        vghy_anonymize_job b = good;
        b.method = c.method;
        EXPECT(refused(b, ws, c.words) && vghy_anonymize_workspace_bytes(&b) == 0);
        rows[c.head] = keep;
    }
    taps[3] = -1;
    {
        vghy_head keep = chroma[2];
        chroma[2] = {0, 0, 50, 50, 1, 1, 2, 0};
        EXPECT(refused(good, ws, "chroma head 2: tap 1 is -1"));
        chroma[2] = keep;
    }

    // the packer: its arguments, and every refusal
    vghy_pack_job pack = {};
    pack.src_dev = memory, pack.src_pitch_bytes = 304, pack.height = 97, pack.width = 100, pack.y_offset = 16;
    pack.planes[0] = {nullptr, out, 0, 104, 0, 1};
    pack.planes[1] = {nullptr, out + 10240 + 1, 0, 104, 0, 2};  // NV21
    pack.planes[2] = {nullptr, out + 10240, 0, 104, 0, 2};
    const int32_t k709[9] = {11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639};
    for (int k = 0; k < 9; ++k) pack.coef[k] = k709[k];
    {
        PackArgs a;
        EXPECT(pack_plan(&pack, a) == OK && a.pair == 2 && a.W == 100 && a.H == 97 && a.CW == 50 && a.CH == 49 && a.coef[8] == -2639 && a.y_offset == 16 && a.y.dst == out);
        vghy_pack_job planar = pack;
        planar.planes[1] = {nullptr, out + 10240, 0, 50, 0, 1};
        planar.planes[2] = {nullptr, out + 10240 + 2450, 0, 50, 0, 1};
        EXPECT(pack_plan(&planar, a) == OK && a.pair == 0 && a.c[1].dstep == 1);
    }
    EXPECT(vghy_pack_rgb(nullptr, nullptr) == VGHY_ERR_INVALID && strstr(vghy_last_error(), "null job"));
#define PACK_REFUSED(change, words)     \
    do {                                \
        vghy_pack_job b = pack;         \
        change;                         \
        EXPECT(pack_refused(b, words)); \
    } while (0)
    PACK_REFUSED(b.src_dev = nullptr, "null image");
    PACK_REFUSED(b.height = 0, "image 0 x 100 outside 1 .. 32767");
    PACK_REFUSED(b.width = 40000, "outside 1 .. 32767");
    PACK_REFUSED(b.src_pitch_bytes = 299, "src_pitch_bytes 299 < width * 3 = 300");
    PACK_REFUSED(b.y_offset = 256, "y_offset 256 outside 0 .. 255");
    PACK_REFUSED(b.coef[4] = (1 << 20) + 1, "coefficient 4 is 1048577");
    PACK_REFUSED(b.planes[1].dst_dev = nullptr, "plane U: null plane");
    PACK_REFUSED(b.planes[0].src_pitch = 104, "plane Y: the src_ fields");
    PACK_REFUSED(b.planes[2].dst_step = 4, "plane V: step 4 is not 1 or 2");
    PACK_REFUSED(b.planes[0].dst_pitch = 99, "plane Y: dst_pitch 99 outside 100");
    PACK_REFUSED(b.planes[0].dst_dev = memory + 96 * 304 + 299, "plane Y overlaps the source image");
    PACK_REFUSED(b.src_dev = out + 10240 + 48 * 104 + 99 - 96 * 304, "overlaps the source image");
#undef PACK_REFUSED
    for (size_t i = 0; i < sizeof(memory); ++i) failures += memory[i] != 0;  // nothing was written anywhere
    free(luma);
    free(chroma);
    free(taps);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("yuv_anonymize host checks passed\n");
    return 0;
}
