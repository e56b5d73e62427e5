// csrc/head_crop_rules.h (the integer functions of the head-tensor rule, the validation of a job, the tile count) under the host sanitizers.  A program of its
// own: built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU.  It includes the rule header alone and
// makes no HIP call: every job here is only validated.
#include <stdlib.h>
#include <string.h>

#include "../head_detector_amd/csrc/head_crop_rules.h"

using namespace head_crop;

static int failures = 0;
static char msg[400];

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("line %d: %s (message: %s)\n", __LINE__, #cond, msg);  \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static bool refused(const vghc_job& j, const char* words) {
    msg[0] = 0;
    const char* m = validate(&j, msg, sizeof(msg));
    return m == msg && strstr(msg, words);
}

static bool accepted(const vghc_job& j) {
    msg[0] = 0;
    return validate(&j, msg, sizeof(msg)) == nullptr;
}

int main() {
    // ---- the integer functions against hand-computed values ----
    const int64_t one = (int64_t)1 << 32;
    EXPECT(sub_position(10 * one, one / 2, -one / 4, 3, 8) == 10 * one + 3 * (one / 2) - 2 * one);
    EXPECT(sub_position(-(one * 40000), one, 0, 8191, 8191) == -(one * 40000) + 8191 * one);
    EXPECT(source_pixel(5 * one + one / 2) == 5 && source_pixel(-1) == -1 && source_pixel(-one) == -1 && source_pixel(-one - 1) == -2 && source_pixel(0) == 0);
    EXPECT(source_pixel(40000 * one) == 40000 && source_pixel(((int64_t)1 << 62) - 1) == (1 << 30) - 1 && source_pixel(-(((int64_t)1 << 62) - 1)) == -(1 << 30));
    EXPECT(fraction(0) == 0 && fraction(one / 2) == 16 && fraction(one - 1) == 31 && fraction(one / 32) == 1 && fraction(one / 32 - 1) == 0);
    EXPECT(fraction(-1) == 31 && fraction(-one / 2) == 16 && fraction(-one) == 0);  // the fraction of a negative position counts up from its floor
    EXPECT(fraction(3 * one + (one / 64)) == 0 && fraction(3 * one + (one / 64) + ((int64_t)1 << 26)) == 1);  // + 2^26 rounds to nearest
    EXPECT(tap4(0, 0, 200, 1, 2, 3) == 1024 * 200 && tap4(31, 31, 1, 2, 3, 200) == 1 * 1 + 31 * 2 + 31 * 3 + 961 * 200);
    EXPECT(tap4(16, 0, 10, 20, 99, 99) == 512 * 10 + 512 * 20 && tap4(0, 8, 100, 0, 200, 0) == 24 * 32 * 100 + 8 * 32 * 200);
    for (int fx = 0; fx < 32; ++fx)
        for (int fy = 0; fy < 32; ++fy) EXPECT(tap4(fx, fy, 255, 255, 255, 255) == 255 * 1024);  // the weights sum to 1024
    EXPECT(round_u8(0, 1) == 0 && round_u8(255 * 1024, 1) == 255 && round_u8(255 * 1024 * 64, 8) == 255 && round_u8(511, 1) == 0 && round_u8(512, 1) == 1);
    EXPECT(round_u8(1024 * 9 * 7 + 4607, 3) == 7 && round_u8(1024 * 9 * 7 + 4608, 3) == 8);  // half rounds up
    EXPECT(clamp8(-1) == 0 && clamp8(256) == 255 && clamp8(77) == 77);
    vghc_source yuv = {};
    yuv.y_offset = 16, yuv.cy = 76309, yuv.crv = 117489, yuv.cgu = -13975, yuv.cgv = -34925, yuv.cbu = 138438;  // BT.709, limited range
    EXPECT(yuv_channel(yuv, 16, 128, 128, 0) == 0 && yuv_channel(yuv, 235, 128, 128, 1) == 255 && yuv_channel(yuv, 126, 128, 128, 2) == 128);
    EXPECT(((76309 * 65 + 117489 * 112 + 32768) >> 16) == 276 && yuv_channel(yuv, 81, 90, 240, 0) == 255 && yuv_channel(yuv, 81, 90, 240, 1) == ((76309 * 65 + 13975 * 38 - 34925 * 112 + 32768) >> 16));
    EXPECT(yuv_channel(yuv, 81, 90, 240, 1) == 24 && yuv_channel(yuv, 81, 90, 240, 2) == 0);  // a red: (76309 * 65 - 138438 * 38 + 32768) >> 16 is negative
    EXPECT(yuv_channel(yuv, 255, 255, 255, 0) == 255 && yuv_channel(yuv, 0, 0, 0, 2) == 0);  // clamped on both sides
    yuv.cy = yuv.crv = yuv.cgu = yuv.cgv = yuv.cbu = kMaxCoef;  // the largest coefficients: nothing overflows
    yuv.y_offset = 0;
    EXPECT(yuv_channel(yuv, 255, 255, 255, 1) == 255);
    yuv.cy = yuv.cgu = yuv.cgv = -kMaxCoef;
    EXPECT(yuv_channel(yuv, 255, 255, 255, 1) == 0);

    // ---- the tile count ----
    EXPECT(tiles_per_side(1) == 1 && tiles_per_side(16) == 1 && tiles_per_side(17) == 2 && tiles_per_side(1024) == 64);
    EXPECT(tile_count(0, 224) == 0 && tile_count(3, 33) == 27 && tile_count(100, 224) == 19600 && tile_count(65536, 1024) == 268435456ll);
    EXPECT(element_bytes(VGHC_DTYPE_U8) == 1 && element_bytes(VGHC_DTYPE_F32) == 4 && element_bytes(VGHC_DTYPE_F16) == 2 && element_bytes(VGHC_DTYPE_BF16) == 2);

    // ---- the validation at each limit and one past it ----
    alignas(16) static uint8_t memory[64];  // stands for device memory: never touched
    // exactly as many rows as the job names: a read past either array is a sanitizer report
    vghc_source* sources = (vghc_source*)calloc(2, sizeof(vghc_source));
    vghc_head* heads = (vghc_head*)calloc(2, sizeof(vghc_head));
    sources[0].kind = VGHC_SOURCE_RGB, sources[0].h = 97, sources[0].w = 131, sources[0].rgb_dev = memory, sources[0].rgb_pitch_bytes = 393;
    sources[1].kind = VGHC_SOURCE_YUV420, sources[1].h = 37, sources[1].w = 51, sources[1].chroma_step = 2, sources[1].y_dev = memory, sources[1].u_dev = memory + 1;
    sources[1].v_dev = memory + 2, sources[1].y_pitch_bytes = 51, sources[1].uv_pitch_bytes = 52, sources[1].y_offset = 16, sources[1].cy = 76309, sources[1].crv = 117489;
    sources[1].cgu = -13975, sources[1].cgv = -34925, sources[1].cbu = 138438;
    for (int k = 0; k < 2; ++k) {
        heads[k].x0 = 10 * one, heads[k].xp = one / 2, heads[k].y0 = -3 * one, heads[k].yq = one / 2, heads[k].source = k, heads[k].supersample = 2;
        heads[k].a[0] = heads[k].a[1] = heads[k].a[2] = 1.0f;
    }
    vghc_job good = {};
    good.sources = sources, good.heads = heads, good.n_sources = 2, good.n_heads = 2, good.size = 17, good.dtype = VGHC_DTYPE_F32, good.layout = VGHC_LAYOUT_NCHW;
    good.channel_order = VGHC_ORDER_RGB, good.fill = 0x0a0b0c, good.dst_dev = memory + 16, good.dst_bytes = 2 * 3 * 17 * 17 * 4;
    EXPECT(accepted(good));
    EXPECT(validate(nullptr, msg, sizeof(msg)) == msg && strstr(msg, "null job"));

    vghc_job j = good;
#define WITH(change, words) \
    j = good;               \
    change;                 \
    EXPECT(refused(j, words))
#define ALLOWED(change) \
    j = good;           \
    change;             \
    EXPECT(accepted(j))
    WITH(j.size = 0, "size 0 outside 1 .. 1024");
    WITH(j.size = 1025, "size 1025");
    ALLOWED((j.size = 1, j.dst_bytes = 24));
    ALLOWED((j.size = 1024, j.dst_bytes = 2ll * 3 * 1024 * 1024 * 4));
    WITH(j.n_heads = -1, "n_heads -1");
    WITH(j.n_heads = 65537, "n_heads 65537 outside 0 .. 65536");
    WITH(j.n_sources = -1, "n_sources -1");
    WITH(j.dtype = 4, "unknown dtype 4");
    WITH(j.dtype = -1, "unknown dtype -1");
    WITH(j.layout = 2, "unknown layout 2");
    WITH(j.channel_order = 2, "unknown channel order 2");
    WITH(j.fill = 1 << 24, "fill");
    WITH(j.fill = -1, "fill");
    WITH(j.dst_bytes = -1, "dst_bytes -1");
    WITH(j.b[1] = __builtin_inff(), "b[1] is not finite");
    WITH(j.b[2] = __builtin_nanf(""), "b[2] is not finite");
    WITH(j.sources = nullptr, "null sources");
    WITH(j.n_sources = 0, "null sources");
    WITH(j.heads = nullptr, "null heads");
    WITH(j.dst_dev = nullptr, "null dst_dev");
    WITH(j.dst_dev = memory + 18, "not aligned to its 4-byte elements");
    ALLOWED((j.dst_dev = memory + 18, j.dtype = VGHC_DTYPE_BF16));
    WITH((j.dst_dev = memory + 17, j.dtype = VGHC_DTYPE_F16), "not aligned to its 2-byte elements");
    ALLOWED((j.dst_dev = memory + 17, j.dtype = VGHC_DTYPE_U8));
    WITH(j.dst_bytes = 2 * 3 * 17 * 17 * 4 - 1, "needs 6936 bytes, the destination has 6935");
    ALLOWED((j.n_heads = 0, j.sources = nullptr, j.heads = nullptr, j.dst_dev = nullptr, j.dst_bytes = 0, j.n_sources = 0));  // no heads: nothing else is looked at
    // sources
    WITH(sources[0].kind = 2, "source 0: unknown kind 2");
    sources[0].kind = VGHC_SOURCE_RGB;
    WITH(sources[0].h = 0, "source 0: 0 x 131");
    WITH(sources[0].h = 32768, "source 0: 32768 x 131 outside 1 .. 32767");
    ALLOWED(sources[0].h = 32767);
    WITH((sources[0].h = 97, sources[0].w = 32768, sources[0].rgb_pitch_bytes = 3 * 32768), "outside 1 .. 32767");
    ALLOWED((sources[0].w = 32767, sources[0].rgb_pitch_bytes = 3 * 32767));
    WITH((sources[0].w = 131, sources[0].rgb_pitch_bytes = 392), "rgb_pitch_bytes 392 < w * 3 = 393");
    WITH((sources[0].rgb_pitch_bytes = 393, sources[0].rgb_dev = nullptr), "source 0: null rgb_dev");
    sources[0].rgb_dev = memory;
    WITH(sources[1].v_dev = nullptr, "source 1: null plane");
    sources[1].v_dev = memory + 2;
    WITH(sources[1].chroma_step = 3, "chroma_step 3");
    WITH((sources[1].chroma_step = 2, sources[1].y_pitch_bytes = 50), "y_pitch_bytes 50 < w = 51");
    WITH((sources[1].y_pitch_bytes = 51, sources[1].uv_pitch_bytes = 51), "uv_pitch_bytes 51 < chroma_step * ((w + 1) / 2) = 52");
    ALLOWED((sources[1].chroma_step = 1, sources[1].uv_pitch_bytes = 26));
    WITH(sources[1].uv_pitch_bytes = 25, "uv_pitch_bytes 25");
    WITH((sources[1].chroma_step = 2, sources[1].uv_pitch_bytes = 52, sources[1].y_offset = 256), "y_offset 256 outside 0 .. 255");
    WITH((sources[1].y_offset = 16, sources[1].cgv = -kMaxCoef - 1), "coefficient -1048577");
    ALLOWED(sources[1].cgv = -kMaxCoef);
    WITH(sources[1].cbu = kMaxCoef + 1, "coefficient 1048577");
    ALLOWED(sources[1].cbu = kMaxCoef);
    // heads
    WITH(heads[1].source = 2, "head 1: source 2 outside the 2 supplied");
    WITH(heads[1].source = -1, "head 1: source -1");
    WITH((heads[1].source = 1, heads[0].supersample = 0), "head 0: supersample 0 outside 1 .. 8");
    WITH(heads[0].supersample = 9, "head 0: supersample 9");
    ALLOWED(heads[0].supersample = 8);
    WITH((heads[0].supersample = 2, heads[1].reserved = 5), "head 1: reserved is 5");
    WITH((heads[1].reserved = 0, heads[1].a[2] = -__builtin_inff()), "head 1: a[2] is not finite");
    heads[1].a[2] = 1.0f;
    // the 2^62 position bound, where a naive |x0| + S K (|xp| + |xq|) in int64 would be a signed overflow: S K = 34 here
    const int64_t limit = (int64_t)1 << 62;
    WITH(heads[0].x0 = limit, "head 0: |x0| + S K (|xp| + |xq|) reaches 2^62");
    WITH(heads[0].x0 = -limit, "head 0: |x0|");
    WITH(heads[0].x0 = INT64_MIN, "head 0: |x0|");
    WITH(heads[0].x0 = INT64_MAX, "head 0: |x0|");
    ALLOWED((heads[0].x0 = limit - 1, heads[0].xp = 0));
    ALLOWED((heads[0].x0 = -(limit - 1), heads[0].xp = 0));
    WITH((heads[0].x0 = limit - 34, heads[0].xp = 1), "head 0: |x0|");     // exactly 2^62
    ALLOWED((heads[0].x0 = limit - 35, heads[0].xp = -1));                  // 2^62 - 1
    WITH((heads[0].x0 = 0, heads[0].xp = INT64_MIN, heads[0].xq = INT64_MIN), "head 0: |x0|");
    WITH((heads[0].xp = INT64_MAX, heads[0].xq = INT64_MAX), "head 0: |x0|");
    WITH((heads[0].xp = limit / 34 + 1, heads[0].xq = 0), "head 0: |x0|");
    WITH((j.size = 16, heads[0].xp = limit / 64, heads[0].xq = -(limit / 64)), "head 0: |x0|");  // S K = 32: 32 * 2 * 2^56 = 2^62
    ALLOWED((j.size = 16, heads[0].xp = limit / 64, heads[0].xq = -(limit / 64) + 1));              // 2^62 - 32
    heads[0].xp = one / 2, heads[0].xq = 0, heads[0].x0 = 10 * one;
    WITH(heads[1].y0 = INT64_MIN, "head 1: |y0| + S K (|yp| + |yq|) reaches 2^62");
    WITH((heads[1].y0 = 0, heads[1].yq = limit / 34 + 1), "head 1: |y0|");
    ALLOWED(heads[1].yq = limit / 34 - 1);
    heads[1].y0 = -3 * one, heads[1].yq = one / 2;
    EXPECT(accepted(good));
    // the most tiles one launch takes
    ALLOWED((j.n_heads = 0, j.size = 1024));
    EXPECT(tile_count(4096, 1024) == VGHC_MAX_TILES && tile_count(4097, 1024) > VGHC_MAX_TILES);
    {
        vghc_head* many = (vghc_head*)calloc(4097, sizeof(vghc_head));
        for (int k = 0; k < 4097; ++k) many[k] = heads[0];
        j = good, j.heads = many, j.size = 1024, j.n_heads = 4097, j.dst_bytes = 4097ll * 3 * 1024 * 1024 * 4;
        EXPECT(refused(j, "16781312 tiles exceed one launch"));
        j.n_heads = 4096;
        EXPECT(accepted(j));
        free(many);
    }
    free(sources);
    free(heads);
    if (failures) {
        printf("%d head crop host checks FAILED\n", failures);
        return 1;
    }
    printf("head crop host checks passed\n");
    return 0;
}
