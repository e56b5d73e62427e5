// Stand-alone check of csrc/conv_tiles.h: the class table of every tile family, the launch-level rule (one admitted launch and its smallest refusing neighbour per clause)
// and the tile counts.  tests/test_conv_tiles_host.py builds it with the host sanitizers (address, undefined), as the product and with -DVGH_EXPERIMENTS, and runs it on
// its own.  It makes no HIP call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../head_detector_amd/csrc/conv_tiles.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            if (failures > 20) exit(1);   \
        }                                 \
    } while (0)

using F = TileFamily;
static const uint16_t kSome[8] = {0};
static const float kSomeF[8] = {0};

// a PREPARED dense conv as both callers of the launchers describe it: pad = ksize / 2, Ho = ceil(H / stride), whole channel counts, 16-byte epilogue, ReLU
static ConvArgs conv(int ksize, int stride, int B, int H, int W, int cin, int cout) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.ksize = ksize, a.stride = stride, a.pad = ksize / 2;
    a.B = B, a.H = H, a.W = W, a.Ho = (H + 2 * a.pad - ksize) / stride + 1, a.Wo = (W + 2 * a.pad - ksize) / stride + 1;
    a.P = B * a.Ho * a.Wo;
    a.cin = cin, a.cblocks = cin / 32, a.nkb = ksize * ksize * a.cblocks, a.in_pitch = cin;
    a.cout_pad = a.cout_store = a.out_split = cout, a.out_pitch = cout;
    a.act = VGH_ACT_RELU, a.fast_epi = 1;
    return a;
}
template <class Fn>
static ConvArgs with(ConvArgs a, Fn change) {
    change(a);
    return a;
}
static ConvArgs fp16_single(ConvArgs a) {  // what vgh_launch_conv_split makes of a single-plane fp16 launch
    a.split = VGH_FMT_F16X2, a.nseg = 1, a.seg_kb = a.nkb, a.out_scale = 1.0f;
    return a;
}

// THE EXPECTED VALUES WERE NOT TAKEN FROM tile_admits: every row that names a tile was answered by the library as it was before conv_tiles.h existed (cfg_ok_for of that
// tile; for the split table its scfg_ok / pp16_ok, held verbatim by the program that compared the two rules over the whole grid: profiles/conv_tiles_refactor.txt), and
// the rows without a tile (KBS = 3 / 4: no row of the split table has more than 2) by that verbatim copy on a made-up row.
struct Case {
    const char* what;
    const char* tile;  // its name in the bf16 table, "split:" + its name in the split table, or nullptr
    F family;
    int BC, KBS;
    ConvArgs a;
    bool admitted;
};
static int make_cases(Case* out) {
    int n = 0;
    auto add = [&](const char* what, const char* tile, F f, int BC, int KBS, const ConvArgs& a, bool admitted) { out[n++] = Case{what, tile, f, BC, KBS, a, admitted}; };
    const ConvArgs c128 = conv(3, 1, 2, 16, 16, 128, 128), c96 = conv(3, 1, 2, 16, 16, 96, 96);
    // cout tile, groups, the class columns reached through a launch
    add("igemm: any conv", "128x128_w64x64_k1", F::Igemm, 128, 1, with(conv(1, 1, 2, 11, 13, 64, 128), [](ConvArgs& a) { a.out_f32 = 1, a.fast_epi = 0, a.act = VGH_ACT_SILU; }), true);
    add("igemm: cout_pad 192 % 128", "128x128_w64x64_k1", F::Igemm, 128, 1, conv(3, 1, 2, 16, 16, 128, 192), false);
    add("igemm: group of 128", "128x128_w64x64_k1", F::Igemm, 128, 1, with(conv(3, 1, 2, 16, 16, 64, 256), [](ConvArgs& a) { a.grp_cout = 128, a.grp_in_stride = 64; }), true);
    add("igemm: group of 64 straddles", "128x128_w64x64_k1", F::Igemm, 128, 1, with(conv(3, 1, 2, 16, 16, 64, 256), [](ConvArgs& a) { a.grp_cout = 64, a.grp_in_stride = 64; }), false);
    add("p: 3x3 / stride 1", "p16x16x128_n4x2", F::Patch, 128, 1, c128, true);
    add("p: 1x1", "p16x16x128_n4x2", F::Patch, 128, 1, conv(1, 1, 2, 16, 16, 128, 128), false);
    add("p: stride 2", "p16x16x128_n4x2", F::Patch, 128, 1, conv(3, 2, 2, 16, 16, 128, 128), false);
    add("p: fp32 output", "p16x16x128_n4x2", F::Patch, 128, 1, with(c128, [](ConvArgs& a) { a.out_f32 = 1; }), false);
    add("p: unaligned epilogue", "p16x16x128_n4x2", F::Patch, 128, 1, with(c128, [](ConvArgs& a) { a.fast_epi = 0; }), false);
    add("q: ragged channels admitted (launch moves to the p twin)", "q16x16x128_n4x2", F::PatchPipe, 128, 1, with(c128, [](ConvArgs& a) { a.cout_store = 124; }), true);
    add("p: SiLU, residual, group of 128", "p16x16x128_n4x2", F::Patch, 128, 1, with(conv(3, 1, 2, 16, 16, 64, 256), [](ConvArgs& a) { a.act = VGH_ACT_SILU, a.res = kSome, a.res_pitch = 256, a.grp_cout = 128; }), true);
    // 8-bit links and the diagonal bypass
    add("g: e4m3 link", "g8x8x128_n8", F::PingPongG, 128, 1, with(c128, [](ConvArgs& a) { a.in_fp8 = 1, a.gscale = kSomeF; }), true);
    add("h: e4m3 link", "h8x8x128_n8", F::PingPongH, 128, 1, with(c128, [](ConvArgs& a) { a.in_fp8 = 1, a.gscale = kSomeF; }), false);
    add("p: int8 output", "p16x16x128_n4x2", F::Patch, 128, 1, with(c128, [](ConvArgs& a) { a.out_fp8 = 2, a.gscale = kSomeF; }), false);
    add("g96: dvec", "g8x8x96_n8", F::PingPongG, 96, 1, with(conv(3, 1, 2, 16, 16, 384, 384), [](ConvArgs& a) { a.in_fp8 = 2, a.gscale = kSomeF, a.dvec = kSomeF; }), true);
    add("g128: dvec", "g8x8x128_n8", F::PingPongG, 128, 1, with(conv(3, 1, 2, 16, 16, 384, 384), [](ConvArgs& a) { a.in_fp8 = 2, a.gscale = kSomeF, a.dvec = kSomeF; }), false);
    // ping-pong tiles: dense, ReLU / none, 16-bit; the s tile's smallest map and cout limit
    add("g: residual", "g8x8x128_n8", F::PingPongG, 128, 1, with(c128, [](ConvArgs& a) { a.res = kSome, a.res_pitch = 128; }), true);
    add("g: SiLU", "g8x8x128_n8", F::PingPongG, 128, 1, with(c128, [](ConvArgs& a) { a.act = VGH_ACT_SILU; }), false);
    add("h: group of 128", "h8x8x128_n8", F::PingPongH, 128, 1, with(conv(3, 1, 2, 16, 16, 64, 256), [](ConvArgs& a) { a.grp_cout = 128; }), false);
    add("g: cout_pad 2048", "g8x8x128_n8", F::PingPongG, 128, 1, conv(3, 1, 1, 8, 8, 32, 2048), true);
    add("g: cout_pad 2176", "g8x8x128_n8", F::PingPongG, 128, 1, conv(3, 1, 1, 8, 8, 32, 2176), false);
    add("s: 4 x 8 map", "s4x8x128_n8", F::PingPongS, 128, 1, conv(3, 1, 2, 4, 8, 128, 128), true);
    add("s: 3 x 8 map", "s4x8x128_n8", F::PingPongS, 128, 1, conv(3, 1, 2, 3, 8, 128, 128), false);
    add("s: 8 x 7 map", "s4x8x128_n8", F::PingPongS, 128, 1, conv(3, 1, 2, 8, 7, 128, 128), false);
    add("g: 3 x 8 map", "g8x8x128_n8", F::PingPongG, 128, 1, conv(3, 1, 2, 3, 8, 128, 128), true);
    add("s: cout_pad 1024", "s4x8x128_n8", F::PingPongS, 128, 1, conv(3, 1, 1, 8, 8, 32, 1024), true);
    add("s: cout_pad 1152", "s4x8x128_n8", F::PingPongS, 128, 1, conv(3, 1, 1, 8, 8, 32, 1152), false);
    // streaming 1x1 tiles
    const ConvArgs t96 = conv(1, 1, 2, 11, 13, 96, 96);
    add("t: plain 1x1", "t128x96_w32x96_k1_r3", F::Stream, 96, 1, t96, true);
    add("t: residual", "t128x96_w32x96_k1_r3", F::Stream, 96, 1, with(t96, [](ConvArgs& a) { a.res = kSome, a.res_pitch = 96; }), false);
    add("t: pad 1", "t128x96_w32x96_k1_r3", F::Stream, 96, 1, with(t96, [](ConvArgs& a) { a.pad = 1; }), false);
    add("t: SiLU", "t128x96_w32x96_k1_r3", F::Stream, 96, 1, with(t96, [](ConvArgs& a) { a.act = VGH_ACT_SILU; }), false);
    add("t: 3x3", "t128x96_w32x96_k1_r3", F::Stream, 96, 1, c96, false);
    // r tile: 96 input channels, stride 2, whole 8 x 8 output tiles
    const ConvArgs r32 = conv(3, 2, 2, 32, 32, 96, 96);
    add("r: 32 x 32 -> 16 x 16", "r8x8x96_n4", F::R, 96, 1, r32, true);
    add("r: 23 x 45 input", "r8x8x96_n4", F::R, 96, 1, conv(3, 2, 2, 23, 45, 96, 96), false);
    add("r: 64 input channels", "r8x8x96_n4", F::R, 96, 1, conv(3, 2, 2, 32, 32, 64, 96), false);
    add("r: residual", "r8x8x96_n4", F::R, 96, 1, with(r32, [](ConvArgs& a) { a.res = kSome, a.res_pitch = 96; }), false);
    add("r: cout_pad 192", "r8x8x96_n4", F::R, 96, 1, conv(3, 2, 2, 32, 32, 96, 192), true);
    add("r: cout_pad 288", "r8x8x96_n4", F::R, 96, 1, conv(3, 2, 2, 32, 32, 96, 288), false);
    // w tiles: cin = the tile's couts, stride 1, whole 8 x 8 tiles; a residual is fine
    add("w96: cin 96", "w8x8x96_n3", F::W, 96, 1, c96, true);
    add("w96: cin 64", "w8x8x96_n3", F::W, 96, 1, conv(3, 1, 2, 16, 16, 64, 96), false);
    add("w96: residual", "w8x8x96_n3", F::W, 96, 1, with(c96, [](ConvArgs& a) { a.res = kSome, a.res_pitch = 96; }), true);
    add("w128: cin 96, cout_pad 384", "w8x8x128_n4", F::W, 128, 1, conv(3, 1, 2, 16, 16, 96, 384), false);
    add("w96: cin 96, cout_pad 384", "w8x8x96_n3", F::W, 96, 1, conv(3, 1, 2, 16, 16, 96, 384), true);
    add("w96: 11 x 13 map", "w8x8x96_n3", F::W, 96, 1, conv(3, 1, 2, 11, 13, 96, 96), false);
    add("w128: cout_pad 1024", "w8x8x128_n4", F::W, 128, 1, conv(3, 1, 1, 8, 8, 128, 1024), true);
    add("w128: cout_pad 1152", "w8x8x128_n4", F::W, 128, 1, conv(3, 1, 1, 8, 8, 128, 1152), false);
#ifdef VGH_EXPERIMENTS  // the d tiles are rows of the experiments build's table only
    add("d: 3x3 / stride 2", "d4x16x96_n1x3", F::PatchS2, 96, 1, conv(3, 2, 2, 23, 45, 64, 96), true);
    add("d: stride 1", "d4x16x96_n1x3", F::PatchS2, 96, 1, c96, false);
#endif
    // the split table
    const ConvArgs s128 = with(c128, [](ConvArgs& a) { a.split = VGH_FMT_F16X2, a.nseg = 3, a.seg_kb = a.nkb, a.nkb *= 3; });
    add("split igemm: any conv", "split:s128x128_w64x64", F::SplitIgemm, 128, 1, with(s128, [](ConvArgs& a) { a.out_f32 = 1, a.fast_epi = 0; }), true);
    add("split patch: 3x3 / stride 1", "split:sp16x16x128_n4x2", F::SplitPatch, 128, 1, s128, true);
    add("split patch: fp32 output", "split:sp16x16x128_n4x2", F::SplitPatch, 128, 1, with(s128, [](ConvArgs& a) { a.out_f32 = 1; }), false);
    add("split KBS 2, no channel count", "split:s128x128_w64x64_k2_r2", F::SplitIgemm, 128, 2, with(s128, [](ConvArgs& a) { a.cblocks = 0; }), true);
    add("split KBS 4: 1x1, 2 channel blocks (4 k-blocks to the boundary)", nullptr, F::SplitIgemm, 128, 4, with(s128, [](ConvArgs& a) { a.ksize = 1, a.pad = 0, a.cblocks = 2; }), true);
    add("split KBS 4: 1x1, 3 channel blocks (6)", nullptr, F::SplitIgemm, 128, 4, with(s128, [](ConvArgs& a) { a.ksize = 1, a.pad = 0, a.cblocks = 3; }), false);
    add("split KBS 4: 3x3, 4 channel blocks (72)", nullptr, F::SplitPatch, 128, 4, s128, true);
    add("split KBS 3: 3x3, 4 channel blocks (72)", nullptr, F::SplitIgemm, 128, 3, s128, true);
    add("split KBS 3: 1x1, 4 channel blocks (8)", nullptr, F::SplitIgemm, 128, 3, with(s128, [](ConvArgs& a) { a.ksize = 1, a.pad = 0; }), false);
    add("split KBS 4, no channel count", nullptr, F::SplitIgemm, 128, 4, with(s128, [](ConvArgs& a) { a.cblocks = 0; }), false);
    add("fp16 g: single plane", "split:g8x8x128_n8", F::PingPongF16, 128, 1, fp16_single(c128), true);
    add("fp16 g: two planes", "split:g8x8x128_n8", F::PingPongF16, 128, 1, s128, false);
    add("fp16 g: bf16 planes", "split:g8x8x128_n8", F::PingPongF16, 128, 1, with(fp16_single(c128), [](ConvArgs& a) { a.split = VGH_FMT_BF16X2; }), false);
    add("fp16 g: ragged channels", "split:g8x8x128_n8", F::PingPongF16, 128, 1, with(fp16_single(c128), [](ConvArgs& a) { a.cout_store = 124; }), false);
    add("fp16 g: SiLU", "split:g8x8x128_n8", F::PingPongF16, 128, 1, with(fp16_single(c128), [](ConvArgs& a) { a.act = VGH_ACT_SILU; }), false);
    add("fp16 g96: cout_pad 128", "split:g8x8x96_n8", F::PingPongF16, 96, 1, fp16_single(c128), false);
    return n;
}

// vgh_conv_pp_fits at its four limits: the last admitted value and the first refused one
static void check_pp_fits() {
    const int64_t lim = (1ll << 31) - 4096;
    ConvArgs a = conv(3, 1, 1, 1, 1, 32, 32);  // one output pixel: the byte counts below are exact
    a.out_pitch = lim / 2 - 1;
    EXPECT(vgh_conv_pp_fits(a), "output: 2 bytes below the limit");
    a.out_pitch = lim / 2;
    EXPECT(!vgh_conv_pp_fits(a), "output: at the limit");
    a.out_fp8 = 1, a.out_pitch = lim - 1;
    EXPECT(vgh_conv_pp_fits(a), "e4m3 output: 1 byte below the limit");
    a.out_pitch = lim;
    EXPECT(!vgh_conv_pp_fits(a), "e4m3 output: at the limit");
    a = conv(3, 1, 1, 1, 1, 32, 32);
    a.res_pitch = lim / 2;  // no residual pointer: not read
    EXPECT(vgh_conv_pp_fits(a), "residual pitch without a residual");
    a.res = kSome;
    EXPECT(!vgh_conv_pp_fits(a), "residual: at the limit");
    a.res_pitch = lim / 2 - 1;
    EXPECT(vgh_conv_pp_fits(a), "residual: 2 bytes below the limit");
    a = conv(3, 1, 1, 4, 4096, 32, 32);
    a.in_pitch = 2047;
    EXPECT(vgh_conv_pp_fits(a), "input row: 8 KiB below 16 MiB");
    a.in_pitch = 2048;
    EXPECT(!vgh_conv_pp_fits(a), "input row: 16 MiB");
    // and through the rule, on a g tile: the whole batch counts (the only batch-dependent term of the rule)
    ConvArgs g = conv(3, 1, 256, 160, 160, 32, 128);  // 6 553 600 output pixels
    g.out_pitch = 160;                                // 2 097 152 000 bytes
    EXPECT(tile_admits(F::PingPongG, 128, 1, g), "g tile below 2 GiB");
    g.out_pitch = 168;  // 2 202 009 600
    EXPECT(!tile_admits(F::PingPongG, 128, 1, g) && tile_admits(F::Patch, 128, 1, g), "g tile above 2 GiB, p tile unaffected");
}

static void check_class_table() {
    struct Row { F f; int ksize, stride, epi16, max_cout_pad; };
    const Row rows[] = {{F::Igemm, 0, 0, 0, 0}, {F::Patch, 3, 1, 1, 0}, {F::PatchPipe, 3, 1, 1, 0}, {F::Stream, 1, 1, 1, 0}, {F::PatchS2, 3, 2, 1, 0}, {F::PingPongG, 3, 1, 1, 0}, {F::PingPongH, 3, 1, 1, 0},
                        {F::PingPongS, 3, 1, 1, 1024}, {F::R, 3, 2, 1, 192}, {F::W, 3, 1, 1, 1024}, {F::SplitIgemm, 0, 0, 0, 0}, {F::SplitPatch, 3, 1, 1, 0}, {F::PingPongF16, 3, 1, 1, 0}};
    static_assert(sizeof(rows) / sizeof(rows[0]) == kNumTileFamilies, "one row per family");
    for (const Row& r : rows) {
        const TileClass& c = kTileClass[(int)r.f];
        EXPECT(c.ksize == r.ksize && c.stride == r.stride && c.epi16 == r.epi16 && c.max_cout_pad == r.max_cout_pad, "class row of family %d", (int)r.f);
        // the row, as tile_class_admits reads it
        for (int ks = 1; ks <= 3; ks += 2)
            for (int st = 1; st <= 2; ++st)
                for (int epi = 0; epi <= 1; ++epi)
                    for (int sh = 0; sh <= 1; ++sh)
                        for (int cout = 96; cout <= 2304; cout += 96) {
                            const bool want = (!r.ksize || ks == r.ksize) && (!r.stride || st == r.stride) && (!r.epi16 || (epi && !sh)) && (!r.max_cout_pad || cout <= r.max_cout_pad);
                            EXPECT(tile_class_admits(r.f, 96, ks, st, cout, epi, sh) == want, "family %d k %d s %d epi %d shuffle %d cout_pad %d", (int)r.f, ks, st, epi, sh, cout);
                            EXPECT(!tile_class_admits(r.f, 128, ks, st, cout + 32, epi, sh) || (cout + 32) % 128 == 0, "cout tile of 128 at cout_pad %d", cout + 32);
                        }
    }
}

static void check_tile_grid() {
    struct Row { F f; int BP, BC, TW, TH, cout; bool whole; TileGrid want; };
    // a ragged 23 x 45 map, batch 3 (3 105 pixels); the r / w tiles admit whole 8 x 8 tiles only: 16 x 24
    const Row rows[] = {
        {F::Igemm, 128, 128, 0, 0, 384, false, {3, 0, 0, 75, 10}},       {F::Patch, 256, 128, 16, 16, 384, false, {3, 3, 2, 54, 7}},   {F::PatchPipe, 256, 96, 32, 8, 384, false, {4, 2, 3, 72, 9}},
        {F::Stream, 128, 192, 0, 0, 384, false, {2, 0, 0, 50, 7}},       {F::PatchS2, 64, 96, 16, 4, 384, false, {4, 3, 6, 216, 27}},  {F::PingPongG, 512, 128, 8, 8, 384, false, {3, 6, 3, 21, 3}},
        {F::PingPongH, 512, 96, 8, 8, 384, false, {4, 6, 3, 28, 4}},     {F::PingPongS, 512, 64, 8, 4, 384, false, {6, 6, 6, 42, 6}},  {F::R, 64, 96, 8, 8, 192, true, {2, 3, 2, 36, 5}},
        {F::W, 64, 128, 8, 8, 384, true, {3, 3, 2, 54, 7}},              {F::SplitIgemm, 64, 96, 0, 0, 384, false, {4, 0, 0, 196, 25}}, {F::SplitPatch, 320, 128, 40, 8, 384, false, {3, 2, 3, 54, 7}},
        {F::PingPongF16, 512, 96, 8, 8, 384, false, {4, 6, 3, 28, 4}},
    };
    static_assert(sizeof(rows) / sizeof(rows[0]) == kNumTileFamilies, "one map per family");
    for (const Row& r : rows) {
        ConvArgs a = r.whole ? conv(3, 1, 3, 16, 24, 96, r.cout) : conv(3, 1, 3, 23, 45, 96, r.cout);
        TileGrid g{-1, -1, -1, -1, -1};
        EXPECT(tile_grid(r.f, r.BP, r.BC, r.TW, r.TH, a, &g), "family %d", (int)r.f);
        EXPECT(g.ntc == r.want.ntc && g.ntx == r.want.ntx && g.nty == r.want.nty && g.total == r.want.total && g.chunk == r.want.chunk, "family %d: %d %d %d %d %d", (int)r.f, g.ntc, g.ntx, g.nty, g.total,
               g.chunk);
    }
    // output sizes, not input sizes: a stride-2 patch tile over a 23 x 45 input has a 12 x 23 output map
    TileGrid g{};
    EXPECT(tile_grid(F::PatchS2, 64, 96, 16, 4, conv(3, 2, 3, 23, 45, 96, 96), &g) && g.ntx == 2 && g.nty == 3 && g.total == 18, "stride-2 map: %d %d %d", g.ntx, g.nty, g.total);
    // the 2^30 refusal: 64 cout tiles x (2^24 - 1) pixel tiles = 2^30 - 64 items pass, one more pixel is 2^30
    ConvArgs big = conv(1, 1, 1, 1, 1, 32, 2048);
    big.P = 64 * ((1 << 24) - 1);
    EXPECT(tile_grid(F::Igemm, 64, 32, 0, 0, big, &g) && g.total == (1 << 30) - 64 && g.chunk == (1 << 27) - 8, "below 2^30: %d %d", g.total, g.chunk);
    big.P += 1;
    const TileGrid before = g;
    EXPECT(!tile_grid(F::Igemm, 64, 32, 0, 0, big, &g) && !memcmp(&g, &before, sizeof(g)), "2^30 items: refused, the grid untouched");
    static_assert(lds_bytes(128, 128, 64, 64, 1, 2) == 34816 && lds_bytes(128, 96, 32, 96, 1, 2) == 51200 && lds_bytes(128, 128, 64, 64, 1, 3) == 53248, "stage ring against epilogue strips");
}

int main() {
    static Case cases[128];
    const int n = make_cases(cases);
    for (int i = 0; i < n; ++i) EXPECT(tile_admits(cases[i].family, cases[i].BC, cases[i].KBS, cases[i].a) == cases[i].admitted, "%s: expected %d", cases[i].what, (int)cases[i].admitted);
    check_pp_fits();
    check_class_table();
    check_tile_grid();
    EXPECT(vgh_conv_b2b_ok(3, 2, 96, 192) && vgh_conv_b2b_ok(1, 1, 96, 256) && !vgh_conv_b2b_ok(3, 2, 128, 192) && !vgh_conv_b2b_ok(3, 2, 96, 64), "b2b pairs");
    printf("%d launch cases\n", n);
    if (failures) return 1;
    printf("conv_tiles host checks passed\n");
    return 0;
}
