// Which conv tile may run which convolution, and how many tiles a launch has: the ONE home of the admission rule of both tile tables (g_cfgs in conv_igemm.hip,
// g_scfgs in conv_split.hip).  Host logic on plain data: no HIP include, so tests/conv_tiles_host.hip checks it on its own under the host sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/vgh.h"
#include "conv_args.h"

// ---- activation storage formats (VGH_FMT_*, include/vgh.h) ----
static inline int vgh_fmt_bytes(int fmt) { return (fmt == VGH_FMT_FP8 || fmt == VGH_FMT_I8) ? 1 : (fmt == 0 || fmt == VGH_FMT_F16) ? 2 : 4; }  // bytes per logical element of an activation buffer
static inline int vgh_fmt_planes(int fmt) { return (fmt == VGH_FMT_BF16X2 || fmt == VGH_FMT_F16X2) ? 2 : 1; }
static inline int vgh_fmt_is_q8(int fmt) { return fmt == VGH_FMT_FP8 || fmt == VGH_FMT_I8; }    // an 8-bit link format
static inline int vgh_fmt_q8_kind(int fmt) { return fmt == VGH_FMT_FP8 ? 1 : fmt == VGH_FMT_I8 ? 2 : 0; }  // ConvArgs::in_fp8 / out_fp8 code

// One value per kernel family.  The bf16 table (conv_igemm.hip) holds the first ten, the split / fp16 table (conv_split.hip) the last three.
enum class TileFamily {
    Igemm,        // conv_igemm_kernel: implicit GEMM, any ksize / stride / epilogue (plain, deep-stage, counted-ring and loader-wave tiles)
    Patch,        // "p": conv3x3_patch_kernel, 3x3 / stride 1, halo patch of TH x TW output pixels
    PatchPipe,    // "q": conv3x3_patch3_kernel, the p tiles pipelined across tiles; stores whole cout tiles into ONE output segment (ragged channels run on the p twin)
    Stream,       // "t": conv1x1_stream_kernel, persistent streaming 1x1 / stride 1
    PatchS2,      // "d": conv3x3_patch_kernel stride 2 (output tile TH x TW), -DVGH_EXPERIMENTS builds only
    PingPongG,    // "g": conv3x3_pp_kernel (conv_pp.hip), 8 waves, an 8 x 8 sub-patch per wave, two barriers per tap; also the e4m3 / int8 links
    PingPongH,    // "h": the same with one barrier per tap
    PingPongS,    // "s": the g tile with two 4 x 8 sub-patches per wave
    R,            // "r": ds_conv_kernel (ds_b2b.hip), 3x3 / stride 2 with 96 input channels, weights resident in registers
    W,            // "w": w_conv_kernel (ds_b2b.hip), 3x3 / stride 1 with cin = the tile's 96 / 128 couts, weights resident in registers
    SplitIgemm,   // conv_igemm_kernel<..., SP>: two-plane (or single-plane fp16) implicit GEMM
    SplitPatch,   // conv3x3_patch_kernel<..., SP>
    PingPongF16,  // the g tile in its single-plane fp16 variant (VGH_FMT_F16 nets)
};
constexpr int kNumTileFamilies = (int)TileFamily::PingPongF16 + 1;

// ---- the class-level rule: what a family asks of (ksize, stride, epilogue, cout_pad), one row per family in the order of the enum ----
struct TileClass {
    int ksize, stride;  // required value, 0 = any
    int epi16;          // 1: needs the LDS-transposed 16-byte epilogue of a 16-bit output (ConvArgs::fast_epi && !out_f32) and no pixel-shuffle store
    int max_cout_pad;   // largest cout_pad, 0 = no limit of the family's own
};
constexpr TileClass kTileClass[kNumTileFamilies] = {
    {0, 0, 0, 0},     // Igemm
    {3, 1, 1, 0},     // Patch
    {3, 1, 1, 0},     // PatchPipe
    {1, 1, 1, 0},     // Stream
    {3, 2, 1, 0},     // PatchS2
    {3, 1, 1, 0},     // PingPongG
    {3, 1, 1, 0},     // PingPongH
    {3, 1, 1, 1024},  // PingPongS: 4-KB bias vector
    {3, 2, 1, 192},   // R
    {3, 1, 1, 1024},  // W
    {0, 0, 0, 0},     // SplitIgemm
    {3, 1, 1, 0},     // SplitPatch
    {3, 1, 1, 0},     // PingPongF16
};
inline bool tile_class_admits(TileFamily f, int BC, int ksize, int stride, int cout_pad, int epi16, int shuffle) {
    const TileClass& c = kTileClass[(int)f];
    if (cout_pad % BC) return false;
    if (c.ksize && ksize != c.ksize) return false;
    if (c.stride && stride != c.stride) return false;
    if (c.epi16 && !(epi16 && !shuffle)) return false;
    return !(c.max_cout_pad && cout_pad > c.max_cout_pad);
}

// ---- the summation chain of a family's bf16 3x3 / stride-1 tiles: what decides every bit of an output element.  All of them issue v_mfma_f32_32x32x16_bf16 with the
//      weights as A and the pixels as B, one 32-channel block of one tap per pair of MFMAs; they differ in the order of those pairs and in where the bias enters.
//      The survivor kernel of postproc.hip walks the same chain for a single pixel (an output element depends on its own weight row and pixel column only). ----
struct ChainTrait {
    int known;       // 0: the chain of this family is not reproduced anywhere else -- its ops always run densely
    int tap_major;   // 1: k-blocks in packed-weight order, tap-major over ascending channel blocks; 0: channel-block-major with the nine taps (ky, then kx) inside
    int bias_first;  // 1: the accumulator starts at the bias; 0: it starts at zero and the bias is added in fp32 afterwards
};  // (in every family lane half `hi` of MFMA h = 0 / 1 of a 32-channel block holds channels 8 (2 h + hi) .. + 7: nothing to record)
constexpr ChainTrait kChainTrait[kNumTileFamilies] = {
    {1, 1, 0},  // Igemm (conv_kernels.inc, stage_load: channel block fastest, then kx, then ky; k-blocks past the end are zeros)
    {1, 0, 0},  // Patch (conv3x3_patch_kernel: steps (cb, ky), sub-steps (kx, h); bias in the epilogue)
    {1, 0, 1},  // PatchPipe (conv3x3_patch3_kernel: the same steps, the bias as the C input of the first MFMA)
    {0, 0, 0},  // Stream (1x1 only)
    {0, 0, 0},  // PatchS2
    {1, 0, 1},  // PingPongG (conv_pp.hip: for cb, for tap, two MFMAs; PP_INIT_ROWS)
    {1, 0, 1},  // PingPongH
    {1, 0, 1},  // PingPongS (pixels of an overlap column are computed twice with the same chain)
    {0, 0, 0},  // R
    {0, 0, 0},  // W
    {0, 0, 0},  // SplitIgemm
    {0, 0, 0},  // SplitPatch
    {0, 0, 0},  // PingPongF16
};
// the chain as one small code for the survivor kernel: -1 unknown, else bit 0 = tap_major, bit 1 = bias_first
inline int chain_code(TileFamily f) {
    const ChainTrait& c = kChainTrait[(int)f];
    return c.known ? (c.tap_major | (c.bias_first << 1)) : -1;
}

// ---- launch-level predicates of single families (`a` prepared) ----
// the ping-pong tiles' epilogue addresses the output and residual tensors through buffer descriptors: 32-bit byte offsets
inline int vgh_conv_pp_fits(const ConvArgs& a) {
    const int64_t lim = (1ll << 31) - 4096;
    return (int64_t)a.P * a.out_pitch * (a.out_fp8 ? 1 : 2) < lim && (!a.res || (int64_t)a.P * a.res_pitch * 2 < lim) && a.cout_pad <= 2048 &&
           (int64_t)a.W * a.in_pitch * 2 < (1 << 24);  // one input row in 24 bits: the halo offsets are 24-bit multiply-adds
}

// back-to-back GEMM (conv_kernels.inc, T2 > 0): a conv whose 96 output channels fit ONE cout tile, fused with the 1x1 conv that is its only reader
inline int vgh_conv_b2b_ok(int ksize, int stride, int cout_pad, int cout2_pad) {
    (void)stride;
    return (ksize == 1 || ksize == 3) && cout_pad == 96 && (cout2_pad == 256 || cout2_pad == 192 || cout2_pad == 128);
}

// ("t" tile of ds_b2b.hip) the pair a (3x3 / stride 2 / pad 1, 48 real input channels at a 48-channel pitch declared as cin = 64, 96 couts) -> 1x1 with 128 / 192 couts, on a map of whole 8 x 8 tiles
inline int vgh_conv_ds_b2b_ok(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 2 && a.pad == 1 && a.cin == 64 && a.in_pitch == 48 && a.in_coff % 8 == 0 && a.cout_pad == 96 && a.cout_store == 96 && (a.cout2_pad == 128 || a.cout2_pad == 192) && a.cout2_store == a.cout2_pad &&
           a.H == 2 * a.Ho && a.W == 2 * a.Wo && a.Ho % 8 == 0 && a.Wo % 8 == 0 && (int64_t)a.W * a.in_pitch * 2 * 20 < (1ll << 30) && !a.split && !a.res && !a.shuffle && !a.grp_cout &&
           !a.in_fp8 && !a.out_fp8 && !a.out_f32 && a.act != VGH_ACT_SILU && a.act2 != VGH_ACT_SILU;
}

// plain 3x3 / stride-2 / pad-1 conv, 96 input channels, whole 96-cout workgroup tiles, a map of whole 8 x 8 tiles ("r" tile)
inline int vgh_conv_ds_ok(const ConvArgs& a) {
    return a.ksize == 3 && a.stride == 2 && a.pad == 1 && a.cin == 96 && a.in_pitch % 8 == 0 && a.in_pitch >= 96 && a.in_coff % 8 == 0 && a.cout_pad % 96 == 0 && a.cout_pad <= 192 &&
           a.cout_store == a.cout_pad && (a.out_split >= a.cout_pad || a.out_split % 16 == 0) && a.out_coff % 8 == 0 && a.out_coff2 % 8 == 0 && a.out_pitch % 8 == 0 && a.H == 2 * a.Ho &&
           a.W == 2 * a.Wo && a.Ho % 8 == 0 && a.Wo % 8 == 0 && (int64_t)a.W * a.in_pitch * 2 * 20 < (1ll << 30) && (int64_t)a.Wo * a.out_pitch * 2 * 9 < (1ll << 30) && !a.split && !a.res &&
           !a.shuffle && !a.grp_cout && !a.in_fp8 && !a.out_fp8 && !a.out_f32 && a.act != VGH_ACT_SILU && !a.w2pack;
}

// 3x3 / stride-1 / pad-1 conv with 96 (-> cout_pad a multiple of 96) or 128 (-> a multiple of 128) input channels on a map of whole 8 x 8 tiles ("w" tile)
inline int vgh_conv_w_ok(const ConvArgs& a) {
    const int ncg = a.cin == 96 ? 3 : a.cin == 128 ? 4 : 0;
    return ncg && a.ksize == 3 && a.stride == 1 && a.pad == 1 && a.in_pitch % 8 == 0 && a.in_coff % 8 == 0 && a.cout_pad % (32 * ncg) == 0 && a.cout_pad <= 1024 && a.cout_store == a.cout_pad &&
           (a.out_split >= a.cout_pad || a.out_split % 16 == 0) && a.out_coff % 8 == 0 && a.out_coff2 % 8 == 0 && a.out_pitch % 8 == 0 && a.Ho == a.H && a.Wo == a.W && a.H % 8 == 0 && a.W % 8 == 0 &&
           (int64_t)a.W * a.in_pitch * 2 * 12 < (1ll << 30) && (int64_t)a.Wo * a.out_pitch * 2 * 9 < (1ll << 30) && (!a.res || ((int64_t)a.Wo * a.res_pitch * 2 * 9 < (1ll << 30) && a.res_pitch % 4 == 0 && a.res_coff % 4 == 0)) &&
           !a.split && !a.shuffle && !a.grp_cout && !a.in_fp8 && !a.out_fp8 && !a.out_f32 && a.act != VGH_ACT_SILU && !a.w2pack;
}

// "dense 16-bit -> 16-bit, ReLU or none": shared by the ping-pong tiles (bf16 and fp16) and the streaming tiles.  The r / w / t predicates above spell out their
// own longer lists (the w tile takes a residual, the r tile does not), and nothing else is shared word for word.
inline bool dense_relu_16bit(const ConvArgs& a) { return !a.grp_cout && a.act != VGH_ACT_SILU && !a.out_f32; }

// ---- the launch-level rule, for both tables: can a tile of family `f` with BC couts per tile (and, split implicit-GEMM / patch tiles, KBS k-blocks per stage)
//      run the PREPARED launch `a`?  The only batch-dependent term is the ping-pong tiles' 2 GiB rule (vgh_conv_pp_fits). ----
inline bool tile_admits(TileFamily f, int BC, int KBS, const ConvArgs& a) {
    if (!tile_class_admits(f, BC, a.ksize, a.stride, a.cout_pad, a.fast_epi && !a.out_f32, a.shuffle)) return false;
    if (a.grp_cout && a.grp_cout % BC) return false;  // a grouped conv needs cout tiles that do not straddle groups
    switch (f) {
        case TileFamily::SplitIgemm:
        case TileFamily::SplitPatch:
            // the accumulators are rescaled between two steps of the K loop: the boundary (2 x the k-blocks of a segment) must fall on a step.  The
            // ABI-level query has no channel count (cblocks = 0): there only KBS <= 2 is promised, which every segment length satisfies
            return !(KBS > 2 && (a.cblocks == 0 || (2 * a.ksize * a.ksize * a.cblocks) % KBS));
        case TileFamily::PingPongF16:  // single-plane fp16 nets only, whole cout tiles
            return a.nseg == 1 && a.split == VGH_FMT_F16X2 && dense_relu_16bit(a) && a.cout_store == a.cout_pad && vgh_conv_pp_fits(a);
        default: break;
    }
    // the bf16 table
    if ((a.in_fp8 || a.out_fp8) && f != TileFamily::PingPongG) return false;  // e4m3 / int8 links: g tiles only (conv_pp.hip)
    if (a.dvec && BC == 128) return false;  // the 128-cout variant of the diagonal bypass spills: 96 or 64 couts per workgroup there
    switch (f) {
        case TileFamily::PingPongS:
            if (a.Wo < 8 || a.Ho < 4) return false;  // 4 x 8 sub-patches are moved back inside the map, never cut
            [[fallthrough]];
        case TileFamily::PingPongG:
        case TileFamily::PingPongH: return dense_relu_16bit(a) && vgh_conv_pp_fits(a);
        case TileFamily::Stream: return dense_relu_16bit(a) && !a.res && !a.pad;  // plain bf16 -> bf16 only
        case TileFamily::R: return vgh_conv_ds_ok(a);                            // 96 input channels, whole 8 x 8 tiles
        case TileFamily::W: return vgh_conv_w_ok(a) && a.cin == BC;              // cin = the tile's 96 / 128, whole 8 x 8 tiles
        default: return true;
    }
}

// ---- tile counts of a launch: the only place that computes them ----
struct TileGrid {
    int ntc;       // cout tiles
    int ntx, nty;  // tiles (ping-pong families: sub-patches) across and down one map; 0 for the pixel-linear families
    int total;     // work items of the launch
    int chunk;     // items per XCD: ceil(total / 8)
};
// BP: pixels per tile of the pixel-linear families; TW x TH: the output tile (sub-patch) of the others.  Output sizes (Ho, Wo) throughout: both callers of the conv
// launchers (net.hip's executor and vgh_conv_run) set pad = ksize / 2, so Ho = H and Wo = W for every 3x3 / stride-1 launch, which is all the halo-patch tiles admit.
// false: 2^30 work items or more (the kernels' index arithmetic is 32-bit) -- the caller refuses the launch.
inline bool tile_grid(TileFamily f, int BP, int BC, int TW, int TH, const ConvArgs& a, TileGrid* g) {
    const int ntc = a.cout_pad / BC;
    int ntx = 0, nty = 0;
    int64_t total;
    switch (f) {
        case TileFamily::Igemm:
        case TileFamily::Stream:
        case TileFamily::SplitIgemm: total = (((int64_t)a.P + BP - 1) / BP) * ntc; break;
        case TileFamily::PingPongG:
        case TileFamily::PingPongH:
        case TileFamily::PingPongS:
        case TileFamily::PingPongF16: {  // a workgroup takes 8 sub-patches of 8 x 8 pixels (s tiles: 16 of 4 x 8), ragged ones included
            ntx = (a.Wo + TW - 1) / TW, nty = (a.Ho + TH - 1) / TH;
            const int per_wg = BP / (TW * TH);
            total = ((int64_t)a.B * nty * ntx + per_wg - 1) / per_wg * ntc;
            break;
        }
        default:  // halo-patch tiles, ragged at the right and bottom edges; r / w tiles, whole 8 x 8 tiles only (tile_admits)
            ntx = (a.Wo + TW - 1) / TW, nty = (a.Ho + TH - 1) / TH;
            total = (int64_t)a.B * nty * ntx * ntc;
    }
    if (total >= (1ll << 30)) return false;
    *g = TileGrid{ntc, ntx, nty, (int)total, (int)((total + 7) / 8)};
    return true;
}

// dynamic LDS of an implicit-GEMM tile: its stage ring (+ the counted rings' per-wave slots), or the LDS-transposed epilogue strips where those are larger
constexpr int lds_bytes(int BP, int BC, int WP, int WC, int KBS, int NST) {
    const int nw = (BP / WP) * (BC / WC);
    const int loop = NST * KBS * (BP + BC) * 64 + (NST > 2 ? nw * 1024 : 0), epi = nw * 32 * (WC + 4) * 4;
    return loop > epi ? loop : epi;
}
