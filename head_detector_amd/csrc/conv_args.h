// The conv launch descriptor shared by the kernels, the launchers and the tile rules (conv_tiles.h).  Plain data: no HIP type, so host-only code can include it.
#pragma once
#include <stdint.h>

// ---- conv launch descriptor (device pointers resolved) ---------------------------------
struct ConvArgs {
    const uint16_t* in;    // bf16 NHWC, pixel pitch in_pitch elements, first channel in_coff
    const uint16_t* wpack; // packed weights [nkb][cout_pad][32] bf16, 16B chunks pre-swizzled
    const float* bias;     // [cout_pad]
    void* out;             // bf16 (or f32 when out_f32) NHWC
    const uint16_t* res;   // residual, same spatial dims as out (or nullptr)
    const uint16_t* zeros; // >= 64 B of zeros (im2col padding source)
    int64_t in_pitch, out_pitch, res_pitch;
    int in_coff, out_coff, out_coff2, out_split, res_coff;
    int B, H, W, Ho, Wo;
    int cin;        // multiple of 32
    int cout_pad;   // rows in wpack (multiple of 32)
    int cout_store; // channels actually written (<= cout_pad)
    int ksize, stride, pad;
    int act;        // VGH_ACT_*
    int out_f32;    // 1: write float
    int shuffle;    // 1: ConvTranspose2d(k=2,s=2) pixel-shuffle store, cout_pad = 4*C
    int shuffle_c;  // C of the transposed conv
    float alpha;    // residual scale
    int P;          // B*Ho*Wo output pixels
    int nkb;        // ksize*ksize*cin/32
    int cblocks;    // cin/32
    unsigned div_howo_m, div_howo_s, div_wo_m, div_wo_s;  // n / d == (umulhi(n, m) + n) >> s for n < 2^30 (filled by vgh_launch_conv)
    int fast_epi;   // 1: LDS-transposed 16-byte epilogue (bf16 out, 8-channel aligned offsets)
    int stagger;    // persistent patch kernels: odd resident-slot blocks start this many ~0.5 us sleeps late (de-phases co-resident blocks)
    int grid_share; // persistent patch kernels: take 1/grid_share of the CU slots (the executor's other lane streams own the rest)
    // ---- grouped convolution (block-diagonal launch of sibling branches): cout tile c0 belongs to group c0 / grp_cout and reads its
    //      input channels at in_coff + group * grp_in_stride; every row of wpack holds that group's cin = a.cin channels ----
    int grp_cout, grp_in_stride;  // 0: dense
    // ---- split-precision parity modes (conv_split.hip): activations are two 16-bit planes per pixel [hi C | lo C] and the K loop runs
    //      three segments x_hi*w_lo, x_lo*w_hi (corrections), then -- after one multiply of the accumulators by acc_scale -- x_hi*w_hi ----
    int split;        // VGH_FMT_BF16 (0): plain; VGH_FMT_BF16X2 / VGH_FMT_F16X2: hi|lo planes
    int in_plane, out_plane, res_plane;  // elements from a pixel's hi plane to its lo plane (the buffer's logical pitch)
    int seg_kb;       // k-blocks per segment = ksize^2 * cblocks (nkb = nseg * seg_kb)
    int nseg;         // 3: the split modes' x_hi*w_lo, x_lo*w_hi, x_hi*w_hi; 1: the single-plane fp16 format (VGH_FMT_F16, r05) rides the F16X2 kernels with its one
                      //    plane as "hi" (split = VGH_FMT_F16X2, in/out/res_plane = 0, acc_scale = 0: no lo plane is read or written) and the [w_hi] weight image
    float acc_scale;  // 1/2048 (fp16: lo planes are stored scaled by 2^11) or 1 (bf16)
    float lo_scale;   // lo = (v - hi) * lo_scale
    float out_scale;  // undoes the per-op power-of-two weight prescale (fp16), applied to the accumulator before the bias
    // ---- e4m3 links (conv_pp.hip, r05): the input view / the output tensor hold OCP e4m3 bytes (pitches and channel offsets then count bytes); the residual stays
    //      bf16.  gscale[cout_pad]: per-cout output factor applied to the accumulator (which starts at bias / gscale when the input is e4m3) ----
    //      in_fp8 / out_fp8: 0 = 16-bit, 1 = e4m3, 2 = int8 (VGH_FMT_I8: the `bias` vector of an int8-INPUT conv holds int32 BIT PATTERNS in accumulator units,
    //      rn(bias[c] / (wscale[c] * scale(in))); the int32 accumulator starts there and out = act(float(acc) * gscale[c]) -- include/vgh.h, conv_pp.hip PP_INIT_ROWS) ----
    int in_fp8, out_fp8;
    const float* gscale;
    const float* dvec;  // int8 -> bf16 only (or nullptr): the diagonal bypass, out[c] += dvec[c] * code(input pixel, channel c) before the activation (conv_pp.hip DG)
    float bias_scale;  // fp16 ping-pong variant: 1 / out_scale (set by vgh_launch_conv_pp)
    int fallback_cfg1;  // 0: a forced tile that cannot run this conv is an error; k + 1: it falls back to tile k (network executor: a table may be stale)
    int nt_out;          // bf16 output stores carry the non-temporal hint (set by vgh_conv_prepare from vgh_conv_set_nt_store)
    // ---- back-to-back GEMM (r06, conv_kernels.inc T2 > 0): this conv's output tile feeds a 1x1 / stride-1 conv inside the same launch; only that conv's output is stored ----
    const uint16_t* w2pack;  // the second conv's packed weights [cout_pad / 32][cout2_pad][32] (vgh_pack_conv_weights_host), or nullptr
    const float* bias2;      // [cout2_pad]
    void* out2;              // the second conv's output tensor (bf16 NHWC), pitch / offsets / split / stored channels as for `out`
    int64_t out2_pitch;
    int out2_coff, out2_coff2, out2_split, cout2_pad, cout2_store, act2;
    int b2b_igemm;           // 1: keep the pair on the implicit-GEMM b2b tile even where the persistent t tile (ds_b2b.hip) could run it (vgh_net_set_b2b(n, 2): A/B, tests)
    int ablate;     // -DVGH_EXPERIMENTS builds only: bit0 skip tile loads, bit1 skip MFMAs, bit3 skip the epilogue (results are garbage)
    unsigned long long* trace;  // -DVGH_EXPERIMENTS builds only: per-(block, tile) phase timestamps (s_memtime), or nullptr
};
