// Internal declarations shared by the libvgh.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vgh.h"
#include "conv_tiles.h"  // ConvArgs (conv_args.h), the tile families and their admission rule

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

// ---- error plumbing: never throw across the C ABI --------------------------------------
void vgh_set_error(const char* fmt, ...);

#define VGH_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            vgh_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return VGH_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

#define VGH_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            vgh_set_error(__VA_ARGS__);   \
            return VGH_ERR_INVALID;       \
        }                                 \
    } while (0)

#define VGH_TRACE_TILES 16  // tiles recorded per block
#define VGH_TRACE_MARKS 4   // marks per tile: tile top, operands landed, K loop done, epilogue done

// Work-skipping switches exist only in the experiments build (tools/, never the shipped libvgh.so)
#ifdef VGH_EXPERIMENTS
#define VGH_ABLATE(a, bit) ((a).ablate & (bit))
#define VGH_MARK(a, tile_no, k)                                                                                                      \
    do {                                                                                                                             \
        if ((a).trace && threadIdx.x == 0 && (tile_no) < VGH_TRACE_TILES)                                                            \
            (a).trace[((size_t)blockIdx.x * VGH_TRACE_TILES + (tile_no)) * VGH_TRACE_MARKS + (k)] = __builtin_amdgcn_s_memtime();   \
    } while (0)
// one tile per block (the implicit-GEMM kernel): row = blockIdx.x, tile 0; the tool's buffer holds 8192 rows
#define VGH_MARK_BLOCK(a, k)                                                                                                  \
    do {                                                                                                                      \
        if ((a).trace && threadIdx.x == 0 && blockIdx.x < 8192)                                                               \
            (a).trace[((size_t)blockIdx.x * VGH_TRACE_TILES) * VGH_TRACE_MARKS + (k)] = __builtin_amdgcn_s_memtime();        \
    } while (0)
struct VghMarkAtExit {  // "epilogue done" on every return path of a kernel body
    unsigned long long* t;
    __device__ ~VghMarkAtExit() {
        if (t && threadIdx.x == 0 && blockIdx.x < 8192) t[((size_t)blockIdx.x * VGH_TRACE_TILES) * VGH_TRACE_MARKS + 3] = __builtin_amdgcn_s_memtime();
    }
};
#define VGH_MARK_EXIT(a) VghMarkAtExit vgh_mark_at_exit_{(a).trace}
#else
#define VGH_ABLATE(a, bit) 0
#define VGH_MARK(a, tile_no, k) \
    do {                        \
    } while (0)
#define VGH_MARK_BLOCK(a, k) \
    do {                     \
    } while (0)
#define VGH_MARK_EXIT(a) \
    do {                 \
    } while (0)
#endif

// postproc.hip (r06): vgh_nms + vgh_compact + the detector's head list as ONE launch (block per image; the last block to finish builds the head list; head_row_dev may be
// null: no head list).  ticket_dev: one zero-initialised int32 the kernel leaves at zero.
int vgh_nms_select(const float* boxes_dev, const float* scores_dev, const float* flame_dev, int B, int n_in, float conf_thr, float iou_thr, int keep_k,
                   int32_t* keep_idx_dev, int32_t* counts_dev, float* out_boxes_dev, float* out_scores_dev, float* out_flame_dev, int capacity, int32_t* head_row_dev,
                   int32_t* head_image_dev, int32_t* n_heads_dev, int32_t* ticket_dev, const vgh_head_level* lazy_levels, int n_levels, const int32_t* lazy_idx_dev,
                   int shape_c, int expr_c, void* stream,   // lazy_idx_dev != null: flame_dev is not read, the survivors' vectors come from the prediction buffers
                   int rows_later = 0);                     // 1: the survivors' vectors are left to vgh_survivor_rows, queued behind this launch (rows past the count are still zeroed)
int vgh_launch_conv(const ConvArgs& a, int force_cfg, hipStream_t stream);
// the ONE launcher type of both tile tables (conv_igemm.hip, conv_split.hip): the prepared launch, its tile counts (tile_grid), the dynamic LDS of the table row, the stream
#define VGH_TILE_LAUNCHER(name) int name(const ConvArgs& a, const TileGrid& g, int lds, hipStream_t st)
// conv_igemm.hip: `a` with its b2b fields set (w2pack ...): the fused launch, or VGH_ERR_INVALID when the pair does not fit a b2b tile (vgh_conv_b2b_ok says so beforehand)
int vgh_launch_conv_b2b(const ConvArgs& a, hipStream_t stream);
// ds_b2b.hip ("t" tile): the stage-1 downsample + conv1|conv2 pair as one persistent launch with register-resident weights; `a` prepared, b2b fields set
int vgh_launch_conv_ds_b2b(const ConvArgs& a, hipStream_t stream);
// ("r" tile) a plain 3x3 / stride-2 conv with 96 input channels in the same execution structure; `a` prepared, `g` its tile_grid
int vgh_launch_conv_ds(const ConvArgs& a, const TileGrid& g, hipStream_t stream);
// ("w" tile) 3x3 / stride-1 convs with 96 / 128 input channels, weights resident in registers; `a` prepared, `g` its tile_grid
int vgh_launch_conv_w(const ConvArgs& a, const TileGrid& g, hipStream_t stream);
// ("u" tile) the same with the stem conv in the launch: u8 NHWC images in, the stem tensor never exists; `a` = the pair (b2b fields set, not yet prepared)
int vgh_launch_stem_ds_b2b(const ConvArgs& a, const void* image_u8, int Hi, int Wi, const float* wstem, const float* bstem, hipStream_t stream);
int vgh_launch_conv_split(const ConvArgs& a, int force_cfg, hipStream_t stream);  // conv_split.hip: a.split = VGH_FMT_BF16X2 / VGH_FMT_F16X2
// dense [cout_pad][ks][ks][cin] f32 -> the three-segment 16-bit image [w_lo | w_hi | w_hi] (each segment laid out like
// vgh_pack_conv_weights_host); fmt = VGH_FMT_BF16X2 / VGH_FMT_F16X2.  Returns through *out_scale the factor the kernel multiplies the
// accumulators by (fp16: 2^-s with 2^s the power-of-two prescale that brings max|w| to ~2^9; bf16: 1).
void vgh_pack_conv_weights_split_host(const float* w, int cout_pad, int ksize, int cin, int fmt, uint16_t* dst, float* out_scale);
// conv_pp.hip (host): OCP e4m3fn conversion and the e4m3 weight image of the ping-pong tiles
uint8_t vgh_f32_to_e4m3_host(float f);
void vgh_pack_conv_weights_fp8_host(const float* w, int cout_pad, int ksize, int cin, uint8_t* dst, float* wscale);
void vgh_pack_conv_weights_i8_host(const float* w, int cout_pad, int ksize, int cin, uint8_t* dst, float* wscale);
// conv_pp.hip: the 8-wave ping-pong 3x3 / stride-1 tiles (family PingPongG / H / S, or PingPongF16; bc = 128 / 96 / 64 couts per workgroup); `a` prepared, `g` its tile_grid
int vgh_launch_conv_pp(const ConvArgs& a, TileFamily family, int bc, const TileGrid& g, int max_blocks_per_xcd, hipStream_t stream);
int vgh_conv_pp_lds(int bc);
int vgh_conv_max_blocks_per_xcd();  // the process-wide cap of vgh_conv_set_max_blocks_per_xcd (0 = none)
int vgh_conv_persistent_blocks_per_xcd(const ConvArgs& a, int chunk, int blocks_per_cu);
int vgh_conv_pick_cfg(const ConvArgs& a);
int vgh_conv_cfg_ok_for(int cfg, const ConvArgs& a);  // `a` prepared; bf16 tiles only (split launches validate in conv_split.hip)
// validates `a` and fills its derived fields (fast-division constants, fast_epi); vgh_launch_conv calls it itself
int vgh_conv_prepare(ConvArgs& a);
// automatic tile of a PREPARED descriptor: index into the bf16 table (a.split == 0) or into conv_split.hip's table
int vgh_conv_pick_auto(const ConvArgs& a);
int vgh_conv_split_pick(const ConvArgs& a);
// the summation chain (conv_tiles.h, chain_code) of the tile that vgh_launch_conv(a, force_cfg) runs this bf16 conv on; -1: a family whose chain nothing else reproduces
int vgh_conv_chain(const ConvArgs& a, int force_cfg);
// host-side weight packing: dense [cout_pad][ks][ks][cin] f32 -> wpack bf16 image
void vgh_pack_conv_weights_host(const float* w, int cout_pad, int ksize, int cin, uint16_t* dst);
// the packing loop of every 16-bit weight image: dense [cout_pad][ks][ks][cin] -> dst[kb][cout][slot][8] with slot = chunk ^ ((cout>>2)&3), kb = (ky*ks + kx)*(cin/32) + cb,
// every element through `cvt` (fp32 -> bf16 for vgh_pack_conv_weights_host, the identity for conv_split.hip's planes that are 16-bit already)
template <class Src, class Cvt>
static inline void vgh_pack_conv_image(const Src* w, int cout_pad, int ksize, int cin, uint16_t* dst, Cvt cvt) {
    const int cblocks = cin / 32, taps = ksize * ksize;
    for (int tap = 0; tap < taps; ++tap)
        for (int cb = 0; cb < cblocks; ++cb) {
            const int kb = tap * cblocks + cb;
            for (int co = 0; co < cout_pad; ++co) {
                const Src* src = w + ((size_t)co * taps + tap) * cin + cb * 32;
                uint16_t* d = dst + ((size_t)kb * cout_pad + co) * 32;
                const int sw = (co >> 2) & 3;
                for (int chunk = 0; chunk < 4; ++chunk) {
                    const int slot = chunk ^ sw;
                    for (int e = 0; e < 8; ++e) d[slot * 8 + e] = cvt(src[chunk * 8 + e]);
                }
            }
        }
}
static inline size_t vgh_wpack_elems(int cout_pad, int ksize, int cin) { return (size_t)cout_pad * ksize * ksize * cin; }

static inline void vgh_fastdiv_magic(unsigned d, unsigned* m, unsigned* s) {
    unsigned sh = 0;
    while ((1ull << sh) < d) ++sh;
    *m = (unsigned)((((1ull << 32) * ((1ull << sh) - d)) / d) + 1);
    *s = sh;
}

static inline uint16_t vgh_f32_to_bf16_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40); // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ---- other launchers --------------------------------------------------------------------
// fmt / plane: VGH_FMT_BF16 (plane unused) or a split format: then out_pitch is the physical pitch and `plane` the elements from hi to lo
int vgh_launch_stem(const void* image, int image_fmt, int B, int H, int W, const float* w /*[64][27] dev*/,
                    const float* bias /*[64] dev*/, uint16_t* out, int64_t out_pitch, int out_coff, int store_ch /*64, or 48 (bf16 only)*/, int fmt, int plane,
                    hipStream_t stream);
// stem_ds.hip: stem + stage-1 downsample in one kernel (bit-identical to vgh_launch_stem + the 3x3 / stride-2 / 64 -> 96 implicit-GEMM conv)
int vgh_launch_stem_ds(const void* image, int image_fmt, int B, int H, int W, const float* wstem, const float* bstem, const uint16_t* wds, const float* bds, uint16_t* out,
                       int64_t out_pitch, int out_coff, hipStream_t stream);
void vgh_pack_stem_ds_weights_host(const float* w /*[96][3][3][64]*/, uint16_t* dst /*[9][3][96][16]*/);
int vgh_launch_conv_f32(const ConvArgs& a, const float* wdense, hipStream_t stream);
int vgh_launch_stem_f32(const void* image, int image_fmt, int B, int H, int W, const float* w, const float* bias, float* out, int64_t out_pitch, int out_coff,
                        hipStream_t stream);
int vgh_launch_spp_pool_f32(float* buf, int64_t pitch, int coff, int C, int B, int H, int W, hipStream_t stream);
int vgh_launch_spp_pool(uint16_t* buf, int64_t pitch, int coff, int C, int B, int H, int W, int fmt, int plane, hipStream_t stream);

// streams.hip: a stream MEASURED to run side by side with every stream in `avoid` (earlier entries matter more when the hardware
// queues do not suffice for all of them); released streams are parked, never destroyed
int vgh_stream_acquire_internal(int device, const hipStream_t* avoid, int n_avoid, hipStream_t* out, bool low_priority = false);
void vgh_stream_release_internal(int device, hipStream_t s, bool low_priority = false);
struct vgh_net;
// net.hip: the net's lane streams for work entering on `main` (picked on first use, re-picked when `main` changes); out[3]
int vgh_net_lane_streams(vgh_net* n, hipStream_t main, hipStream_t* out);
extern "C" __attribute__((visibility("hidden"))) int vgh_net_device(vgh_net* n);  // library-internal
// net.hip, library-internal since r06 (was exported): the first op of the next forwards that writes a prediction buffer waits for `event` (or nullptr) on its stream
extern "C" __attribute__((visibility("hidden"))) int vgh_net_set_pred_guard(vgh_net* n, void* event);
// net.hip, library-internal: how many forwards (vgh_net_forward, vgh_net_forward_graph, vgh_net_profile) have been queued on this net -- the prediction buffers hold the
// results of the latest one.  The detector's lazy FLAME gather is tied to the generation it decoded (detect.hip)
extern "C" __attribute__((visibility("hidden"))) uint64_t vgh_net_generation(vgh_net* n);
// One deferrable prediction conv (NetPlan::Op::deferrable) as the survivor-row kernel of postproc.hip needs it: row p of the op's output is
// act(W . in[p * in_pitch + in_coff ...] + bias), channels [0, cout_store) of it landing at channel out_coff of the prediction row.
struct vgh_row_op {
    const uint16_t* in;     // bf16 input tensor, batch row 0
    const uint16_t* wpack;  // packed weights (vgh_pack_conv_weights_host), [cblocks][cout_pad][32]
    const float* bias;      // [cout_pad]
    int in_pitch, in_coff, cblocks, cout_pad, cout_store, out_coff, act;
};
constexpr int kMaxRowOps = 4;  // per prediction buffer
// net.hip, library-internal (the exported ABI is frozen): the defer switch (default off: forwards run every op), the pending convs of the latest forward on `stream`
// (ordered behind that forward; idempotent, a no-op when nothing is pending), whether there are any, and a buffer's address WITHOUT running them (vgh_net_buffer does)
extern "C" __attribute__((visibility("hidden"))) int vgh_net_set_defer(vgh_net* n, int on);
extern "C" __attribute__((visibility("hidden"))) int vgh_net_run_deferred(vgh_net* n, void* stream);
extern "C" __attribute__((visibility("hidden"))) int vgh_net_deferred_pending(vgh_net* n);
extern "C" __attribute__((visibility("hidden"))) void* vgh_net_buffer_ptr(vgh_net* n, int buf_id);
// what the survivor-row kernel asks of an op: 16-byte aligned bf16 rows, whole 32-cout weight tiles, its stored channels inside the `width` FLAME channels of the row
static inline bool vgh_row_op_ok(const vgh_row_op& o, int width) {
    return o.in && o.wpack && o.bias && o.cblocks >= 1 && o.cout_pad >= 32 && o.cout_pad % 32 == 0 && o.cout_store >= 1 && o.cout_store <= o.cout_pad && o.in_coff >= 0 && o.in_coff % 8 == 0 &&
           o.in_pitch % 8 == 0 && o.in_coff + 32 * o.cblocks <= o.in_pitch && o.out_coff >= VGH_PRED_FLAME_OFF && o.out_coff - VGH_PRED_FLAME_OFF + o.cout_store <= width && o.act != VGH_ACT_SILU;
}
// net.hip: the deferrable ops that write buffer `out_buf`, in program order; their count, or -1 when there are more than max_ops
extern "C" __attribute__((visibility("hidden"))) int vgh_net_row_ops(vgh_net* n, int out_buf, vgh_row_op* out, int max_ops);
// postproc.hip: the FLAME segment of the prediction rows of the survivors of a select, computed from the inputs of the deferred prediction convs.  Image b's survivors
// are keep_idx_dev[b][0 .. counts_dev[b]) (positions into idx_dev[b][0 .. n_in), anchors); launched over B x keep_k, blocks past the device-side count exit.
// out_dev [B, keep_k, 413]: the fixed-up vectors (gather_kernel's arithmetic); rows at and past the count are not written
int vgh_survivor_rows(const vgh_head_level* levels, int n_levels, const vgh_row_op* ops /*[n_levels][kMaxRowOps]*/, const int* n_ops, int B, int n_in, int keep_k,
                      const int32_t* idx_dev, const int32_t* keep_idx_dev, const int32_t* counts_dev, int shape_c, int expr_c, float* out_dev, void* stream);

// ---- deferred FLAME towers: the 3x3 convs in front of the deferred prediction convs (tower_plan.h), walked per survivor by postproc.hip ----
constexpr int kMaxTreeOps = 12;  // tower ops (kMaxTowerOps) + prediction convs (kMaxRowOps) of one level
struct vgh_tree_op {
    const uint16_t* wpack;  // packed weights, [tap * cblocks + cb][cout_pad][32]
    const float* bias;      // [cout_pad]
    int layer;              // 1 .. depth: a 3x3 conv from tensor layer - 1 to tensor layer; depth + 1: a prediction 1x1 conv from tensor depth to the fp32 row
    int in_coff, cblocks, cout_pad, cout_store, out_coff, act;  // out_coff: channel of the output tensor / of the prediction row
    int grp_cout, grp_in_stride;  // grouped conv (0: dense): cout group g reads the input window at in_coff + g * grp_in_stride
    int chain;              // conv_tiles.h chain_code of the tile the dense op would have run on (bit 0 tap-major, bit 1 bias first); prediction convs: 1
};
struct vgh_tower_tree {
    const uint16_t* root;   // bf16 root tensor, batch row 0
    int root_pitch, root_c0, root_c;  // its pitch and the channel window [c0, c0 + c) the first layer reads
    int depth;              // 3x3 layers: the root window of a survivor is (2 depth + 1)^2 pixels
    int chan[4];            // channels of tensor t as kept per survivor (t = 0: root_c; t >= 1: the pitch of the layer's buffer)
    int n_ops;
    vgh_tree_op op[kMaxTreeOps];  // program order: layers ascend, prediction convs last
};
// LDS of a survivor's walk: tensor t (t = 0 .. depth) as [(2 (depth - t) + 1)^2 pixels][chan[t] + 8] bf16 (8 channels of padding per pixel keep the 16-byte fragment
// reads of neighbouring pixels on different banks), then the fp32 prediction row.  off[t]: byte offset of tensor t, off[depth + 1]: of the row; returns the total
static inline int vgh_tower_lds(const vgh_tower_tree& t, int* off) {
    int at = 0;
    for (int l = 0; l <= t.depth; ++l) {
        const int side = 2 * (t.depth - l) + 1;
        if (off) off[l] = at;
        at += (side * side * (t.chan[l] + 8) * 2 + 15) / 16 * 16;
    }
    if (off) off[t.depth + 1] = at;
    return at + 416 * 4;
}
// what the survivor kernel asks of a tree: windows inside their tensors, 16-byte aligned fragment reads, whole 32-cout weight tiles, the prediction convs inside the
// `width` FLAME channels of the row, and a walk that fits the LDS of a workgroup
static inline bool vgh_tower_tree_ok(const vgh_tower_tree& t, int width) {
    if (!t.root || t.depth < 1 || t.depth > 3 || t.n_ops < 2 || t.n_ops > kMaxTreeOps || t.root_pitch % 8 || t.root_c0 % 8 || t.root_c < 32 || t.root_c % 8 || t.root_c0 + t.root_c > t.root_pitch) return false;
    for (int l = 0; l <= t.depth; ++l)
        if (t.chan[l] < 32 || t.chan[l] % 8) return false;
    int last = 1;
    for (int k = 0; k < t.n_ops; ++k) {
        const vgh_tree_op& o = t.op[k];
        if (!o.wpack || !o.bias || o.layer < last || o.layer > t.depth + 1 || o.cblocks < 1 || o.cout_pad < 32 || o.cout_pad % 32 || o.cout_store < 1 || o.cout_store > o.cout_pad) return false;
        if (o.chain < 0 || o.chain > 3 || o.act == VGH_ACT_SILU || o.in_coff < 0 || o.in_coff % 8 || o.grp_in_stride % 8 || o.grp_in_stride < 0) return false;
        if (o.grp_cout && (o.grp_cout % 32 || o.cout_pad % o.grp_cout)) return false;
        const int groups = o.grp_cout ? o.cout_pad / o.grp_cout : 1;
        if (o.in_coff + (groups - 1) * o.grp_in_stride + 32 * o.cblocks > t.chan[o.layer - 1]) return false;
        if (o.layer <= t.depth) {
            if (o.out_coff < 0 || o.out_coff + o.cout_store > t.chan[o.layer]) return false;
        } else if (o.grp_cout || o.out_coff < VGH_PRED_FLAME_OFF || o.out_coff - VGH_PRED_FLAME_OFF + o.cout_store > width || width > 413) {
            return false;
        }
        last = o.layer;
    }
    return last == t.depth + 1 && vgh_tower_lds(t, nullptr) <= 144 * 1024;
}
// net.hip: the tree in front of prediction buffer `out_buf` with the chains of the forward that left it pending; 0 and *t filled, or -1: no tree, nothing pending, or an
// op of it on a tile whose chain is unknown (the caller then runs the pending ops densely)
extern "C" __attribute__((visibility("hidden"))) int vgh_net_tower_tree(vgh_net* n, int out_buf, vgh_tower_tree* t);
// 1: the latest forward left tower ops pending (it skipped them), 0: it ran them or only the prediction convs are pending
extern "C" __attribute__((visibility("hidden"))) int vgh_net_towers_pending(vgh_net* n);
// postproc.hip: as vgh_survivor_rows, from the root windows: one workgroup per survivor walks its level's tree
int vgh_survivor_towers(const vgh_head_level* levels, int n_levels, const vgh_tower_tree* trees /*[n_levels]*/, int B, int n_in, int keep_k, const int32_t* idx_dev,
                        const int32_t* keep_idx_dev, const int32_t* counts_dev, int shape_c, int expr_c, float* out_dev, void* stream);

// letterbox.hip: the batched letterbox of VGH_IMG_U8_RAW / VGH_IMG_YUV420_RAW / VGH_IMG_YUV420P16_RAW, owned by a detector (canvas [arena_batch, S, S, 3] + two pinned / device staging slots)
struct vgh_lb_batch;
// Validates the B descriptors (VGH_ERR_INVALID naming the image; nothing allocated or queued) and packs their tables + the un-pad table into the
// next staging slot; *lb (NULL before the first RAW call) is created here.
int vgh_lb_prepare(vgh_lb_batch** lb, int S, int max_batch, int arena_batch, int image_fmt, const void* imgs, int B);  // imgs: B vgh_raw_image / vgh_yuv420_image
int vgh_lb_chunk(vgh_lb_batch* lb, int chunk, int n, hipStream_t stream);  // chunk's upload + ONE launch -> canvas rows [0, n)
int vgh_lb_unpad_read(vgh_lb_batch* lb, hipStream_t stream);            // a select on `stream` read the un-pad table of the last call
uint8_t* vgh_lb_canvas(const vgh_lb_batch* lb);
float* vgh_lb_unpad(const vgh_lb_batch* lb);  // [max_batch, 3] of the last prepared call
void vgh_lb_destroy(vgh_lb_batch* lb);
