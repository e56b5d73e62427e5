// The program plan of the network executor: everything vgh_net_create decides from (image_size, max_batch, bufs, ops, weights) WITHOUT a device -- the validation of
// the program, the arena and weight-blob layouts, the fusion marks, the cross-lane events -- plus the two pieces of arithmetic the executor shares with the rest of
// net.hip: the batch split over lanes and the descriptor -> ConvArgs filler.  Host logic on plain data: no HIP include, so tests/net_plan_host.hip checks it on its
// own under the host sanitizers, and vgh_net_create runs it before its first HIP call (a refused program allocates nothing).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/vgh.h"
#include "conv_tiles.h"

constexpr int kNetLanes = 4;  // lane 0 = the caller's stream

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// the ONE place that splits a batch over lanes: the rows of lane l when B images run on L lanes (the first B % L lanes take one more)
inline int rows_of_lane(int B, int L, int l) { return B / L + (l < B % L ? 1 : 0); }

// the sub-batches of B images on L lanes, in lane order: fn(rows, first row); stops at the first non-zero result and returns it
template <class F>
inline int for_each_lane(int B, int L, F&& fn) {
    int at = 0;
    for (int l = 0; l < L; ++l) {
        const int nb = rows_of_lane(B, L, l);
        if (int rc = fn(nb, at)) return rc;
        at += nb;
    }
    return 0;
}

// ---- descriptor -> ConvArgs: every numeric field of a conv launch, for the executor (vgh_op_desc + its buffers) and for vgh_conv2d (vgh_conv_call); both
//      descriptors name the shared fields alike.  The caller binds the pointers and out_scale afterwards. ----
struct ConvGeom {
    int fmt;                               // VGH_FMT_* of the input tensor
    int out_f32, out_fp8;                  // the executor takes them from the output buffer's format, vgh_conv2d from the call
    int B, H, W;
    int64_t in_pitch, out_pitch, res_pitch;  // LOGICAL channels per pixel (res_pitch = 0: the executor's "no residual")
    int out_planes, res_planes;            // planes of the output / residual tensors (an fp32 output has one whatever the input format)
};
template <class Desc>
inline void conv_args_fill(ConvArgs* a, const Desc& d, const ConvGeom& g) {
    memset(a, 0, sizeof(*a));
    // split parity modes: a pixel is [hi plane | lo plane]; the kernels address it with the physical pitch and the plane stride
    const bool h16 = g.fmt == VGH_FMT_F16;  // single-plane fp16 (r05): the fp16 split kernels with ONE K segment and no lo plane (ConvArgs::nseg)
    a->split = h16 ? VGH_FMT_F16X2 : vgh_fmt_planes(g.fmt) > 1 ? g.fmt : 0;
    a->nseg = h16 ? 1 : 3;
    a->in_plane = h16 ? 0 : (int)g.in_pitch;
    a->out_plane = h16 ? 0 : (int)g.out_pitch;
    a->res_plane = h16 ? 0 : (int)g.res_pitch;
    a->grp_cout = d.grp_cout;
    a->grp_in_stride = d.grp_in_stride;
    a->in_pitch = g.in_pitch * vgh_fmt_planes(g.fmt);
    a->in_coff = d.in_coff;
    a->cin = d.cin;
    a->B = g.B;
    a->H = g.H;
    a->W = g.W;
    a->ksize = d.ksize;
    a->stride = d.stride;
    a->pad = d.ksize / 2;  // (conv_tiles.h's tile_grid relies on it)
    a->Ho = (g.H + 2 * a->pad - d.ksize) / d.stride + 1;
    a->Wo = (g.W + 2 * a->pad - d.ksize) / d.stride + 1;
    a->out_pitch = g.out_pitch * g.out_planes;
    a->out_coff = d.out_coff;
    a->out_coff2 = d.out_coff2;
    a->out_split = d.out_split;
    a->cout_pad = d.cout_pad;
    a->cout_store = d.cout_store;
    a->out_f32 = g.out_f32;
    a->res_pitch = g.res_pitch * g.res_planes;
    a->res_coff = d.res_coff;
    a->in_fp8 = vgh_fmt_q8_kind(g.fmt);
    a->out_fp8 = g.out_fp8;
    a->alpha = d.alpha;
    a->act = d.act;
    a->shuffle = d.shuffle;
    a->shuffle_c = d.shuffle ? d.cout_pad / 4 : 0;
    a->P = g.B * a->Ho * a->Wo;
    a->cblocks = d.cin / (a->in_fp8 ? 64 : 32);  // 64-byte channel blocks
    a->nkb = d.ksize * d.ksize * a->cblocks;
}

// An int8 -> bf16 3x3 conv takes the diagonal bypass (conv_pp.hip DG) when at least half of its live rows have w[c][centre][c] as their largest weight -- the folded
// identity branch of a RepVGG block.  Exact either way (one element of the sum is evaluated in fp32 instead of through the int8 image); what it buys is the int8 grid
// of the remaining weights.  `enabled`: the process-wide switch (vgh_net_set_i8_diag).
inline bool i8_peel_diag(const float* w, const vgh_op_desc& d, bool enabled) {
    if (!enabled || d.ksize != 3 || d.stride != 1 || d.grp_cout || d.cin < d.cout_pad || d.cout_pad > 1024) return false;
    const size_t row = (size_t)9 * d.cin;
    int live = 0, dom = 0;
    for (int c = 0; c < d.cout_pad; ++c) {
        float mx = 0.0f;
        for (size_t i = 0; i < row; ++i) mx = fmaxf(mx, fabsf(w[(size_t)c * row + i]));
        if (mx > 0.0f) {
            ++live;
            if (fabsf(w[(size_t)c * row + (size_t)4 * d.cin + c]) >= mx) ++dom;
        }
    }
    return live > 0 && 2 * dom >= live;
}

// ops i and i + 1 are the only ones that touch tensor `buf`: no other conv or pool reads it, writes it or adds it as a residual (what lets a fused launch skip writing it)
inline bool sole_link(const vgh_op_desc* ops, int n_ops, int i, int buf) {
    for (int j = 0; j < n_ops; ++j)
        if (j != i && j != i + 1 && (ops[j].kind == VGH_OP_CONV || ops[j].kind == VGH_OP_SPP_POOL) && (ops[j].in_buf == buf || ops[j].out_buf == buf || ops[j].res_buf == buf)) return false;
    return true;
}

// Deferrable op (vgh_net_set_defer): a plain 1x1 / stride-1 bf16 conv that writes FLAME channels (VGH_PRED_FLAME_OFF and up: the box / score channels below are
// needed densely by the top-k) of an fp32 buffer which NO op of the program reads -- its rows reach the post-network stages only.  A pointwise conv: any row can be
// computed later, alone, from the row of its input -- which therefore has to survive the forward (no later op writes it) and must not be rewritten by the NEXT
// forward before the prediction guard has been waited for (every writer of the input stands behind the first conv with an fp32 output, where the executor waits).
// `fused_or_awaited`: the op is part of a back-to-back pair, a later op waits for its event, or its K window overhangs the pitch.
inline bool net_op_deferrable(const vgh_buf_desc* bufs, const vgh_op_desc* ops, int n_ops, int i, bool fused_or_awaited) {
    const vgh_op_desc& d = ops[i];
    if (d.kind != VGH_OP_CONV || d.ksize != 1 || d.stride != 1 || fused_or_awaited) return false;
    if (bufs[d.out_buf].is_f32 != VGH_FMT_F32 || bufs[d.in_buf].is_f32 != VGH_FMT_BF16) return false;
    if (d.res_buf >= 0 || d.shuffle || d.grp_cout || d.act == VGH_ACT_SILU || d.out_coff < VGH_PRED_FLAME_OFF || d.out_split < d.cout_pad || d.cout_store > d.cout_pad) return false;
    int first_f32 = n_ops;
    for (int j = n_ops - 1; j >= 0; --j)
        if (ops[j].kind == VGH_OP_CONV && bufs[ops[j].out_buf].is_f32 == VGH_FMT_F32) first_f32 = j;
    for (int j = 0; j < n_ops; ++j) {
        const vgh_op_desc& e = ops[j];
        if (e.kind == VGH_OP_FORK) continue;
        const bool conv = e.kind == VGH_OP_CONV;
        if ((conv || e.kind == VGH_OP_SPP_POOL) && e.in_buf == d.out_buf) return false;  // a second reader of the prediction buffer
        if (conv && e.res_buf == d.out_buf) return false;
        const bool writes_in = (conv || e.kind == VGH_OP_STEM) ? e.out_buf == d.in_buf : e.kind == VGH_OP_SPP_POOL && e.in_buf == d.in_buf;  // (the pool writes behind the channels it reads)
        if (writes_in && (j > i || j < first_f32)) return false;
    }
    return true;
}

// Pending state of the deferred ops, per forward generation: a deferring forward of B images leaves them pending; vgh_net_run_deferred takes them (once); a forward
// that runs every op, or the next deferring forward, replaces the state.
struct DeferState {
    bool on = false;       // vgh_net_set_defer
    bool pending = false;  // the current generation's deferrable ops have not run
    int B = 0;             // images of that forward
    bool towers = false;   // ... and neither have its tower-deferrable ops (tower_plan.h); never set without `pending`
    int lanes = 1;         // batch lanes of that forward: the pending tower ops run on the same sub-batches, hence on the same tiles
    bool skip() const { return on; }  // does a forward queued now skip the deferrable ops?
    void forward(int batch, bool skipped, bool skipped_towers = false, int batch_lanes = 1) {
        pending = skipped;
        B = skipped ? batch : 0;
        towers = skipped && skipped_towers;
        lanes = towers ? batch_lanes : 1;
    }
    int take() {  // the batch to run the deferred ops for, 0 = nothing pending; clears the mark
        const int b = pending ? B : 0;
        pending = false;
        towers = false;
        B = 0;
        return b;
    }
};

struct NetPlan {
    // arena: one slab, every buffer live for the whole forward (288 GB HBM: no aliasing games), in buffer order
    std::vector<int64_t> buf_off, buf_bytes;  // buf_bytes: the tensor for max_batch, without the slack behind it
    int64_t arena_bytes = 0;
    struct Op {
        int64_t w = 0, bias = 0;     // weight-blob offsets (bytes) of the weight image and the bias vector
        int64_t gscale = -1;         // per-cout output factors of an op that reads or writes an 8-bit buffer, else -1
        int64_t dvec = -1;           // the diagonal bypass of an int8 -> bf16 conv (i8_peel_diag), else -1
        int b2b = 0;                 // back-to-back GEMM: 1 = this conv and the NEXT op (a 1x1 / stride-1 conv, the only reader of its output) run as ONE launch, 2 = that second conv
        int overhang_ok = 0;         // the K window is wider than the input buffer's pitch, over weight columns verified to be exactly zero
        int ev_done = 0;             // a later op names this one as its producer (vgh_op_desc.lane bits 8+): an event is recorded behind it
        int deferrable = 0;          // a prediction 1x1 conv whose fp32 rows only the post-network stages read (net_op_deferrable): a deferring forward skips it
        int tower = 0;               // 1 + its tree: a 3x3 conv in front of deferrable convs whose output only they (or other such convs) read: skipped too (tower_plan.h fills it)
        int writes_tower_root = 0;   // the op writes the root window of a tower tree (tower_plan.h)
    };
    std::vector<Op> ops;
    int64_t wds = -1;         // -DVGH_EXPERIMENTS builds: the stage-1 downsample's second weight image (stem_ds.hip), else -1
    int64_t blob_bytes = 0;
    // index of the stem op when the stem + stage-1 downsample qualify as a pair (bf16, the architecture's 3x3 / stride-2 / 64 -> 96 conv as the stem tensor's only reader), else -1
    int stem_pair = -1;
    // two SIDE lanes wait for each other's ops: fine eagerly, but ROCm 7.0's hipStreamEndCapture recurses without end on such a program (vgh_net_capture refuses it)
    bool lane_wait_cycle = false;
    char err[256] = "";  // the message of a refusal
};

// VGH_OK and a filled plan, or VGH_ERR_INVALID and p->err.  No rule indexes an array that an earlier rule has not bounded.
inline int net_plan(int image_size, int max_batch, const vgh_buf_desc* bufs, int n_bufs, const vgh_op_desc* ops, int n_ops, const float* weights, int64_t n_weights, int64_t n_biases,
                    bool i8_diag, NetPlan* p) {
#define PLAN_REQUIRE(cond, ...)                          \
    do {                                                 \
        if (!(cond)) {                                   \
            snprintf(p->err, sizeof(p->err), __VA_ARGS__); \
            return VGH_ERR_INVALID;                      \
        }                                                \
    } while (0)
    *p = NetPlan();
    PLAN_REQUIRE(n_bufs >= 0 && n_ops >= 0, "net_create: negative buffer or op count");
    for (int i = 0; i < n_bufs; ++i) {
        PLAN_REQUIRE(bufs[i].is_f32 >= VGH_FMT_BF16 && bufs[i].is_f32 <= VGH_FMT_I8, "net_create: buffer %d has unknown format %d", i, bufs[i].is_f32);
        PLAN_REQUIRE(!vgh_fmt_is_q8(bufs[i].is_f32) || (bufs[i].scale > 0.0f && bufs[i].scale < 1e30f && bufs[i].pitch % 16 == 0), "net_create: 8-bit buffer %d needs a positive scale and a pitch that is a multiple of 16", i);
        const int64_t bytes = (int64_t)max_batch * bufs[i].h * bufs[i].w * bufs[i].pitch * vgh_fmt_bytes(bufs[i].is_f32);
        p->buf_off.push_back(p->arena_bytes);
        p->buf_bytes.push_back(bytes);
        p->arena_bytes += align_up(bytes + 256, 256);  // +256: slack so 16-byte gathers at the very end stay in-bounds
    }
    const auto buf_ok = [&](int id) { return id >= 0 && id < n_bufs; };
    p->ops.assign(n_ops, NetPlan::Op());
    int64_t at = 0;  // weight blob: per op its weight image, bias, gscale, dvec, each aligned to 256 bytes
    const auto take = [&](int64_t bytes) {
        const int64_t off = at;
        at += align_up(bytes, 256);
        return off;
    };
    for (int i = 0; i < n_ops; ++i) {
        const vgh_op_desc& d = ops[i];
        NetPlan::Op& o = p->ops[i];
        if (d.kind == VGH_OP_CONV) {
            PLAN_REQUIRE(d.cin % 32 == 0 && d.cout_pad % 32 == 0, "net_create: op %d channel padding", i);
            PLAN_REQUIRE(buf_ok(d.in_buf) && buf_ok(d.out_buf) && d.res_buf < n_bufs, "net_create: op %d buffer ids", i);
            const int64_t we = (int64_t)d.cout_pad * d.ksize * d.ksize * d.cin;
            PLAN_REQUIRE(d.w_off >= 0 && d.w_off + we <= n_weights && d.b_off >= 0 && d.b_off + d.cout_pad <= n_biases, "net_create: op %d weight range", i);
            const vgh_buf_desc& ib = bufs[d.in_buf];
            if (d.in_coff + d.cin > ib.pitch && !d.grp_cout) {
                // a K window wider than the pitch is legal only over all-zero weight columns, in the single-plane bf16 format (a split pixel's lo plane follows its hi plane):
                // the channels past the pitch are the next pixel's first ones, and finite x 0 adds +-0 to the accumulator
                const int live = ib.pitch - d.in_coff;
                PLAN_REQUIRE(live > 0 && ib.is_f32 == VGH_FMT_BF16, "net_create: op %d reads past the pitch of buffer %d", i, d.in_buf);
                const float* w = weights + d.w_off;
                for (int64_t r = 0; r < (int64_t)d.cout_pad * d.ksize * d.ksize; ++r)
                    for (int c = live; c < d.cin; ++c)
                        PLAN_REQUIRE(w[r * d.cin + c] == 0.0f, "net_create: op %d reads %d channels of a %d-channel pitch with a non-zero weight at input channel %d", i, d.cin, ib.pitch, c);
                o.overhang_ok = 1;
            }
            const int wf = ib.is_f32, of = bufs[d.out_buf].is_f32;
            // weight image: 8-bit (1 B), bf16 / fp16 (2 B), dense fp32 (4 B) or the three 16-bit segments of the split modes (6 B)
            o.w = take(we * (vgh_fmt_is_q8(wf) ? 1 : (wf == VGH_FMT_BF16 || wf == VGH_FMT_F16) ? 2 : wf == VGH_FMT_F32 ? 4 : 6));
            o.bias = take((int64_t)d.cout_pad * 4);
            if (vgh_fmt_is_q8(wf) || vgh_fmt_is_q8(of)) {
                o.gscale = take((int64_t)d.cout_pad * 4);
                if (wf == VGH_FMT_I8 && of == VGH_FMT_BF16 && i8_peel_diag(weights + d.w_off, d, i8_diag)) o.dvec = take((int64_t)d.cout_pad * 4);
            }
        } else if (d.kind == VGH_OP_STEM) {
            PLAN_REQUIRE(buf_ok(d.out_buf), "net_create: op %d buffer ids", i);
            PLAN_REQUIRE(d.w_off >= 0 && d.w_off + 27 * 48 <= n_weights && d.b_off >= 0 && d.b_off + 48 <= n_biases, "net_create: stem weight range");
            o.w = take(27 * 48 * 4);
            o.bias = take(64 * 4);
        } else if (d.kind == VGH_OP_SPP_POOL) {
            PLAN_REQUIRE(buf_ok(d.in_buf), "net_create: op %d buffer ids", i);
        }
        // exact cross-lane dependencies (arch.schedule_latency): lane = lane | (1 + producer op index) << 8
        if (d.lane >> 8) {
            const int dep = (d.lane >> 8) - 1;
            PLAN_REQUIRE(dep >= 0 && dep < i, "net_create: op %d waits for op %d, which does not precede it", i, dep);
            p->ops[dep].ev_done = 1;
        }
    }
    // stem + stage-1 downsample pair: the first stem that a conv follows, if that conv is the architecture's downsample and the stem tensor's only reader
    for (int i = 0; i + 1 < n_ops; ++i) {
        const vgh_op_desc &a = ops[i], &d = ops[i + 1];
        if (a.kind != VGH_OP_STEM || d.kind != VGH_OP_CONV) continue;
        if (image_size % 4 == 0 /* vgh_launch_stem_ds tiles 4 x 16 outputs of the 1/4-resolution map */ && d.in_buf == a.out_buf && d.in_coff == a.out_coff && d.ksize == 3 && d.stride == 2 && d.cin == 64 &&
            d.cout_pad == 96 && d.cout_store == 96 && d.res_buf < 0 && !d.shuffle && d.out_split >= 96 && d.act == VGH_ACT_RELU && d.grp_cout == 0 && bufs[a.out_buf].is_f32 == VGH_FMT_BF16 &&
            bufs[d.out_buf].is_f32 == VGH_FMT_BF16 && d.out_coff % 8 == 0 && bufs[d.out_buf].pitch % 8 == 0 && sole_link(ops, n_ops, i, a.out_buf)) {
            p->stem_pair = i;
#ifdef VGH_EXPERIMENTS  // (the pair is what the "u" tile of ds_b2b.hip fuses; the experiments build's stem_ds.hip needs a second weight image on top)
            p->wds = take((int64_t)9 * 3 * 96 * 16 * 2);
#endif
        }
        break;
    }
    p->blob_bytes = at;
    // back-to-back pairs (r06): a plain bf16 conv whose whole output tensor -- all of its channels in ONE cout tile -- is read by exactly one op, the next one, a plain
    // 1x1 / stride-1 bf16 conv (the architecture's stage downsample -> the CSP layer's merged conv1|conv2); nothing else touches that tensor.  An op is in one pair at most.
    for (int i = 0; i + 1 < n_ops; ++i) {
        const vgh_op_desc &a = ops[i], &b = ops[i + 1];
        if (a.kind != VGH_OP_CONV || b.kind != VGH_OP_CONV || p->ops[i].b2b != 0) continue;
        const vgh_buf_desc &ab = bufs[a.out_buf], &ai = bufs[a.in_buf], &bo = bufs[b.out_buf];
        if (ab.is_f32 == VGH_FMT_BF16 && ai.is_f32 == VGH_FMT_BF16 && bo.is_f32 == VGH_FMT_BF16 && vgh_conv_b2b_ok(a.ksize, a.stride, a.cout_pad, b.cout_pad) && a.cout_store == a.cout_pad &&
            a.out_coff == 0 && a.out_split >= a.cout_pad && ab.pitch == a.cout_pad && a.res_buf < 0 && !a.shuffle && !a.grp_cout && a.act != VGH_ACT_SILU && b.ksize == 1 && b.stride == 1 &&
            b.in_buf == a.out_buf && b.in_coff == 0 && b.cin == a.cout_pad && b.res_buf < 0 && !b.shuffle && !b.grp_cout && b.act != VGH_ACT_SILU && b.out_coff % 8 == 0 && b.out_coff2 % 8 == 0 &&
            b.out_split % 8 == 0 && b.cout_store % 8 == 0 && bo.pitch % 8 == 0 && sole_link(ops, n_ops, i, a.out_buf)) {
            p->ops[i].b2b = 1;
            p->ops[i + 1].b2b = 2;
        }
    }
    bool w[kNetLanes][kNetLanes] = {};  // w[a][b]: side lane a waits for an op of side lane b (directly, then transitively)
    for (int i = 0; i < n_ops; ++i) {
        if (!(ops[i].lane >> 8)) continue;
        const int a = ops[i].lane & 0xff, b = ops[(ops[i].lane >> 8) - 1].lane & 0xff;
        if (a > 0 && a < kNetLanes && b > 0 && b < kNetLanes && a != b) w[a][b] = true;
    }
    for (int k = 1; k < kNetLanes; ++k)
        for (int a = 1; a < kNetLanes; ++a)
            for (int b = 1; b < kNetLanes; ++b) w[a][b] = w[a][b] || (w[a][k] && w[k][b]);
    for (int a = 1; a < kNetLanes; ++a) p->lane_wait_cycle = p->lane_wait_cycle || w[a][a];
    for (int i = 0; i < n_ops; ++i) {
        const NetPlan::Op& o = p->ops[i];
        p->ops[i].deferrable = net_op_deferrable(bufs, ops, n_ops, i, o.b2b || o.ev_done || o.overhang_ok) && ops[i].out_coff + ops[i].cout_store <= bufs[ops[i].out_buf].pitch ? 1 : 0;
    }
    return VGH_OK;
#undef PLAN_REQUIRE
}
