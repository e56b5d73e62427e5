// Host side of libvgh.so: static-schedule network executor (pre-planned arena, concat-by-offset, one
// stream, optional hipGraph replay), stand-alone conv entry point, error/stream/event helpers.
//
// Replaces the TorchScript interpreter call `self.model(image)` (head_detector/detector.py:58-59).
#include <stdarg.h>

#include <atomic>
#include <memory>
#include <vector>

#include "net_plan.h"
#include "tower_plan.h"
#include "per_device.h"
#include "vgh_internal.h"

static thread_local char g_err[1024] = "";

void vgh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct NetOp {
    vgh_op_desc d;
    uint16_t* wpack = nullptr;  // device (conv)
    float* wf32 = nullptr;      // device (stem [27][48]; fp32 parity nets: the dense weights, same storage as wpack)
    float* bias = nullptr;      // device
    float out_scale = 1.0f;     // split parity modes: accumulator scale of the op (vgh_pack_conv_weights_split_host)
    // automatic tile of the op, resolved ONCE at vgh_net_create for the arena batch: every forward -- any batch size, any chunk, any lane -- then runs the op
    // on the same tile, so its fp32 summation order (hence every output bit) does not depend on how many images ride along
    int auto_cfg = -1;
    uint16_t* wds = nullptr;   // stage-1 downsample only: its weights in the fused stem + downsample kernel's layout (stem_ds.hip)
    float* gscale = nullptr;   // device [cout_pad] (NetPlan::Op::gscale), else nullptr
    float* dvec = nullptr;     // device [cout_pad] (NetPlan::Op::dvec), else nullptr
    int overhang_ok = 0, b2b = 0, deferrable = 0;  // as planned (NetPlan::Op)
    int tower = 0, writes_tower_root = 0;          // as planned (tower_plan.h): 1 + the op's tree / the op writes a tree's root window
    hipEvent_t ev_done = nullptr;  // recorded behind this op when the plan says a later op waits for it (NetPlan::Op::ev_done), else nullptr
};

static std::atomic<int> g_i8_diag{1};

struct vgh_net {
    int device = 0, image_size = 0, max_batch = 0;
    std::vector<vgh_buf_desc> bufs;
    std::vector<void*> buf_ptr;
    std::vector<int64_t> buf_bytes;
    std::vector<NetOp> ops;
    char* arena = nullptr;
    char* wblob = nullptr;  // all packed weights + biases
    uint16_t* zeros = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    static constexpr int kLanes = kNetLanes;  // lane 0 = the caller's stream
    hipStream_t side[kLanes] = {nullptr, nullptr, nullptr, nullptr};  // picked by ensure_lanes for `lanes_main`
    hipStream_t lanes_main = nullptr;
    bool lanes_ready = false;
    hipEvent_t ev_fork = nullptr, ev_join[kLanes] = {nullptr, nullptr, nullptr, nullptr}, ev_lag[kLanes] = {nullptr, nullptr, nullptr, nullptr};
    // optional guard (borrowed event): the first op that writes an fp32 prediction buffer waits for it, so a consumer of the
    // PREVIOUS forward's predictions may still be running on another stream while this forward's backbone / neck execute
    hipEvent_t pred_guard = nullptr;
    // batch split: the batch runs as `nsplit` independent sub-batches on the lane streams, so the fixed cost of every launch
    // (dispatch, tile prologue, first-load latency, epilogue store burst, tail) of one sub-batch hides under the main loops of
    // the others (measured on the M net at B = 32: 5.75 ms -> 5.35 ms with 4 lanes)
    int nsplit = 1;
    int stem_pair = -1;  // NetPlan::stem_pair: the stem + stage-1 downsample as ONE kernel (stem_ds.hip, ds_b2b.hip's "u" tile); results are bit-identical
    // NetPlan::lane_wait_cycle: under stream capture ROCm 7.0's runtime links a non-origin stream to the stream of every event it waits for and hipStreamEndCapture
    // then recurses without end (measured r06: a stack overflow inside hip::Stream::EndCapture) -> vgh_net_capture refuses
    bool lane_wait_cycle = false;
    int fuse_b2b = 1;   // vgh_net_set_b2b: the back-to-back pairs found at create time run fused (default) or as their two launches (every intermediate tensor then exists)
    int stem3_ok = 0;   // the stem + stage-1 pair can run as ONE launch (ds_b2b.hip, "u" tile): decided at the end of vgh_net_create, from the pair's descriptor
    // forward generation: bumped by every call that (re)writes the prediction buffers -- vgh_net_forward (and with it every chunk of vgh_detector_candidates and the
    // capture's recording pass), vgh_net_forward_graph, vgh_net_profile.  A detector's lazy FLAME gather remembers the generation it decoded and its select refuses another one
    uint64_t generation = 0;
    // deferred prediction ops (vgh_net_set_defer, NetPlan::Op::deferrable): a deferring forward skips them and leaves them pending for vgh_net_run_deferred; their
    // inputs (the last tensors of the FLAME towers) stay intact in the arena until the next forward.  `skipping`: true while such a forward queues its ops
    DeferState defer;
    bool skipping = false;
    // deferred towers (tower_plan.h): a deferring forward also skips the tower-deferrable ops when every one of them would run on a tile whose summation chain the
    // survivor kernel reproduces (conv_tiles.h, kChainTrait) -- decided per forward, for its batch and lanes, by the launcher's own tile resolution; else it runs them
    bool skipping_towers = false;   // true while such a forward queues its ops
    std::vector<int> tower_chain;   // per op: the chain code of the pending generation (valid where defer.towers)
    std::vector<TowerTree> trees;   // NetPlan::towers.trees
    bool guard_roots = false;       // the forward in front of the one being queued skipped its towers: selects of it read the trees' roots (writes_guarded)
    bool prev_towers = false;       // ... as left by the latest forward, replay or profile, for the next one
    bool graph_skips_towers = false;
    int graph_lanes = 1;
    std::vector<int> graph_chain;   // tower_chain as the capture resolved it
    bool graph_skips = false;  // what the captured graph does, whatever the switch says at replay
    int graph_B = 0;
    hipStream_t last_stream = nullptr;  // the caller's stream of the latest forward / replay: where vgh_net_buffer queues convs that forward left pending
    int fuse_stem = 0;  // opt-in (vgh_net_set_fuse_stem): measured r03, the fused kernel saves 1.5 GB of HBM traffic per L b64 forward but no time (EXPERIMENTS.md 8c)
};

static inline int64_t buf_image_bytes(const vgh_buf_desc& b) { return (int64_t)b.h * b.w * b.pitch * vgh_fmt_bytes(b.is_f32); }
static inline char* buf_at(const vgh_net* n, int id, int at) { return (char*)n->buf_ptr[id] + at * buf_image_bytes(n->bufs[id]); }  // batch row `at` of buffer `id`

static int net_conv_args(vgh_net* n, const NetOp& op, int B, int at, ConvArgs* a) {
    const vgh_op_desc& d = op.d;
    const vgh_buf_desc &ib = n->bufs[d.in_buf], &ob = n->bufs[d.out_buf];
    const vgh_buf_desc* rb = d.res_buf >= 0 ? &n->bufs[d.res_buf] : nullptr;
    conv_args_fill(a, d, ConvGeom{ib.is_f32, ob.is_f32 == VGH_FMT_F32, vgh_fmt_q8_kind(ob.is_f32), B, ib.h, ib.w, ib.pitch, ob.pitch, rb ? rb->pitch : 0, vgh_fmt_planes(ob.is_f32), rb ? vgh_fmt_planes(rb->is_f32) : 0});
    a->in = (const uint16_t*)buf_at(n, d.in_buf, at);
    a->out = buf_at(n, d.out_buf, at);
    a->res = rb ? (const uint16_t*)buf_at(n, d.res_buf, at) : nullptr;
    a->wpack = op.wpack;
    a->bias = op.bias;
    a->gscale = op.gscale;
    a->dvec = op.dvec;
    a->out_scale = op.out_scale;
    a->zeros = n->zeros;
    // e4m3 links (r05): bf16 -> e4m3, e4m3 -> bf16 and e4m3 -> e4m3 are legal pairs (3x3 / stride-1 convs on the ping-pong tiles); the residual of such an op is bf16
    const bool in8 = vgh_fmt_is_q8(ib.is_f32), out8 = vgh_fmt_is_q8(ob.is_f32);
    VGH_REQUIRE(a->out_f32 || ob.is_f32 == ib.is_f32 || (in8 && ob.is_f32 == VGH_FMT_BF16) || (out8 && ib.is_f32 == VGH_FMT_BF16), "net: op writes buffer %d in another format than it reads", d.out_buf);
    VGH_REQUIRE(!rb || rb->is_f32 == (in8 ? VGH_FMT_BF16 : ib.is_f32), "net: residual buffer %d has another format than the input", d.res_buf);
    VGH_REQUIRE(!(in8 || out8) || (d.ksize == 3 && d.stride == 1 && !d.grp_cout && !d.shuffle && (!in8 || d.cin % 64 == 0)), "net: an e4m3 buffer can only link plain 3x3 / stride-1 convs (cin %% 64 == 0)");
    const int eh = d.shuffle ? 2 * a->Ho : a->Ho, ew = d.shuffle ? 2 * a->Wo : a->Wo;
    VGH_REQUIRE(ob.h == eh && ob.w == ew, "net: op output buffer %d is %dx%d, conv produces %dx%d", d.out_buf, ob.h, ob.w, eh, ew);
    VGH_REQUIRE(op.overhang_ok || d.in_coff + d.cin + (d.grp_cout ? (d.cout_pad / d.grp_cout - 1) * d.grp_in_stride : 0) <= ib.pitch, "net: conv reads past the input pitch (buf %d)", d.in_buf);
    return VGH_OK;
}

static void net_b2b_fields(ConvArgs& a, const ConvArgs& a2) {  // the second conv of a back-to-back pair rides in the first one's descriptor
    a.w2pack = a2.wpack;
    a.bias2 = a2.bias;
    a.out2 = a2.out;
    a.out2_pitch = a2.out_pitch;
    a.out2_coff = a2.out_coff;
    a.out2_coff2 = a2.out_coff2;
    a.out2_split = a2.out_split;
    a.cout2_pad = a2.cout_pad;
    a.cout2_store = a2.cout_store;
    a.act2 = a2.act;
}

// forwards of u8 images run the stem conv inside the stage-1 pair's launch (ds_b2b.hip, "u" tile): the default b2b mode, the pair found and on its persistent tile.
// The stem is then a bf16 x 3 split GEMM on the matrix cores -- exact products, another fp32 summation order: a bf16 value across a rounding boundary where the sum lies within ~1e-7 of one (0.7 - 1.0 % of the stem values
// on the tie-rich `chain` case of tests/stem_pair_exact_cases.py, measured by tests/test_gpu_stem_pair_exact.py; rare with random weights);
// vgh_net_set_b2b(n, 3) keeps the stem launch and with it the bit-identity of every mode
static bool stem_in_pair_launch(const vgh_net* n) { return n->fuse_b2b == 1 && n->stem_pair >= 0 && n->stem3_ok == 1 && n->ops[n->stem_pair + 1].b2b == 1; }

// runs one op for the `B` images starting at batch row `at` (image pointer and every activation buffer offset accordingly)
static int net_run_op(vgh_net* n, const NetOp& op, const void* image0, int fmt, int B, int at, hipStream_t st, int share = 1) {
    const vgh_op_desc& d = op.d;
    const void* image = (const char*)image0 + (int64_t)at * n->image_size * n->image_size * 3 * (fmt == VGH_IMG_F32_NCHW ? 4 : 1);
    const int op_index = (int)(&op - n->ops.data());
    const bool fused = n->fuse_stem && n->stem_pair >= 0;
    const bool stem3 = stem_in_pair_launch(n) && !fused && fmt == VGH_IMG_U8_NHWC;
    switch (d.kind) {
        case VGH_OP_STEM: {
            if (stem3 && op_index == n->stem_pair) {
                const NetOp &ds = n->ops[op_index + 1], &nx = n->ops[op_index + 2];
                ConvArgs a, a2;
                if (int rc = net_conv_args(n, ds, B, at, &a)) return rc;
                if (int rc = net_conv_args(n, nx, B, at, &a2)) return rc;
                a.grid_share = share;
                net_b2b_fields(a, a2);
                return vgh_launch_stem_ds_b2b(a, image, n->image_size, n->image_size, op.wf32, op.bias, st);
            }
#ifdef VGH_EXPERIMENTS  // (stem_ds.hip is part of the experiments build only)
            if (fused && op_index == n->stem_pair) {
                const NetOp& ds = n->ops[op_index + 1];
                const vgh_buf_desc& db = n->bufs[ds.d.out_buf];
                return vgh_launch_stem_ds(image, fmt, B, n->image_size, n->image_size, op.wf32, op.bias, ds.wds, ds.bias, (uint16_t*)buf_at(n, ds.d.out_buf, at), db.pitch, ds.d.out_coff, st);
            }
#endif
            const vgh_buf_desc& ob = n->bufs[d.out_buf];
            if (ob.is_f32 == VGH_FMT_F32)  // fp32 parity mode
                return vgh_launch_stem_f32(image, fmt, B, n->image_size, n->image_size, op.wf32, op.bias, (float*)buf_at(n, d.out_buf, at), ob.pitch, d.out_coff, st);
            if (ob.is_f32 == VGH_FMT_F16)  // single-plane fp16: the fp16 split stem with plane stride 0 (split_store then writes the hi plane only)
                return vgh_launch_stem(image, fmt, B, n->image_size, n->image_size, op.wf32, op.bias, (uint16_t*)buf_at(n, d.out_buf, at), ob.pitch, d.out_coff, d.cout_store, VGH_FMT_F16X2, 0, st);
            return vgh_launch_stem(image, fmt, B, n->image_size, n->image_size, op.wf32, op.bias, (uint16_t*)buf_at(n, d.out_buf, at), (int64_t)ob.pitch * vgh_fmt_planes(ob.is_f32), d.out_coff,
                                   d.cout_store, ob.is_f32, ob.pitch, st);
        }
        case VGH_OP_CONV: {
            if ((fused || stem3) && op_index == n->stem_pair + 1) return VGH_OK;  // ran inside the stem's launch
            if (n->fuse_b2b && op.b2b == 2) return VGH_OK;             // ran inside the previous conv's launch
            if (n->skipping && op.deferrable) return VGH_OK;           // left pending for vgh_net_run_deferred
            if (n->skipping_towers && op.tower) return VGH_OK;         // its tower too: the select walks it for the survivors alone
            ConvArgs a;
            if (int rc = net_conv_args(n, op, B, at, &a)) return rc;
            a.grid_share = share;
            if (n->fuse_b2b && op.b2b == 1) {
                const NetOp& nx = n->ops[op_index + 1];
                ConvArgs a2;
                if (int rc = net_conv_args(n, nx, B, at, &a2)) return rc;
                net_b2b_fields(a, a2);
                a.b2b_igemm = n->fuse_b2b == 2;
                return vgh_launch_conv_b2b(a, st);
            }
            if (n->bufs[d.in_buf].is_f32 != VGH_FMT_F32) {
                a.fallback_cfg1 = op.auto_cfg + 1;
                return vgh_launch_conv(a, d.force_cfg >= 0 ? d.force_cfg : op.auto_cfg, st);
            }
            // fp32 parity mode: dense fp32 weights, FMA kernel
            VGH_REQUIRE(a.out_f32 && (d.res_buf < 0 || n->bufs[d.res_buf].is_f32 == VGH_FMT_F32), "net: fp32 conv needs fp32 output / residual buffers");
            VGH_REQUIRE(!d.grp_cout, "net: the fp32 FMA kernel has no grouped mode");
            return vgh_launch_conv_f32(a, op.wf32, st);
        }
        case VGH_OP_SPP_POOL: {
            const vgh_buf_desc& ib = n->bufs[d.in_buf];
            if (ib.is_f32 == VGH_FMT_F32) return vgh_launch_spp_pool_f32((float*)buf_at(n, d.in_buf, at), ib.pitch, d.in_coff, d.cin, B, ib.h, ib.w, st);
            if (ib.is_f32 == VGH_FMT_F16) return vgh_launch_spp_pool((uint16_t*)buf_at(n, d.in_buf, at), ib.pitch, d.in_coff, d.cin, B, ib.h, ib.w, VGH_FMT_F16X2, 0, st);  // plane stride 0: single plane
            return vgh_launch_spp_pool((uint16_t*)buf_at(n, d.in_buf, at), (int64_t)ib.pitch * vgh_fmt_planes(ib.is_f32), d.in_coff, d.cin, B, ib.h, ib.w, ib.is_f32, ib.pitch, st);
        }
        case VGH_OP_FORK:
            return VGH_OK;  // handled by the executor
        default:
            VGH_REQUIRE(false, "net: unknown op kind %d", d.kind);
    }
    return VGH_OK;
}

// Lane streams that are measured to overlap with the caller's stream and with each other (streams.hip: a fresh hipStreamCreate may
// share a hardware queue with `main`, which serialises the lanes and costs ~40 % of the forward).  Picked on the first forward that
// enters on `main`; a different caller stream re-picks.  Not callable while `main` is capturing (vgh_net_capture picks first).
static int ensure_lanes(vgh_net* n, hipStream_t main) {
    if (n->lanes_ready && n->lanes_main == main) return VGH_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(main, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
        VGH_REQUIRE(n->lanes_ready, "net: the lane streams cannot be picked while the caller's stream is capturing; run vgh_net_capture (or one forward) first");
        return VGH_OK;  // captured with the lanes picked for another caller stream: still correct, possibly not side by side
    }
    hipStream_t avoid[vgh_net::kLanes] = {main};
    for (int l = 1; l < vgh_net::kLanes; ++l) {
        if (n->side[l]) {
            VGH_HIP(hipStreamSynchronize(n->side[l]));
            vgh_stream_release_internal(n->device, n->side[l]);
            n->side[l] = nullptr;
        }
    }
    for (int l = 1; l < vgh_net::kLanes; ++l) {
        if (int rc = vgh_stream_acquire_internal(n->device, avoid, l, &n->side[l])) return rc;  // same priority as the caller's stream: a lower-priority lane starves (16.6 vs 13.6 ms)
        avoid[l] = n->side[l];
    }
    n->lanes_main = main;
    n->lanes_ready = true;
    return VGH_OK;
}

int vgh_net_lane_streams(vgh_net* n, hipStream_t main, hipStream_t* out) {
    if (int rc = ensure_lanes(n, main)) return rc;
    for (int l = 1; l < vgh_net::kLanes; ++l) out[l - 1] = n->side[l];
    return VGH_OK;
}

// The batch as nsplit independent sub-batches, one per lane stream (lane 0 = the caller's stream); launches are interleaved
// op by op.  lane_lag = 0: the lanes advance together.  lane_lag = k > 0: lane l starts when lane l-1 has finished its first k ops and
// stays k ops behind, so that the kernels running side by side are DIFFERENT layers (an HBM-bound 1x1 conv of one lane next to an
// MFMA-bound 3x3 conv of the other) instead of two copies of the same one.
static std::atomic<int> g_lane_lag{0};

// the ONE rule for how many batch lanes a forward of B images runs on (1: the whole batch on the caller's stream)
static int forward_lanes(const vgh_net* n, int B) { return (n->nsplit > 1 && B > 1) ? (n->nsplit < B ? n->nsplit : B) : 1; }

// The prediction guard (overlap mode): what a select of the PREVIOUS forward may still be reading on another stream.  The fp32 prediction buffers always; and, where
// that previous forward skipped its towers, the root windows of the trees, which such a select reads in their place (`guard_roots`: what the previous forward did,
// whatever this one does -- the switch may have been turned in between, or this batch may resolve to a tile without a chain trait).  The roots' writers stand in
// front of the first fp32 conv, so the wait moves up to them.  A forward behind one that ran its towers waits exactly where it always did.
static bool writes_guarded(const vgh_net* n, const NetOp& op) {
    if (op.d.kind == VGH_OP_CONV && n->bufs[op.d.out_buf].is_f32 == VGH_FMT_F32) return true;
    return n->guard_roots && op.writes_tower_root;
}

// The chain codes of the tower-deferrable ops for a forward of B images on L lanes: every op resolved as the launcher would, per lane.  false: there are no such ops,
// or one of them would run on a tile whose chain is unknown, or on different chains in different lanes -- the forward then runs its towers.
static bool tower_chains(vgh_net* n, int B, int L, std::vector<int>* chain) {
    chain->assign(n->ops.size(), -1);
    if (n->trees.empty() || B < 1) return false;
    for (size_t i = 0; i < n->ops.size(); ++i) {
        const NetOp& op = n->ops[i];
        if (!op.tower) continue;
        int lane = 0;
        const int bad = for_each_lane(B, L, [&](int nb, int at) {
            ConvArgs a;
            if (net_conv_args(n, op, nb, at, &a)) return 1;
            a.fallback_cfg1 = op.auto_cfg + 1;
            const int c = vgh_conv_chain(a, op.d.force_cfg >= 0 ? op.d.force_cfg : op.auto_cfg);
            if (c < 0 || (lane++ > 0 && c != (*chain)[i])) return 1;
            (*chain)[i] = c;
            return 0;
        });
        if (bad) return false;
    }
    return true;
}

static int net_forward_split(vgh_net* n, const void* image_dev, int image_fmt, int B, hipStream_t main) {
    const int L = forward_lanes(n, B);
    int at[vgh_net::kLanes + 1];
    at[0] = 0;
    for (int l = 0; l < L; ++l) at[l + 1] = at[l] + rows_of_lane(B, L, l);
    VGH_HIP(hipEventRecord(n->ev_fork, main));
    for (int l = 1; l < L; ++l) VGH_HIP(hipStreamWaitEvent(n->side[l], n->ev_fork, 0));
    std::vector<const NetOp*> seq;
    seq.reserve(n->ops.size());
    for (const NetOp& op : n->ops)
        if (op.d.kind != VGH_OP_FORK) seq.push_back(&op);  // head lanes are not combined with the batch split
    const int N = (int)seq.size();
    int lag = g_lane_lag.load(std::memory_order_relaxed);
    if (lag < 0) lag = 0;
    if (lag > N) lag = N;
    bool guard_pending[vgh_net::kLanes];
    for (int l = 0; l < L; ++l) guard_pending[l] = n->pred_guard != nullptr;
    for (int s = 0; s < N + lag * (L - 1); ++s) {
        for (int l = 0; l < L; ++l) {
            const int i = s - l * lag;
            if (i < 0 || i >= N) continue;
            const NetOp& op = *seq[i];
            hipStream_t st = l == 0 ? main : n->side[l];
            if (lag > 0 && l > 0 && i == 0) VGH_HIP(hipStreamWaitEvent(st, n->ev_lag[l - 1], 0));  // recorded below, `lag` ops into lane l-1
            if (guard_pending[l] && writes_guarded(n, op)) {
                VGH_HIP(hipStreamWaitEvent(st, n->pred_guard, 0));
                guard_pending[l] = false;
            }
            if (int rc = net_run_op(n, op, image_dev, image_fmt, at[l + 1] - at[l], at[l], st)) return rc;
            if (lag > 0 && l + 1 < L && i == lag - 1) VGH_HIP(hipEventRecord(n->ev_lag[l], st));
        }
    }
    for (int l = 1; l < L; ++l) {
        VGH_HIP(hipEventRecord(n->ev_join[l], n->side[l]));
        VGH_HIP(hipStreamWaitEvent(main, n->ev_join[l], 0));
    }
    return VGH_OK;
}

// Fills the host image of the weight blob at the plan's offsets; oscale[i]: the accumulator scale of a split-format op (else left at 1)
static void pack_weights(const NetPlan& plan, const vgh_buf_desc* bufs, const vgh_op_desc* ops, int n_ops, const float* weights_host, const float* biases_host, char* host, float* oscale) {
#ifdef VGH_EXPERIMENTS
    if (plan.stem_pair >= 0) vgh_pack_stem_ds_weights_host(weights_host + ops[plan.stem_pair + 1].w_off, (uint16_t*)(host + plan.wds));
#endif
    for (int i = 0; i < n_ops; ++i) {
        const vgh_op_desc& d = ops[i];
        const NetPlan::Op& po = plan.ops[i];
        if (d.kind == VGH_OP_CONV) {
            const int wf = bufs[d.in_buf].is_f32;
            if (wf == VGH_FMT_F32)
                memcpy(host + po.w, weights_host + d.w_off, (size_t)d.cout_pad * d.ksize * d.ksize * d.cin * 4);
            else if (wf == VGH_FMT_BF16)
                vgh_pack_conv_weights_host(weights_host + d.w_off, d.cout_pad, d.ksize, d.cin, (uint16_t*)(host + po.w));
            else if (vgh_fmt_is_q8(wf))
                ;  // below: the 8-bit image comes with per-cout scales that also enter the bias
            else
                vgh_pack_conv_weights_split_host(weights_host + d.w_off, d.cout_pad, d.ksize, d.cin, wf, (uint16_t*)(host + po.w), &oscale[i]);
            memcpy(host + po.bias, biases_host + d.b_off, (size_t)d.cout_pad * 4);
            if (po.gscale >= 0) {
                // e4m3 links: out = act(acc * g + bias) with g[c] = wscale[c] * scale(in) for an e4m3 input (1 for bf16), divided by scale(out) for an e4m3 output.
                // The kernel starts its accumulator at the bias, so the bias is stored in accumulator units: bias / (wscale[c] * scale(in)).
                float* g = (float*)(host + po.gscale);
                float* bq = (float*)(host + po.bias);
                const float s_out = vgh_fmt_is_q8(bufs[d.out_buf].is_f32) ? bufs[d.out_buf].scale : 1.0f;
                if (wf == VGH_FMT_I8) {
                    // int8: exact int32 accumulator that starts at the bias in accumulator units (int32 bit patterns in the bias vector); out = act(acc * g) with
                    // g = wscale[c] * scale(in) / scale(out)
                    std::vector<float> ws(d.cout_pad);
                    const float* wsrc = weights_host + d.w_off;
                    std::vector<float> peeled;
                    if (po.dvec >= 0) {  // diagonal bypass: w[c][centre][c] leaves the int8 image and is applied in fp32 by the epilogue (s_out = 1: bf16 output)
                        peeled.assign(wsrc, wsrc + (size_t)d.cout_pad * 9 * d.cin);
                        float* dv = (float*)(host + po.dvec);
                        for (int c = 0; c < d.cout_pad; ++c) {
                            float& wd = peeled[(size_t)c * 9 * d.cin + (size_t)4 * d.cin + c];
                            dv[c] = wd * bufs[d.in_buf].scale;
                            wd = 0.0f;
                        }
                        wsrc = peeled.data();
                    }
                    vgh_pack_conv_weights_i8_host(wsrc, d.cout_pad, d.ksize, d.cin, (uint8_t*)(host + po.w), ws.data());
                    for (int c = 0; c < d.cout_pad; ++c) {
                        const float acc_unit = ws[c] * bufs[d.in_buf].scale;
                        g[c] = acc_unit / s_out;
                        const float bi = __builtin_nearbyintf(bq[c] / acc_unit);
                        const int32_t b32 = bi != bi ? 0 : bi > 2.0e9f ? 2000000000 : bi < -2.0e9f ? -2000000000 : (int32_t)bi;  // (|bias| / unit is ~1e4 - 1e6 in practice)
                        memcpy(&bq[c], &b32, 4);
                    }
                } else if (wf == VGH_FMT_FP8) {
                    std::vector<float> ws(d.cout_pad);
                    vgh_pack_conv_weights_fp8_host(weights_host + d.w_off, d.cout_pad, d.ksize, d.cin, (uint8_t*)(host + po.w), ws.data());
                    for (int c = 0; c < d.cout_pad; ++c) {
                        const float acc_unit = ws[c] * bufs[d.in_buf].scale;
                        bq[c] = bq[c] / acc_unit;
                        g[c] = acc_unit / s_out;
                    }
                } else {
                    for (int c = 0; c < d.cout_pad; ++c) g[c] = 1.0f / s_out;
                }
            }
        } else if (d.kind == VGH_OP_STEM) {
            // host gives [48][3(ky)][3(kx)][3(ci)] -> device [27][48]
            float* dst = (float*)(host + po.w);
            for (int co = 0; co < 48; ++co)
                for (int k = 0; k < 27; ++k) dst[k * 48 + co] = weights_host[d.w_off + co * 27 + k];
            memcpy(host + po.bias, biases_host + d.b_off, 48 * 4);
        }
    }
}

// a network runs on a canvas; `who` names the entry point in the message
static int require_canvas(const char* who, int image_fmt) {
    VGH_REQUIRE(image_fmt == VGH_IMG_F32_NCHW || image_fmt == VGH_IMG_U8_NHWC, "%s: image format %d is not a canvas (VGH_IMG_U8_RAW, VGH_IMG_YUV420_RAW and VGH_IMG_YUV420P16_RAW are letterboxed by vgh_detect)", who, image_fmt);
    return VGH_OK;
}

struct NetDestroy {  // vgh_net_create's guard
    void operator()(vgh_net* net) const { vgh_net_destroy(net); }
};

extern "C" {

const char* vgh_version(void) { return "vgh 0.1.0 (gfx950)"; }
const char* vgh_last_error(void) { return g_err; }
int vgh_abi_version(void) { return VGH_ABI_VERSION; }

int vgh_net_create(int device, int image_size, int max_batch, const vgh_buf_desc* bufs, int n_bufs, const vgh_op_desc* ops, int n_ops,
                   const float* weights_host, int64_t n_weights, const float* biases_host, int64_t n_biases, vgh_net** out) {
    VGH_REQUIRE(out && bufs && ops && weights_host && biases_host, "net_create: null argument");
    VGH_REQUIRE(max_batch >= 1 && image_size >= 32 && image_size % 32 == 0, "net_create: bad max_batch / image_size");
    // ---- plan: no HIP call before the program is accepted, so a refused program allocates nothing ----
    NetPlan plan;
    if (int rc = net_plan(image_size, max_batch, bufs, n_bufs, ops, n_ops, weights_host, n_weights, n_biases, g_i8_diag.load(std::memory_order_relaxed) != 0, &plan)) {
        vgh_set_error("%s", plan.err);
        return rc;
    }
    TowerPlan towers;  // the second mark of the defer switch (tower_plan.h)
    net_plan_towers(bufs, ops, n_ops, &plan, &towers);
    VGH_HIP(hipSetDevice(device));
    // ---- allocate: from here on the guard destroys the half-built net on every early return (vgh_net_destroy takes null pointers and events) ----
    std::unique_ptr<vgh_net, NetDestroy> guard(new vgh_net());
    vgh_net* n = guard.get();
    n->device = device;
    n->image_size = image_size;
    n->max_batch = max_batch;
    n->bufs.assign(bufs, bufs + n_bufs);
    n->buf_bytes = plan.buf_bytes;
    n->stem_pair = plan.stem_pair;
    n->lane_wait_cycle = plan.lane_wait_cycle;
    VGH_HIP(hipMalloc((void**)&n->arena, plan.arena_bytes));
    VGH_HIP(hipMemset(n->arena, 0, plan.arena_bytes));  // padding channels that no op writes must be exact zeros
    for (int i = 0; i < n_bufs; ++i) n->buf_ptr.push_back(n->arena + plan.buf_off[i]);
    VGH_HIP(hipMalloc((void**)&n->zeros, 256));
    VGH_HIP(hipMemset(n->zeros, 0, 256));
    VGH_HIP(hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming));
    for (int l = 1; l < vgh_net::kLanes; ++l) VGH_HIP(hipEventCreateWithFlags(&n->ev_join[l], hipEventDisableTiming));  // lane streams: ensure_lanes
    for (int l = 0; l < vgh_net::kLanes; ++l) VGH_HIP(hipEventCreateWithFlags(&n->ev_lag[l], hipEventDisableTiming));
    // ---- weights: pack on the host, one upload ----
    std::vector<char> host(plan.blob_bytes > 0 ? plan.blob_bytes : 1, 0);
    std::vector<float> oscale(n_ops, 1.0f);
    pack_weights(plan, bufs, ops, n_ops, weights_host, biases_host, host.data(), oscale.data());
    VGH_HIP(hipMalloc((void**)&n->wblob, host.size()));
    VGH_HIP(hipMemcpy(n->wblob, host.data(), host.size(), hipMemcpyHostToDevice));
    for (int i = 0; i < n_ops; ++i) {
        const NetPlan::Op& po = plan.ops[i];
        NetOp op;
        op.d = ops[i];
        op.out_scale = oscale[i];
        op.overhang_ok = po.overhang_ok;
        op.b2b = po.b2b;
        op.deferrable = po.deferrable;
        op.tower = po.tower;
        op.writes_tower_root = po.writes_tower_root;
        if (ops[i].kind == VGH_OP_CONV || ops[i].kind == VGH_OP_STEM) {
            op.wf32 = (float*)(n->wblob + po.w);  // conv: the same storage as wpack, bf16 image (throughput mode) or dense fp32 (parity mode)
            op.bias = (float*)(n->wblob + po.bias);
        }
        if (ops[i].kind == VGH_OP_CONV) op.wpack = (uint16_t*)(n->wblob + po.w);
        if (po.gscale >= 0) op.gscale = (float*)(n->wblob + po.gscale);
        if (po.dvec >= 0) op.dvec = (float*)(n->wblob + po.dvec);
        if (plan.wds >= 0 && i == plan.stem_pair + 1) op.wds = (uint16_t*)(n->wblob + plan.wds);
        n->ops.push_back(op);  // (before its event: vgh_net_destroy finds the event through the op)
        if (po.ev_done) VGH_HIP(hipEventCreateWithFlags(&n->ops[i].ev_done, hipEventDisableTiming));
    }
    // ---- the automatic tile of every 16-bit conv, for the arena batch: one choice per op whatever batch / chunk / lane later runs it (bit-identical results across
    // chunkings), resolved here so that a max_batch whose tensors break the 2 GiB rule of the loaders fails at creation, and no forward ever writes the net ----
    for (NetOp& op : n->ops) {
        if (op.d.kind != VGH_OP_CONV || n->bufs[op.d.in_buf].is_f32 == VGH_FMT_F32) continue;
        ConvArgs ref;
        if (int rc = net_conv_args(n, op, n->max_batch, 0, &ref)) return rc;
        if (int rc = vgh_conv_prepare(ref)) return rc;
        op.auto_cfg = vgh_conv_pick_auto(ref);
    }
    n->trees = towers.trees;
    n->tower_chain.assign(n->ops.size(), -1);
    // ---- the stem + the stage-1 pair as one launch ("u" tile): decided once, from the pair's descriptor ----
    if (n->stem_pair >= 0 && n->stem_pair + 2 < (int)n->ops.size() && n->ops[n->stem_pair + 1].b2b == 1 && image_size % 32 == 0) {
        ConvArgs a, a2;
        if (!net_conv_args(n, n->ops[n->stem_pair + 1], 1, 0, &a) && !net_conv_args(n, n->ops[n->stem_pair + 2], 1, 0, &a2)) {
            net_b2b_fields(a, a2);
            if (!vgh_conv_prepare(a)) n->stem3_ok = vgh_conv_ds_b2b_ok(a) && a.act == VGH_ACT_RELU ? 1 : 0;
        }
    }
    *out = guard.release();
    return VGH_OK;
}

void vgh_net_destroy(vgh_net* n) {
    if (!n) return;
    if (n->graph_exec) hipGraphExecDestroy(n->graph_exec);
    if (n->graph) hipGraphDestroy(n->graph);
    for (int l = 1; l < vgh_net::kLanes; ++l) {
        if (n->side[l]) {
            hipStreamSynchronize(n->side[l]);
            vgh_stream_release_internal(n->device, n->side[l]);
        }
        if (n->ev_join[l]) hipEventDestroy(n->ev_join[l]);
    }
    for (int l = 0; l < vgh_net::kLanes; ++l)
        if (n->ev_lag[l]) hipEventDestroy(n->ev_lag[l]);
    if (n->ev_fork) hipEventDestroy(n->ev_fork);
    for (NetOp& op : n->ops)
        if (op.ev_done) hipEventDestroy(op.ev_done);
    hipFree(n->arena);
    hipFree(n->wblob);
    hipFree(n->zeros);
    delete n;
}

int vgh_net_forward(vgh_net* n, const void* image_dev, int image_fmt, int B, void* stream) {
    VGH_REQUIRE(n && image_dev, "net_forward: null argument");
    if (int rc = require_canvas("net_forward", image_fmt)) return rc;
    VGH_REQUIRE(B >= 0 && B <= n->max_batch, "net_forward: B=%d exceeds max_batch=%d", B, n->max_batch);
    // Independent branches (the three detection heads) run on side streams: a FORK op records an event on the main stream,
    // the first op of a lane after it makes that lane's stream wait for the event, and every used lane is joined back into
    // the main stream at the end (also valid under stream capture: the graph gets parallel branches).
    hipStream_t main = (hipStream_t)stream;
    ++n->generation;  // before anything is queued: a forward that fails half-way has touched the prediction buffers too
    {
        std::vector<int> chain;
        const int L = forward_lanes(n, B);
        const bool towers = n->defer.skip() && tower_chains(n, B, L, &chain);
        n->guard_roots = n->prev_towers;  // (sticky: vgh_net_run_deferred clears defer.towers, but a select queued before it may still be reading the roots)
        n->prev_towers = towers;
        n->defer.forward(B, n->defer.skip(), towers, L);
        if (towers) n->tower_chain.swap(chain);
    }
    n->last_stream = main;
    struct Skipping {  // cleared on every return path
        vgh_net* n;
        ~Skipping() { n->skipping = n->skipping_towers = false; }
    } skipping{n};
    n->skipping = n->defer.pending;
    n->skipping_towers = n->defer.towers;
    if (int rc = ensure_lanes(n, main)) return rc;
    if (forward_lanes(n, B) > 1) return net_forward_split(n, image_dev, image_fmt, B, main);
    bool pending[vgh_net::kLanes] = {false, false, false, false}, used[vgh_net::kLanes] = {false, false, false, false};
    bool guard_pending = n->pred_guard != nullptr;
    for (const NetOp& op : n->ops) {
        if (guard_pending && writes_guarded(n, op)) {
            // every stream that may run a prediction conv waits (main; the lanes inherit it through the fork / their own wait)
            VGH_HIP(hipStreamWaitEvent(main, n->pred_guard, 0));
            for (int l = 1; l < vgh_net::kLanes; ++l)
                if (n->side[l]) VGH_HIP(hipStreamWaitEvent(n->side[l], n->pred_guard, 0));
            guard_pending = false;
        }
        if (op.d.kind == VGH_OP_FORK) {
            VGH_HIP(hipEventRecord(n->ev_fork, main));
            for (int l = 1; l < vgh_net::kLanes; ++l) pending[l] = true;
            continue;
        }
        const int lane_f = op.d.lane & 0xff, dep = (op.d.lane >> 8) - 1;
        const int lane = (lane_f > 0 && lane_f < vgh_net::kLanes) ? lane_f : 0;
        hipStream_t st = main;
        if (lane > 0) {
            st = n->side[lane];
            if (pending[lane]) {
                VGH_HIP(hipStreamWaitEvent(st, n->ev_fork, 0));
                pending[lane] = false;
            }
            used[lane] = true;
        }
        if (dep >= 0 && dep < (int)n->ops.size() && n->ops[dep].ev_done) VGH_HIP(hipStreamWaitEvent(st, n->ops[dep].ev_done, 0));  // the ONE op this op waits for, on another lane
        if (int rc = net_run_op(n, op, image_dev, image_fmt, B, 0, st)) return rc;
        if (op.ev_done) VGH_HIP(hipEventRecord(op.ev_done, st));
    }
    for (int l = 1; l < vgh_net::kLanes; ++l)
        if (used[l]) {
            VGH_HIP(hipEventRecord(n->ev_join[l], n->side[l]));
            VGH_HIP(hipStreamWaitEvent(main, n->ev_join[l], 0));
        }
    return VGH_OK;
}

int vgh_net_profile(vgh_net* n, const void* image_dev, int image_fmt, int B, void* stream, float* op_ms) {
    VGH_REQUIRE(n && image_dev && op_ms, "net_profile: null argument");
    if (int rc = require_canvas("net_profile", image_fmt)) return rc;
    VGH_REQUIRE(B >= 0 && B <= n->max_batch, "net_profile: B=%d exceeds max_batch=%d", B, n->max_batch);
    hipStream_t st = (hipStream_t)stream;
    ++n->generation;
    n->defer.forward(B, false);  // the profiler runs every op: dense prediction buffers, nothing pending
    n->prev_towers = false;
    if (int rc = ensure_lanes(n, st)) return rc;
    const size_t m = n->ops.size();
    struct Events {  // destroyed on every return path
        std::vector<hipEvent_t> v;
        ~Events() {
            for (hipEvent_t e : v)
                if (e) hipEventDestroy(e);
        }
    } events{std::vector<hipEvent_t>(m + 1, nullptr)};
    std::vector<hipEvent_t>& ev = events.v;
    for (auto& e : ev) VGH_HIP(hipEventCreate(&e));
    VGH_HIP(hipEventRecord(ev[0], st));
    const int L = forward_lanes(n, B);
    for (size_t i = 0; i < m; ++i) {
        if (L == 1) {
            if (int rc = net_run_op(n, n->ops[i], image_dev, image_fmt, B, 0, st)) return rc;
        } else {
            // batch-split mode: the op's sub-batches run concurrently on the lane streams, as in vgh_net_forward
            VGH_HIP(hipEventRecord(n->ev_fork, st));
            int at = 0;
            for (int l = 0; l < L; ++l) {
                const int nb = rows_of_lane(B, L, l);
                hipStream_t ls = l == 0 ? st : n->side[l];
                if (l > 0) VGH_HIP(hipStreamWaitEvent(ls, n->ev_fork, 0));
                if (int rc = net_run_op(n, n->ops[i], image_dev, image_fmt, nb, at, ls)) return rc;
                if (l > 0) {
                    VGH_HIP(hipEventRecord(n->ev_join[l], ls));
                    VGH_HIP(hipStreamWaitEvent(st, n->ev_join[l], 0));
                }
                at += nb;
            }
        }
        VGH_HIP(hipEventRecord(ev[i + 1], st));
    }
    VGH_HIP(hipEventSynchronize(ev[m]));
    for (size_t i = 0; i < m; ++i) VGH_HIP(hipEventElapsedTime(&op_ms[i], ev[i], ev[i + 1]));
    return VGH_OK;
}

int vgh_net_capture(vgh_net* n, const void* image_dev, int image_fmt, int B, void* stream) {
    VGH_REQUIRE(n && stream, "net_capture: needs a non-null stream");
    if (int rc = require_canvas("net_capture", image_fmt)) return rc;
    VGH_REQUIRE(!n->pred_guard, "net_capture: a prediction guard event is set (detector overlap mode); graph replay cannot honour it");
    VGH_REQUIRE(!n->lane_wait_cycle, "net_capture: two side lanes of this program wait for each other's ops; the HIP runtime cannot end the capture of such a program (run it eagerly, "
                "or lay the lanes out so that the wait-for relation among lanes 1..3 is acyclic, as arch.schedule_latency does)");
    hipStream_t st = (hipStream_t)stream;
    if (n->graph_exec) {
        hipGraphExecDestroy(n->graph_exec);
        n->graph_exec = nullptr;
    }
    if (n->graph) {
        hipGraphDestroy(n->graph);
        n->graph = nullptr;
    }
    if (int rc = ensure_lanes(n, st)) return rc;  // probing launches kernels: before the capture begins
    VGH_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = vgh_net_forward(n, image_dev, image_fmt, B, stream);
    n->graph_skips = n->defer.pending;
    n->graph_skips_towers = n->defer.towers;
    n->graph_lanes = n->defer.lanes;
    n->graph_chain = n->tower_chain;
    n->graph_B = B;
    n->defer.forward(0, false);  // the recording pass ran nothing: no tower outputs of this generation to run deferred ops on
    hipError_t e = hipStreamEndCapture(st, &n->graph);
    if (rc) return rc;
    VGH_HIP(e);
    VGH_HIP(hipGraphInstantiate(&n->graph_exec, n->graph, nullptr, nullptr, 0));
    return VGH_OK;
}

int vgh_net_forward_graph(vgh_net* n, void* stream) {
    VGH_REQUIRE(n && n->graph_exec, "net_forward_graph: call vgh_net_capture first");
    VGH_REQUIRE(!n->pred_guard, "net_forward_graph: a prediction guard event is set (detector overlap mode); use vgh_net_forward");
    ++n->generation;
    n->defer.forward(n->graph_B, n->graph_skips, n->graph_skips_towers, n->graph_lanes);
    n->prev_towers = n->graph_skips_towers;
    if (n->graph_skips_towers) n->tower_chain = n->graph_chain;
    n->last_stream = (hipStream_t)stream;
    VGH_HIP(hipGraphLaunch(n->graph_exec, (hipStream_t)stream));
    return VGH_OK;
}

int vgh_net_set_defer(vgh_net* n, int on) {
    VGH_REQUIRE(n, "net_set_defer: null handle");
    n->defer.on = on != 0;  // from the next forward on; ops left pending by an earlier one stay pending
    return VGH_OK;
}

int vgh_net_run_deferred(vgh_net* n, void* stream) {
    VGH_REQUIRE(n, "net_run_deferred: null handle");
    const bool towers = n->defer.towers;
    const int L = n->defer.lanes;
    const int B = n->defer.take();
    if (B == 0) return VGH_OK;
    // every pending op in program order, on the stream the forward was joined into: the towers first -- on the forward's own sub-batches, so each runs on the tile
    // (and summation chain) it would have had there -- then the prediction convs, one launch per op for the whole batch: a 1x1's chain is the same on every tile of
    // the table, so the rows are the bits a forward that runs the op itself writes, whatever its batch split
    for (const NetOp& op : n->ops) {
        if (towers && op.tower)
            if (int rc = for_each_lane(B, L, [&](int nb, int at) { return net_run_op(n, op, nullptr, VGH_IMG_U8_NHWC, nb, at, (hipStream_t)stream); })) return rc;
        if (op.deferrable)
            if (int rc = net_run_op(n, op, nullptr, VGH_IMG_U8_NHWC, B, 0, (hipStream_t)stream)) return rc;
    }
    return VGH_OK;
}

int vgh_net_deferred_pending(vgh_net* n) { return n && n->defer.pending ? 1 : 0; }
int vgh_net_towers_pending(vgh_net* n) { return n && n->defer.pending && n->defer.towers ? 1 : 0; }

void* vgh_net_buffer_ptr(vgh_net* n, int buf_id) { return (n && buf_id >= 0 && buf_id < (int)n->buf_ptr.size()) ? n->buf_ptr[buf_id] : nullptr; }
// dense buffers are handed out complete: convs that the latest forward left pending (vgh_net_set_defer) and that write this buffer are queued first, behind that forward
void* vgh_net_buffer(vgh_net* n, int buf_id) {
    void* p = vgh_net_buffer_ptr(n, buf_id);
    if (p && n->defer.pending)
        for (const NetOp& op : n->ops)
            if ((op.deferrable || (n->defer.towers && op.tower)) && op.d.out_buf == buf_id) {
                if (vgh_net_run_deferred(n, n->last_stream)) return nullptr;  // (vgh_last_error says why)
                break;
            }
    return p;
}
int64_t vgh_net_buffer_bytes(vgh_net* n, int buf_id) { return (n && buf_id >= 0 && buf_id < (int)n->buf_bytes.size()) ? n->buf_bytes[buf_id] : -1; }

#ifdef VGH_EXPERIMENTS
int vgh_net_set_lane_lag(int ops) {
    VGH_REQUIRE(ops >= 0, "net_set_lane_lag: negative");
    g_lane_lag.store(ops, std::memory_order_relaxed);
    return VGH_OK;
}
#endif

int vgh_net_set_split(vgh_net* n, int nsplit) {
    VGH_REQUIRE(n, "net_set_split: null handle");
    VGH_REQUIRE(nsplit >= 1 && nsplit <= vgh_net::kLanes, "net_set_split: 1..%d lanes", vgh_net::kLanes);
    n->nsplit = nsplit;
    return VGH_OK;
}

#ifdef VGH_EXPERIMENTS
int vgh_net_set_fuse_stem(vgh_net* n, int enable) {
    VGH_REQUIRE(n, "net_set_fuse_stem: null handle");
    n->fuse_stem = enable ? 1 : 0;
    return VGH_OK;
}
#endif

int vgh_net_set_pred_guard(vgh_net* n, void* event) {
    VGH_REQUIRE(n, "net_set_pred_guard: null handle");
    n->pred_guard = (hipEvent_t)event;
    return VGH_OK;
}

// Back-to-back GEMM pairs (a stage's downsample + the CSP layer's conv1|conv2 behind it) as one launch each (default) or as two: the outputs are the same bits; unfused,
// every intermediate tensor of the program exists in the arena (what the per-op parity tests read)
int vgh_net_set_b2b(vgh_net* n, int enable) {
    VGH_REQUIRE(n, "net_set_b2b: null handle");
    n->fuse_b2b = (enable == 2 || enable == 3) ? enable : enable ? 1 : 0;  // 1: pairs fused, the stem conv inside the stage-1 pair's launch for u8 images; 3: without the stem; 2: every pair on the implicit-GEMM b2b tile
    return VGH_OK;
}
int vgh_net_stem_fused(vgh_net* n) {  // 1: forwards of u8 images run the stem conv inside the stage-1 pair's launch (the stem tensor is not written)
    return n && stem_in_pair_launch(n) ? 1 : 0;
}
int vgh_net_b2b_pairs(vgh_net* n) {
    int k = 0;
    if (n)
        for (const NetOp& op : n->ops) k += op.b2b == 1;
    return k;
}

uint64_t vgh_net_generation(vgh_net* n) { return n ? n->generation : 0; }

int vgh_net_row_ops(vgh_net* n, int out_buf, vgh_row_op* out, int max_ops) {
    if (!n || !out) return -1;
    int k = 0;
    for (const NetOp& op : n->ops) {
        if (!op.deferrable || op.d.out_buf != out_buf) continue;
        if (k == max_ops) return -1;
        const vgh_buf_desc& ib = n->bufs[op.d.in_buf];
        out[k++] = vgh_row_op{(const uint16_t*)n->buf_ptr[op.d.in_buf], op.wpack, op.bias, ib.pitch, op.d.in_coff, op.d.cin / 32, op.d.cout_pad, op.d.cout_store, op.d.out_coff, op.d.act};
    }
    return k;
}
int vgh_net_tower_tree(vgh_net* n, int out_buf, vgh_tower_tree* t) {
    if (!n || !t || !n->defer.pending || !n->defer.towers) return -1;
    for (const TowerTree& tr : n->trees) {
        if (tr.pred_buf != out_buf) continue;
        memset(t, 0, sizeof(*t));
        const vgh_buf_desc& rb = n->bufs[tr.root_buf];
        t->root = (const uint16_t*)n->buf_ptr[tr.root_buf];
        t->root_pitch = rb.pitch;
        t->root_c0 = tr.root_c0;
        t->root_c = tr.root_c1 - tr.root_c0;
        t->depth = tr.depth;
        if (tr.depth < 1 || tr.depth > kMaxTowerDepth) return -1;
        t->chan[0] = t->root_c;
        for (int l = 1; l <= tr.depth; ++l) t->chan[l] = n->bufs[tr.bufs[l]].pitch;
        int k = 0;
        for (size_t j = 0; j < tr.ops.size(); ++j) {
            const NetOp& op = n->ops[tr.ops[j]];
            const int chain = n->tower_chain[tr.ops[j]];
            if (chain < 0 || k == kMaxTreeOps) return -1;
            // layer 1 reads the root window, kept per survivor from channel root_c0 on
            t->op[k++] = vgh_tree_op{op.wpack, op.bias, tr.layer[j], op.d.in_coff - (tr.layer[j] == 1 ? tr.root_c0 : 0), op.d.cin / 32, op.d.cout_pad, op.d.cout_store, op.d.out_coff, op.d.act,
                                     op.d.grp_cout, op.d.grp_in_stride, chain};
        }
        for (const NetOp& op : n->ops) {
            if (!op.deferrable || op.d.out_buf != out_buf) continue;
            if (k == kMaxTreeOps || op.d.in_buf != tr.bufs[tr.depth]) return -1;
            t->op[k++] = vgh_tree_op{op.wpack, op.bias, tr.depth + 1, op.d.in_coff, op.d.cin / 32, op.d.cout_pad, op.d.cout_store, op.d.out_coff, op.d.act, 0, 0, 1};
        }
        t->n_ops = k;
        return 0;
    }
    return -1;
}
int vgh_net_max_batch(vgh_net* n) { return n ? n->max_batch : 0; }
int vgh_net_device(vgh_net* n) { return n ? n->device : 0; }
int vgh_net_image_size(vgh_net* n) { return n ? n->image_size : 0; }

int vgh_net_set_cfg(vgh_net* n, int op_index, int cfg) {
    VGH_REQUIRE(n && op_index >= 0 && op_index < (int)n->ops.size(), "net_set_cfg: bad op index");
    const int fmt0 = n->bufs[n->ops[op_index].d.kind == VGH_OP_CONV ? n->ops[op_index].d.in_buf : 0].is_f32;
    const bool split_net = vgh_fmt_planes(fmt0) > 1 || fmt0 == VGH_FMT_F16;  // the single-plane fp16 nets index the split modes' tile table too
    VGH_REQUIRE(cfg >= -1 && cfg < (split_net ? vgh_conv_split_num_cfgs() : vgh_conv_num_cfgs()), "net_set_cfg: bad cfg");
    NetOp& op = n->ops[op_index];
    if (cfg >= 0 && op.d.kind == VGH_OP_CONV && !split_net && (n->bufs[op.d.in_buf].is_f32 == VGH_FMT_BF16 || vgh_fmt_is_q8(n->bufs[op.d.in_buf].is_f32))) {
        // eligibility is decided ONCE, for the arena batch: a tile that fits a small chunk but not max_batch (the ping-pong tiles' 2 GiB rule depends on the
        // pixel count) would otherwise run some batch sizes and silently fall back on others -- two summation orders for one op, against the "same bits for
        // any chunk" invariant of NetOp::auto_cfg.  Such a tile is replaced by the automatic one for every batch, and the replacement is logged.
        ConvArgs ref;
        int rc = net_conv_args(n, op, n->max_batch, 0, &ref);
        if (!rc) rc = vgh_conv_prepare(ref);
        if (rc) return rc;
        if (!vgh_conv_cfg_ok_for(cfg, ref)) {
            fprintf(stderr, "[vgh] net_set_cfg: op %d: tile %s cannot run this op at max_batch=%d; its automatic tile %s runs it at every batch size\n", op_index, vgh_conv_cfg_name(cfg),
                    n->max_batch, vgh_conv_cfg_name(op.auto_cfg));
            cfg = -1;
        }
    }
    op.d.force_cfg = cfg;
    return VGH_OK;
}

int vgh_net_op_cfg(vgh_net* n, int op_index) {
    if (!n || op_index < 0 || op_index >= (int)n->ops.size()) return -1;
    const NetOp& op = n->ops[op_index];
    if (op.d.kind != VGH_OP_CONV || n->bufs[op.d.in_buf].is_f32 == VGH_FMT_F32) return -1;  // (fp32 parity nets run the FMA kernel: no tile table)
    return op.d.force_cfg >= 0 ? op.d.force_cfg : op.auto_cfg;
}

static uint16_t* g_zeros[kMaxDevices];  // vgh_conv2d's page of zeros per device, allocated once per device (per_device.h)
static PerDevice g_zeros_made;

int vgh_conv2d(const vgh_conv_call* c, void* stream) {
    VGH_REQUIRE(c && c->in_dev && c->wpack_dev && c->bias_dev && c->out_dev, "conv2d: null argument");
    int dev = 0;
    VGH_HIP(hipGetDevice(&dev));  // (a machine without a device says so here)
    VGH_REQUIRE(device_slot(hipSuccess, dev) != kNoSlot, "conv2d: device index");
    hipError_t zeros_err = hipSuccess;
    once_per_device(g_zeros_made, dev, [&] {
        uint16_t* z = nullptr;
        if ((zeros_err = hipMalloc((void**)&z, 256)) == hipSuccess && (zeros_err = hipMemset(z, 0, 256)) == hipSuccess) g_zeros[dev] = z;
        return zeros_err == hipSuccess ? 1 : 0;
    });
    VGH_HIP(zeros_err);
    VGH_REQUIRE(c->fmt == VGH_FMT_BF16 || c->fmt == VGH_FMT_BF16X2 || c->fmt == VGH_FMT_F16X2 || c->fmt == VGH_FMT_FP8 || c->fmt == VGH_FMT_F16 || c->fmt == VGH_FMT_I8, "conv2d: fmt %d", c->fmt);
    const int in_fp8 = vgh_fmt_q8_kind(c->fmt);
    VGH_REQUIRE(c->out_fp8 >= 0 && c->out_fp8 <= 2 && (!in_fp8 || !c->out_fp8 || in_fp8 == c->out_fp8), "conv2d: out_fp8 is 0, 1 (e4m3) or 2 (int8), and an 8-bit input keeps its format");
    VGH_REQUIRE(!c->diag_dev || (c->fmt == VGH_FMT_I8 && !c->out_fp8 && c->cin >= c->cout_pad && c->cout_pad <= 1024), "conv2d: diag_dev belongs to an int8 -> bf16 conv with cout_pad <= min(cin, 1024)");
    VGH_REQUIRE(!(in_fp8 || c->out_fp8) || (c->gscale_dev && (vgh_fmt_is_q8(c->fmt) || c->fmt == VGH_FMT_BF16) && !c->out_f32), "conv2d: an e4m3 / int8 conv needs gscale_dev, a bf16 or e4m3 input and no fp32 output");
    const int planes = vgh_fmt_planes(c->fmt);
    ConvArgs a;
    conv_args_fill(&a, *c, ConvGeom{c->fmt, c->out_f32, c->out_fp8, c->B, c->H, c->W, c->in_pitch, c->out_pitch, c->res_pitch, c->out_f32 ? 1 : planes, planes});
    a.in = (const uint16_t*)c->in_dev;
    a.out = c->out_dev;
    a.res = (const uint16_t*)c->res_dev;
    a.wpack = (const uint16_t*)c->wpack_dev;
    a.bias = c->bias_dev;
    a.gscale = c->gscale_dev;
    a.dvec = c->diag_dev;
    a.out_scale = c->out_scale;
    a.zeros = g_zeros[dev];
    return vgh_launch_conv(a, c->force_cfg, (hipStream_t)stream);
}

int vgh_pack_conv_weights(const float* w_host, int cout_pad, int ksize, int cin, uint16_t* wpack_host) {
    VGH_REQUIRE(w_host && wpack_host, "pack: null argument");
    VGH_REQUIRE(cin % 32 == 0 && cout_pad % 32 == 0 && (ksize == 1 || ksize == 3), "pack: cin/cout_pad must be multiples of 32, ksize 1 or 3");
    vgh_pack_conv_weights_host(w_host, cout_pad, ksize, cin, wpack_host);
    return VGH_OK;
}

int vgh_pack_conv_weights_fp8(const float* w_host, int cout_pad, int ksize, int cin, uint8_t* wpack_host, float* wscale_host) {
    VGH_REQUIRE(w_host && wpack_host && wscale_host, "pack_fp8: null argument");
    VGH_REQUIRE(cin % 64 == 0 && cout_pad % 32 == 0 && ksize == 3, "pack_fp8: cin must be a multiple of 64, cout_pad of 32, ksize 3");
    vgh_pack_conv_weights_fp8_host(w_host, cout_pad, ksize, cin, wpack_host, wscale_host);
    return VGH_OK;
}
int vgh_net_set_i8_diag(int on) {
    g_i8_diag.store(on ? 1 : 0, std::memory_order_relaxed);
    return VGH_OK;
}
int vgh_net_op_has_diag(vgh_net* n, int op_index) { return (n && op_index >= 0 && op_index < (int)n->ops.size() && n->ops[op_index].dvec) ? 1 : 0; }
int vgh_pack_conv_weights_i8(const float* w_host, int cout_pad, int ksize, int cin, uint8_t* wpack_host, float* wscale_host) {
    VGH_REQUIRE(w_host && wpack_host && wscale_host, "pack_i8: null argument");
    VGH_REQUIRE(cin % 64 == 0 && cout_pad % 32 == 0 && ksize == 3, "pack_i8: cin must be a multiple of 64, cout_pad of 32, ksize 3");
    vgh_pack_conv_weights_i8_host(w_host, cout_pad, ksize, cin, wpack_host, wscale_host);
    return VGH_OK;
}

int vgh_stream_create(int device, void** stream_out) {
    VGH_REQUIRE(stream_out, "stream_create: null");
    VGH_HIP(hipSetDevice(device));
    hipStream_t s;
    VGH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = (void*)s;
    return VGH_OK;
}
int vgh_stream_destroy(void* stream) {
    VGH_HIP(hipStreamDestroy((hipStream_t)stream));
    return VGH_OK;
}
int vgh_stream_sync(void* stream) {
    VGH_HIP(hipStreamSynchronize((hipStream_t)stream));
    return VGH_OK;
}
int vgh_event_create(void** ev_out) {
    VGH_REQUIRE(ev_out, "event_create: null");
    hipEvent_t e;
    VGH_HIP(hipEventCreate(&e));
    *ev_out = (void*)e;
    return VGH_OK;
}
int vgh_event_destroy(void* ev) {
    VGH_HIP(hipEventDestroy((hipEvent_t)ev));
    return VGH_OK;
}
int vgh_event_record(void* ev, void* stream) {
    VGH_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return VGH_OK;
}
int vgh_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out) {
    VGH_REQUIRE(ms_out, "event_elapsed: null");
    VGH_HIP(hipEventSynchronize((hipEvent_t)ev_stop));
    VGH_HIP(hipEventElapsedTime(ms_out, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
    return VGH_OK;
}

}  // extern "C"
