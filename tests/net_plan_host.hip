// Stand-alone check of csrc/net_plan.h (what vgh_net_create decides about a program before its first HIP call: validation, arena and weight-blob layout, fusion
// marks, cross-lane events, the lane split, the descriptor -> ConvArgs filler).  tests/test_net_plan_host.py builds it with the host sanitizers (address, undefined),
// as the product and with -DVGH_EXPERIMENTS, and runs it on its own.  It makes no HIP call.
// EVERY EXPECTED VALUE BELOW IS WORKED OUT BY HAND IN THE COMMENT NEXT TO IT, none was printed by the code under test.
#include <stdio.h>
#include <stdlib.h>

#include "../head_detector_amd/csrc/net_plan.h"

static int failures = 0, checks = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        ++checks;                         \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            if (failures > 20) exit(1);   \
        }                                 \
    } while (0)

static const std::vector<float> kZeros(120000, 0.0f);  // the weights of every program unless it brings its own; all offsets 0
static const int64_t kBiases = 256;

static vgh_buf_desc buf(int h, int w, int pitch, int fmt, float scale = 0.0f) { return vgh_buf_desc{h, w, pitch, fmt, scale}; }
static vgh_op_desc conv(int in_buf, int cin, int out_buf, int cout, int ksize, int stride) {  // dense, ReLU, no residual, whole channels at offset 0
    vgh_op_desc d;
    memset(&d, 0, sizeof(d));
    d.kind = VGH_OP_CONV;
    d.in_buf = in_buf, d.cin = cin, d.out_buf = out_buf, d.cout_pad = d.cout_store = d.out_split = cout;
    d.res_buf = -1, d.ksize = ksize, d.stride = stride, d.act = VGH_ACT_RELU, d.force_cfg = -1;
    return d;
}
static vgh_op_desc stem(int out_buf) {
    vgh_op_desc d = conv(0, 0, out_buf, 64, 3, 2);
    d.kind = VGH_OP_STEM, d.cout_store = 48;
    return d;
}
static vgh_op_desc pool(int buf_id, int cin) {
    vgh_op_desc d = conv(buf_id, cin, buf_id, 0, 0, 0);
    d.kind = VGH_OP_SPP_POOL;
    return d;
}
static vgh_op_desc on_lane(vgh_op_desc d, int lane, int waits_for = -1) {
    d.lane = lane | (waits_for + 1) << 8;
    return d;
}

struct Program {
    std::vector<vgh_buf_desc> bufs;
    std::vector<vgh_op_desc> ops;
    int image_size = 32, max_batch = 1;
    const float* weights = kZeros.data();
    int64_t n_weights = (int64_t)kZeros.size(), n_biases = kBiases;
    bool i8_diag = true;
    int plan(NetPlan* p) const { return net_plan(image_size, max_batch, bufs.data(), (int)bufs.size(), ops.data(), (int)ops.size(), weights, n_weights, n_biases, i8_diag, p); }
};

static void check_layout() {
    // one buffer of each format class, max_batch = 3.  bytes = 3 * h * w * pitch * element bytes; slab = the next multiple of 256 at or above bytes + 256
    Program g;
    g.max_batch = 3;
    g.bufs = {buf(8, 8, 48, VGH_FMT_BF16),         // 0: 3 * 64 * 48 * 2 = 18432, slab 18688, at 0
              buf(4, 4, 40, VGH_FMT_F32),          // 1: 3 * 16 * 40 * 4 = 7680, slab 7936, at 18688
              buf(4, 4, 32, VGH_FMT_BF16X2),       // 2: 3 * 16 * 32 * 4 (two 2-byte planes) = 6144, slab 6400, at 26624
              buf(4, 4, 64, VGH_FMT_FP8, 0.5f),    // 3: 3 * 16 * 64 * 1 = 3072, slab 3328, at 33024
              buf(2, 2, 104, VGH_FMT_BF16),        // 4: 3 * 4 * 104 * 2 = 2496, + 256 = 2752 -> slab 2816 (the one that is rounded up), at 36352
              buf(4, 4, 64, VGH_FMT_BF16)};        // 5: 3 * 16 * 64 * 2 = 6144, slab 6400, at 39168; total 45568
    g.ops = {stem(0),                    // 0: w 27 * 48 * 4 = 5184 -> 5376 at 0; bias 64 * 4 = 256 at 5376; next 5632
             conv(0, 32, 5, 64, 3, 2),   // 1: bf16 in: 64 * 9 * 32 * 2 = 36864 at 5632; bias 256 at 42496; next 42752
             conv(5, 64, 3, 64, 3, 1),   // 2: bf16 in, e4m3 out: 64 * 9 * 64 * 2 = 73728 at 42752; bias at 116480; gscale 256 at 116736; next 116992
             conv(3, 64, 5, 32, 3, 1),   // 3: e4m3 in: 32 * 9 * 64 * 1 = 18432 at 116992; bias 128 -> 256 at 135424; gscale at 135680; next 135936
             conv(1, 32, 1, 32, 1, 1),   // 4: fp32 in: 32 * 32 * 4 = 4096 at 135936; bias at 140032; next 140288
             conv(2, 32, 2, 32, 1, 1),   // 5: two-plane in: 32 * 32 * 6 = 6144 at 140288; bias at 146432; next 146688
             pool(4, 32),                // 6: nothing in the blob
             conv(4, 32, 4, 96, 1, 1)};  // 7: bf16 in: 96 * 32 * 2 = 6144 at 146688; bias 384 -> 512 at 152832; total 153344
    g.ops[3].out_coff = 32;
    g.ops[7].out_coff = 8;
    NetPlan p;
    EXPECT(g.plan(&p) == VGH_OK, "layout program: %s", p.err);
    const int64_t off[6] = {0, 18688, 26624, 33024, 36352, 39168}, bytes[6] = {18432, 7680, 6144, 3072, 2496, 6144};
    for (int i = 0; i < 6; ++i) EXPECT(p.buf_off[i] == off[i] && p.buf_bytes[i] == bytes[i], "buffer %d: at %lld, %lld bytes", i, (long long)p.buf_off[i], (long long)p.buf_bytes[i]);
    EXPECT(p.arena_bytes == 45568, "arena %lld", (long long)p.arena_bytes);
    const int64_t w[8] = {0, 5632, 42752, 116992, 135936, 140288, 0, 146688}, b[8] = {5376, 42496, 116480, 135424, 140032, 146432, 0, 152832};
    const int64_t gs[8] = {-1, -1, 116736, 135680, -1, -1, -1, -1};
    for (int i = 0; i < 8; ++i) {
        const NetPlan::Op& o = p.ops[i];
        EXPECT(o.w == w[i] && o.bias == b[i] && o.gscale == gs[i] && o.dvec == -1, "op %d: w %lld bias %lld gscale %lld dvec %lld", i, (long long)o.w, (long long)o.bias, (long long)o.gscale, (long long)o.dvec);
        EXPECT(o.b2b == 0 && o.overhang_ok == 0 && o.ev_done == 0, "op %d marks", i);
    }
    EXPECT(p.blob_bytes == 153344 && p.wds == -1 && p.stem_pair == -1 && !p.lane_wait_cycle, "blob %lld, wds %lld, stem_pair %d", (long long)p.blob_bytes, (long long)p.wds, p.stem_pair);

    // int8 -> bf16 3x3 conv whose rows all have w[c][centre][c] as their largest weight: the diagonal bypass, behind gscale -- and not with the process-wide switch off
    std::vector<float> wid((size_t)64 * 9 * 64, 0.0f);
    for (int c = 0; c < 64; ++c) wid[(size_t)c * 9 * 64 + 4 * 64 + c] = 1.0f, wid[(size_t)c * 9 * 64 + 3] = -0.5f;
    Program q;
    q.bufs = {buf(4, 4, 64, VGH_FMT_I8, 0.1f), buf(4, 4, 64, VGH_FMT_BF16)};
    q.ops = {conv(0, 64, 1, 64, 3, 1)};  // w 64 * 9 * 64 * 1 = 36864 at 0; bias at 36864; gscale at 37120; dvec at 37376; total 37632
    q.weights = wid.data(), q.n_weights = (int64_t)wid.size();
    NetPlan pq;
    EXPECT(q.plan(&pq) == VGH_OK && pq.ops[0].bias == 36864 && pq.ops[0].gscale == 37120 && pq.ops[0].dvec == 37376 && pq.blob_bytes == 37632, "int8 diag: %s, dvec %lld", pq.err, (long long)pq.ops[0].dvec);
    q.i8_diag = false;
    NetPlan pq0;
    EXPECT(q.plan(&pq0) == VGH_OK && pq0.ops[0].gscale == 37120 && pq0.ops[0].dvec == -1 && pq0.blob_bytes == 37376, "int8 diag switched off: dvec %lld", (long long)pq0.ops[0].dvec);
    q.i8_diag = true;
    for (int c = 0; c < 33; ++c) wid[(size_t)c * 9 * 64 + 3] = -2.0f;  // 33 of 64 live rows now have a larger weight elsewhere: fewer than half are dominated
    NetPlan pq1;
    EXPECT(q.plan(&pq1) == VGH_OK && pq1.ops[0].dvec == -1, "int8 diag, 31 of 64 rows dominated");
}

static void refused(const char* what, const Program& g, const char* needle) {
    NetPlan p;
    const int rc = g.plan(&p);
    EXPECT(rc == VGH_ERR_INVALID && strstr(p.err, needle), "%s: rc %d, message \"%s\", expected \"%s\"", what, rc, p.err, needle);
}

// the program of test_stem_tensor_at_its_48_channel_pitch in miniature: a 48-pitch bf16 buffer read as cin = 64
static Program overhang_program(std::vector<float>& w) {
    Program g;
    g.bufs = {buf(8, 8, 48, VGH_FMT_BF16), buf(8, 8, 32, VGH_FMT_BF16)};
    g.ops = {conv(0, 64, 1, 32, 1, 1)};
    w.assign((size_t)32 * 64, 0.0f);
    for (int r = 0; r < 32; ++r)
        for (int c = 0; c < 48; ++c) w[(size_t)r * 64 + c] = 1.0f + c;  // the live columns may hold anything
    g.weights = w.data(), g.n_weights = (int64_t)w.size();
    return g;
}

static void check_refusals() {
    Program ok;  // the base every refusal is one edit away from
    ok.bufs = {buf(16, 16, 48, VGH_FMT_BF16), buf(16, 16, 64, VGH_FMT_BF16)};
    ok.ops = {stem(0), conv(0, 32, 1, 64, 3, 1), pool(1, 32)};
    NetPlan p;
    EXPECT(ok.plan(&p) == VGH_OK && p.err[0] == 0, "base program: %s", p.err);
    Program g = ok;
    {
        NetPlan pn;
        const int rc = net_plan(32, 1, g.bufs.data(), -1, g.ops.data(), 3, g.weights, g.n_weights, g.n_biases, true, &pn);
        EXPECT(rc == VGH_ERR_INVALID && strstr(pn.err, "negative buffer or op count"), "negative n_bufs: %s", pn.err);
    }
    g.bufs[1].is_f32 = 7;
    refused("format 7", g, "buffer 1 has unknown format 7");
    g = ok, g.bufs[1].is_f32 = -1;
    refused("format -1", g, "buffer 1 has unknown format -1");
    g = ok, g.bufs[1] = buf(16, 16, 64, VGH_FMT_FP8, 0.0f);
    refused("e4m3 without a scale", g, "8-bit buffer 1 needs a positive scale");
    g = ok, g.bufs[1] = buf(16, 16, 72, VGH_FMT_I8, 0.5f);
    refused("int8 pitch 72", g, "8-bit buffer 1 needs a positive scale and a pitch that is a multiple of 16");
    g = ok, g.ops[1].cin = 48;
    refused("cin 48", g, "op 1 channel padding");
    g = ok, g.ops[1].cout_pad = 40;
    refused("cout_pad 40", g, "op 1 channel padding");
    g = ok, g.ops[1].in_buf = 2;
    refused("conv in_buf", g, "op 1 buffer ids");
    g = ok, g.ops[1].out_buf = -1;
    refused("conv out_buf", g, "op 1 buffer ids");
    g = ok, g.ops[1].res_buf = 2;
    refused("conv res_buf", g, "op 1 buffer ids");
    g = ok, g.n_weights = 64 * 9 * 32 - 1;
    refused("weights one short", g, "op 1 weight range");
    g = ok, g.ops[1].w_off = -1;
    refused("w_off -1", g, "op 1 weight range");
    g = ok, g.ops[1].b_off = kBiases - 63;
    refused("bias one short", g, "op 1 weight range");
    g = ok, g.ops[1].b_off = -1;
    refused("conv b_off -1", g, "op 1 weight range");
    g = ok, g.ops[0].out_buf = 2;
    refused("stem out_buf (new rule)", g, "op 0 buffer ids");
    g = ok, g.n_weights = 27 * 48 - 1, g.ops = {stem(0)};
    refused("stem weights one short", g, "stem weight range");
    g = ok, g.ops[0].b_off = kBiases - 47;
    refused("stem bias one short", g, "stem weight range");
    g = ok, g.ops[0].b_off = -1;
    refused("stem b_off -1 (new rule)", g, "stem weight range");
    g = ok, g.ops[2].in_buf = -1;
    refused("pool in_buf -1 (new rule)", g, "op 2 buffer ids");
    g = ok, g.ops[2].in_buf = 2;
    refused("pool in_buf 2 (new rule)", g, "op 2 buffer ids");
    g = ok, g.ops[1] = on_lane(g.ops[1], 1, 1);
    refused("waits for itself", g, "op 1 waits for op 1, which does not precede it");
    g = ok, g.ops[1] = on_lane(g.ops[1], 1, 2);
    refused("waits for a later op", g, "op 1 waits for op 2, which does not precede it");
    g = ok, g.ops[2] = on_lane(g.ops[2], 1, 3);
    refused("waits for an op past the program", g, "op 2 waits for op 3, which does not precede it");
    g = ok, g.ops[1].lane = -256;  // bits 8+ = -1: producer index -2 (new rule: the index has a lower bound)
    refused("negative producer", g, "op 1 waits for op -2, which does not precede it");

    // the K window past the pitch
    std::vector<float> w;
    Program o = overhang_program(w);
    NetPlan po;
    EXPECT(o.plan(&po) == VGH_OK && po.ops[0].overhang_ok == 1, "48 channels read as 64 over zero columns: %s", po.err);
    w[(size_t)17 * 64 + 50] = -0.0f;  // a zero of either sign is a zero
    EXPECT(o.plan(&po) == VGH_OK, "-0.0 at channel 50");
    w[(size_t)17 * 64 + 50] = 1e-30f;
    refused("non-zero weight at channel 50", o, "op 0 reads 64 channels of a 48-channel pitch with a non-zero weight at input channel 50");
    w[(size_t)17 * 64 + 50] = 0.0f;
    o.bufs[0].is_f32 = VGH_FMT_BF16X2;
    refused("two-plane buffer past its pitch", o, "op 0 reads past the pitch of buffer 0");
    o.bufs[0].is_f32 = VGH_FMT_BF16, o.ops[0].in_coff = 48;
    refused("window that starts at the pitch", o, "op 0 reads past the pitch of buffer 0");
    o.ops[0].in_coff = 0, o.ops[0].grp_cout = 32, o.ops[0].grp_in_stride = 0;  // a grouped conv is not this rule's business (net_conv_args refuses it at the launch)
    EXPECT(o.plan(&po) == VGH_OK && po.ops[0].overhang_ok == 0, "grouped conv: %s", po.err);
}

// stem -> 3x3 / s2 / 64 -> 96 -> 1x1 / 96 -> 128 on a 32 x 32 image
static Program stage1_chain() {
    Program g;
    g.bufs = {buf(16, 16, 48, VGH_FMT_BF16), buf(8, 8, 96, VGH_FMT_BF16), buf(8, 8, 128, VGH_FMT_BF16)};
    g.ops = {stem(0), conv(0, 64, 1, 96, 3, 2), conv(1, 96, 2, 128, 1, 1)};
    return g;
}

static void check_pairs() {
    Program g = stage1_chain();
    NetPlan p;
    EXPECT(g.plan(&p) == VGH_OK && p.stem_pair == 0 && p.ops[0].b2b == 0 && p.ops[1].b2b == 1 && p.ops[2].b2b == 2 && p.ops[1].overhang_ok == 1, "chain: %s, stem_pair %d, b2b %d %d %d", p.err, p.stem_pair,
           p.ops[0].b2b, p.ops[1].b2b, p.ops[2].b2b);
    // blob: stem w at 0, bias at 5376; op 1: 96 * 9 * 64 * 2 = 110592 at 5632, bias 384 -> 512 at 116224; op 2: 128 * 96 * 2 = 24576 at 116736, bias 512 at 141312; 141824.
    // The experiments build appends the downsample's second image, 9 * 3 * 96 * 16 * 2 = 82944 bytes, behind every op: 224768
    EXPECT(p.ops[1].w == 5632 && p.ops[1].bias == 116224 && p.ops[2].w == 116736 && p.ops[2].bias == 141312, "chain offsets");
#ifdef VGH_EXPERIMENTS
    EXPECT(p.wds == 141824 && p.blob_bytes == 224768, "wds %lld, blob %lld", (long long)p.wds, (long long)p.blob_bytes);
#else
    EXPECT(p.wds == -1 && p.blob_bytes == 141824, "wds %lld, blob %lld", (long long)p.wds, (long long)p.blob_bytes);
#endif
    // a second reader of the middle tensor: no b2b pair (the stem pair is another tensor's business)
    Program r = g;
    r.ops.push_back(conv(1, 96, 2, 128, 1, 1));
    NetPlan pr;
    EXPECT(r.plan(&pr) == VGH_OK && pr.stem_pair == 0 && pr.ops[1].b2b == 0 && pr.ops[2].b2b == 0 && pr.ops[3].b2b == 0, "second reader: b2b %d %d %d", pr.ops[1].b2b, pr.ops[2].b2b, pr.ops[3].b2b);
    r = g, r.ops.push_back(conv(2, 128, 2, 128, 1, 1)), r.ops[3].res_buf = 1;  // ... as a residual
    EXPECT(r.plan(&pr) == VGH_OK && pr.ops[1].b2b == 0 && pr.ops[2].b2b == 0, "residual reader");
    // a second reader of the STEM tensor: no stem pair, the b2b pair stays
    r = g, r.ops.push_back(pool(0, 32));
    EXPECT(r.plan(&pr) == VGH_OK && pr.stem_pair == -1 && pr.wds == -1 && pr.ops[1].b2b == 1 && pr.ops[2].b2b == 2, "pool on the stem tensor: stem_pair %d", pr.stem_pair);
    // only the first stem -> conv adjacency is looked at, and a 4-divisible image is asked for (image_size is a multiple of 32 in every accepted program)
    r = g, r.ops[1].cout_store = 88;
    EXPECT(r.plan(&pr) == VGH_OK && pr.stem_pair == -1 && pr.ops[1].b2b == 0, "88 stored channels");
    // two pairs in a row: (1, 2) and (4, 5); an op is in one pair at most.  (Two candidate pairs that OVERLAP on one op cannot be written down: the first conv of a
    // pair has 96 couts and the second 128 / 192 / 256 -- vgh_conv_b2b_ok --, so no op qualifies as both; the plan keeps the parent's `b2b == 0` term all the same.)
    r = g;
    r.bufs.push_back(buf(4, 4, 96, VGH_FMT_BF16)), r.bufs.push_back(buf(4, 4, 192, VGH_FMT_BF16));
    r.ops.push_back(pool(2, 128)), r.ops.push_back(conv(2, 128, 3, 96, 3, 2)), r.ops.push_back(conv(3, 96, 4, 192, 1, 1));
    EXPECT(r.plan(&pr) == VGH_OK && pr.ops[1].b2b == 1 && pr.ops[2].b2b == 2 && pr.ops[3].b2b == 0 && pr.ops[4].b2b == 1 && pr.ops[5].b2b == 2, "two pairs: %s", pr.err);
    r.ops[5].cout_pad = r.ops[5].cout_store = r.ops[5].out_split = 160;  // not a cout2 the b2b tile has
    EXPECT(r.plan(&pr) == VGH_OK && pr.ops[4].b2b == 0 && pr.ops[5].b2b == 0, "cout2 160");
}

static void check_lanes() {
    Program g;
    g.bufs = {buf(4, 4, 32, VGH_FMT_BF16)};
    const vgh_op_desc c = conv(0, 32, 0, 32, 1, 1);
    NetPlan p;
    g.ops = {c, on_lane(c, 1), on_lane(c, 2, 1), on_lane(c, 1, 2)};  // lane 2 waits for lane 1, lane 1 for lane 2
    EXPECT(g.plan(&p) == VGH_OK && p.lane_wait_cycle, "1 -> 2 -> 1");
    EXPECT(!p.ops[0].ev_done && p.ops[1].ev_done && p.ops[2].ev_done && !p.ops[3].ev_done, "events behind ops 1 and 2");
    NetPlan p3;
    g.ops = {c, on_lane(c, 1), on_lane(c, 2, 1), on_lane(c, 3, 2)};  // a chain
    EXPECT(g.plan(&p3) == VGH_OK && !p3.lane_wait_cycle, "1 -> 2 -> 3");
    NetPlan p0;
    g.ops = {c, on_lane(c, 1, 0), on_lane(c, 0, 1), on_lane(c, 1, 2)};  // lane 1 and lane 0 wait for each other: the caller's stream never counts
    EXPECT(g.plan(&p0) == VGH_OK && !p0.lane_wait_cycle && p0.ops[0].ev_done && p0.ops[1].ev_done && p0.ops[2].ev_done, "waits on lane 0");
    NetPlan pt;
    g.ops = {c, on_lane(c, 1), on_lane(c, 2, 1), on_lane(c, 3, 2), on_lane(c, 1, 3)};  // 2 -> 1, 3 -> 2, 1 -> 3: a cycle through three lanes
    EXPECT(g.plan(&pt) == VGH_OK && pt.lane_wait_cycle, "1 -> 2 -> 3 -> 1");
    for (int B = 1; B <= 9; ++B)
        for (int L = 1; L <= 4; ++L) {
            int sum = 0;
            for (int l = 0; l < L; ++l) {
                const int r = rows_of_lane(B, L, l);
                sum += r;
                EXPECT(r == B / L || r == B / L + 1, "B %d L %d lane %d: %d rows", B, L, l, r);
                EXPECT(l == 0 || r <= rows_of_lane(B, L, l - 1), "B %d L %d: lane %d has more rows than lane %d", B, L, l, l - 1);
            }
            EXPECT(sum == B, "B %d L %d: %d rows in all", B, L, sum);
        }
    EXPECT(rows_of_lane(3, 2, 0) == 2 && rows_of_lane(3, 2, 1) == 1 && rows_of_lane(9, 4, 0) == 3 && rows_of_lane(9, 4, 1) == 2 && rows_of_lane(9, 4, 3) == 2, "3 over 2, 9 over 4");
}

#define CONV_ARGS_FIELDS(F)                                                                                                                                                                    \
    F(in) F(wpack) F(bias) F(out) F(res) F(zeros) F(in_pitch) F(out_pitch) F(res_pitch) F(in_coff) F(out_coff) F(out_coff2) F(out_split) F(res_coff) F(B) F(H) F(W) F(Ho) F(Wo) F(cin) F(cout_pad)  \
    F(cout_store) F(ksize) F(stride) F(pad) F(act) F(out_f32) F(shuffle) F(shuffle_c) F(alpha) F(P) F(nkb) F(cblocks) F(div_howo_m) F(div_howo_s) F(div_wo_m) F(div_wo_s) F(fast_epi) F(stagger)      \
    F(grid_share) F(grp_cout) F(grp_in_stride) F(split) F(in_plane) F(out_plane) F(res_plane) F(seg_kb) F(nseg) F(acc_scale) F(lo_scale) F(out_scale) F(in_fp8) F(out_fp8) F(gscale) F(dvec)      \
    F(bias_scale) F(fallback_cfg1) F(nt_out) F(w2pack) F(bias2) F(out2) F(out2_pitch) F(out2_coff) F(out2_coff2) F(out2_split) F(cout2_pad) F(cout2_store) F(act2) F(b2b_igemm) F(ablate) F(trace)
static void same_args(const char* what, const ConvArgs& got, const ConvArgs& want) {
#define SAME(f) EXPECT(got.f == want.f, "%s: field %s", what, #f);
    CONV_ARGS_FIELDS(SAME)
#undef SAME
    EXPECT(memcmp(&got, &want, sizeof(ConvArgs)) == 0, "%s: a field the list above does not name", what);  // (both start from memset 0, padding included)
}

static void check_filler() {
    ConvArgs got, e;
    memset(&got, 0xff, sizeof(got));  // the filler owns every byte
    // bf16 3x3 / stride 1 with a residual, the executor's descriptor: 3 images of 20 x 12, ragged channel layout
    vgh_op_desc d = conv(0, 64, 1, 96, 3, 1);
    d.in_coff = 8, d.out_coff = 16, d.cout_store = 88, d.out_split = 64, d.out_coff2 = 128, d.res_buf = 2, d.res_coff = 4, d.alpha = 0.5f;
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_BF16, 0, 0, 3, 20, 12, 72, 256, 104, 1, 1});
    memset(&e, 0, sizeof(e));
    e.nseg = 3, e.in_plane = 72, e.out_plane = 256, e.res_plane = 104;  // split 0: the plane strides are carried but not used
    e.in_pitch = 72, e.out_pitch = 256, e.res_pitch = 104, e.in_coff = 8, e.out_coff = 16, e.out_coff2 = 128, e.out_split = 64, e.res_coff = 4;
    e.B = 3, e.H = 20, e.W = 12, e.pad = 1, e.Ho = 20, e.Wo = 12;  // (20 + 2 - 3) / 1 + 1, (12 + 2 - 3) / 1 + 1
    e.cin = 64, e.cout_pad = 96, e.cout_store = 88, e.ksize = 3, e.stride = 1, e.act = VGH_ACT_RELU, e.alpha = 0.5f;
    e.P = 720, e.cblocks = 2, e.nkb = 18;  // 3 * 20 * 12; 64 / 32; 9 * 2
    same_args("bf16 3x3 with residual", got, e);

    // two-plane fp16, vgh_conv2d's descriptor: 1x1 on 2 images of 5 x 7, no residual (its pitch 0), 16-bit output
    vgh_conv_call c;
    memset(&c, 0, sizeof(c));
    c.cin = 32, c.cout_pad = c.cout_store = c.out_split = 32, c.ksize = 1, c.stride = 1, c.act = VGH_ACT_NONE, c.in_coff = 8;
    conv_args_fill(&got, c, ConvGeom{VGH_FMT_F16X2, 0, 0, 2, 5, 7, 40, 48, 0, 2, 2});
    memset(&e, 0, sizeof(e));
    e.split = VGH_FMT_F16X2, e.nseg = 3, e.in_plane = 40, e.out_plane = 48, e.in_pitch = 80, e.out_pitch = 96, e.in_coff = 8;  // physical pitch = 2 planes
    e.B = 2, e.H = 5, e.W = 7, e.Ho = 5, e.Wo = 7, e.cin = 32, e.cout_pad = 32, e.cout_store = 32, e.out_split = 32, e.ksize = 1, e.stride = 1;  // pad 0
    e.P = 70, e.cblocks = 1, e.nkb = 1;
    same_args("two-plane 1x1", got, e);
    // ... the same writing an fp32 prediction buffer: one output plane, and a two-plane residual of pitch 24
    conv_args_fill(&got, c, ConvGeom{VGH_FMT_F16X2, 1, 0, 2, 5, 7, 40, 48, 24, 1, 2});
    e.out_f32 = 1, e.out_pitch = 48, e.res_pitch = 48, e.res_plane = 24;
    same_args("two-plane 1x1 -> fp32", got, e);

    // single-plane fp16: 3x3 / stride 2 on a 15 x 9 map -> (15 + 2 - 3) / 2 + 1 = 8, (9 + 2 - 3) / 2 + 1 = 5
    d = conv(0, 32, 1, 64, 3, 2);
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_F16, 0, 0, 1, 15, 9, 32, 64, 64, 1, 1});
    memset(&e, 0, sizeof(e));
    e.split = VGH_FMT_F16X2, e.nseg = 1;  // the F16X2 kernels with one segment; every plane stride 0
    e.in_pitch = 32, e.out_pitch = 64, e.res_pitch = 64, e.B = 1, e.H = 15, e.W = 9, e.pad = 1, e.Ho = 8, e.Wo = 5;
    e.cin = 32, e.cout_pad = 64, e.cout_store = 64, e.out_split = 64, e.ksize = 3, e.stride = 2, e.act = VGH_ACT_RELU;
    e.P = 40, e.cblocks = 1, e.nkb = 9;
    same_args("single-plane fp16 3x3 / s2", got, e);

    // e4m3 in, e4m3 out: 64-byte channel blocks hold 64 channels
    d = conv(0, 128, 1, 64, 3, 1);
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_FP8, 0, 1, 2, 8, 8, 128, 64, 0, 1, 0});
    memset(&e, 0, sizeof(e));
    e.nseg = 3, e.in_plane = 128, e.out_plane = 64, e.in_pitch = 128, e.out_pitch = 64, e.in_fp8 = 1, e.out_fp8 = 1;
    e.B = 2, e.H = 8, e.W = 8, e.pad = 1, e.Ho = 8, e.Wo = 8, e.cin = 128, e.cout_pad = 64, e.cout_store = 64, e.out_split = 64, e.ksize = 3, e.stride = 1, e.act = VGH_ACT_RELU;
    e.P = 128, e.cblocks = 2, e.nkb = 18;  // 128 / 64; 9 * 2
    same_args("e4m3 3x3", got, e);
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_I8, 0, 0, 2, 8, 8, 128, 64, 0, 1, 0});  // int8 in, bf16 out
    e.in_fp8 = 2, e.out_fp8 = 0;
    same_args("int8 3x3", got, e);

    // ConvTranspose2d(k = 2, s = 2) as a 1x1 conv with a pixel-shuffle store: cout_pad = 4 * 32
    d = conv(0, 64, 1, 128, 1, 1);
    d.shuffle = 1, d.act = VGH_ACT_NONE;
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_BF16, 0, 0, 1, 4, 6, 64, 32, 0, 1, 0});
    memset(&e, 0, sizeof(e));
    e.nseg = 3, e.in_plane = 64, e.out_plane = 32, e.in_pitch = 64, e.out_pitch = 32, e.B = 1, e.H = 4, e.W = 6, e.Ho = 4, e.Wo = 6;
    e.cin = 64, e.cout_pad = 128, e.cout_store = 128, e.out_split = 128, e.ksize = 1, e.stride = 1, e.shuffle = 1, e.shuffle_c = 32;
    e.P = 24, e.cblocks = 2, e.nkb = 2;
    same_args("pixel shuffle", got, e);

    // a grouped conv carries its two fields
    d = conv(0, 32, 1, 128, 3, 1);
    d.grp_cout = 64, d.grp_in_stride = 32;
    conv_args_fill(&got, d, ConvGeom{VGH_FMT_BF16, 0, 0, 1, 8, 8, 64, 128, 0, 1, 0});
    EXPECT(got.grp_cout == 64 && got.grp_in_stride == 32 && got.cblocks == 1 && got.nkb == 9, "grouped");
}

int main() {
    check_layout();
    check_refusals();
    check_pairs();
    check_lanes();
    check_filler();
    if (failures) return 1;
    printf("net_plan host checks passed (%d checks)\n", checks);
    return 0;
}
