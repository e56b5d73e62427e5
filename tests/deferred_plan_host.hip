// Stand-alone check of the deferrable-op marks and the pending state of csrc/net_plan.h (vgh_net_set_defer / vgh_net_run_deferred).  tests/test_deferred_plan_host.py
// writes the buffer and op descriptors of real programs (arch.build_program) to files and builds this with the host sanitizers (address, undefined); it makes no HIP
// call and runs on the CPU.  Usage: deferred_plan_host FILE...   (one file per program)
//   file: int64 header [image_size, n_bufs, n_ops, n_weights, n_biases, sizeof(buf desc), sizeof(op desc), n_expected], int32 expected op indices [n_expected],
//         the vgh_buf_desc array, the vgh_op_desc array.  The weights are not in the file: the plan reads them only where a K window overhangs a pitch (and then
//         wants zeros), so an all-zero array of the stated length stands in.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../head_detector_amd/csrc/net_plan.h"

static int checks = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        ++checks;                                             \
        if (!(cond)) {                                        \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

struct Prog {
    int image_size = 0;
    std::vector<vgh_buf_desc> bufs;
    std::vector<vgh_op_desc> ops;
    std::vector<float> weights;
    int64_t n_biases = 0;
    std::vector<int> expected;
    int plan(NetPlan* p) const { return net_plan(image_size, 2, bufs.data(), (int)bufs.size(), ops.data(), (int)ops.size(), weights.data(), (int64_t)weights.size(), n_biases, true, p); }
};

static Prog load(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    int64_t h[8];
    CHECK(fread(h, sizeof(int64_t), 8, f) == 8, "%s: short header", path);
    CHECK(h[5] == (int64_t)sizeof(vgh_buf_desc) && h[6] == (int64_t)sizeof(vgh_op_desc), "%s: descriptor sizes %lld / %lld, the header has %zu / %zu", path, (long long)h[5], (long long)h[6],
          sizeof(vgh_buf_desc), sizeof(vgh_op_desc));
    CHECK(h[1] > 0 && h[1] < 4096 && h[2] > 0 && h[2] < 4096 && h[3] > 0 && h[3] < (1ll << 28) && h[7] >= 0 && h[7] < 64, "%s: implausible header", path);
    Prog g;
    g.image_size = (int)h[0];
    g.n_biases = h[4];
    std::vector<int32_t> e((size_t)h[7]);
    CHECK(fread(e.data(), 4, e.size(), f) == e.size(), "%s: short index list", path);
    g.expected.assign(e.begin(), e.end());
    g.bufs.resize((size_t)h[1]);
    g.ops.resize((size_t)h[2]);
    CHECK(fread(g.bufs.data(), sizeof(vgh_buf_desc), g.bufs.size(), f) == g.bufs.size(), "%s: short buffer table", path);
    CHECK(fread(g.ops.data(), sizeof(vgh_op_desc), g.ops.size(), f) == g.ops.size(), "%s: short op table", path);
    fclose(f);
    g.weights.assign((size_t)h[3], 0.0f);
    return g;
}

static std::vector<int> marked(const NetPlan& p) {
    std::vector<int> m;
    for (size_t i = 0; i < p.ops.size(); ++i)
        if (p.ops[i].deferrable) m.push_back((int)i);
    return m;
}

// a plain 1x1 conv, 32 -> 32 channels, from channel 0 of `in_buf` to channel 0 of `out_buf`
static vgh_op_desc conv1x1(int in_buf, int out_buf) {
    vgh_op_desc d{};
    d.kind = VGH_OP_CONV;
    d.in_buf = in_buf;
    d.cin = 32;
    d.out_buf = out_buf;
    d.cout_pad = d.cout_store = d.out_split = 32;
    d.res_buf = -1;
    d.ksize = d.stride = 1;
    d.force_cfg = -1;
    return d;
}

static void check_program(const char* path) {
    const Prog g = load(path);
    NetPlan p;
    CHECK(g.plan(&p) == VGH_OK, "%s: the plan refuses the program: %s", path, p.err);
    const std::vector<int> m = marked(p);
    CHECK(!g.expected.empty() && m == g.expected, "%s: %zu ops marked, %zu expected (first marked %d)", path, m.size(), g.expected.size(), m.empty() ? -1 : m[0]);
    for (int i : m) {
        const vgh_op_desc& d = g.ops[i];
        CHECK(d.ksize == 1 && g.bufs[d.out_buf].is_f32 == VGH_FMT_F32 && d.out_coff >= VGH_PRED_FLAME_OFF, "%s: op %d is marked but is no FLAME prediction conv", path, i);
    }
    // the box / score convs write the same buffers below VGH_PRED_FLAME_OFF and are never marked
    int dense_pred = 0;
    for (size_t i = 0; i < g.ops.size(); ++i)
        dense_pred += g.ops[i].kind == VGH_OP_CONV && g.bufs[g.ops[i].out_buf].is_f32 == VGH_FMT_F32 && g.ops[i].out_coff < VGH_PRED_FLAME_OFF && !p.ops[i].deferrable;
    CHECK(dense_pred >= 1, "%s: no dense prediction conv found", path);

    // a second reader of ONE prediction buffer: the ops that write it lose the mark, the other levels keep theirs
    const int pred0 = g.ops[m[0]].out_buf, some_bf16 = g.ops[m[0]].in_buf;
    int scratch = -1;  // a bf16 buffer that no marked op reads, for the extra op's output
    for (size_t b = 0; b < g.bufs.size() && scratch < 0; ++b) {
        bool used = g.bufs[b].is_f32 != VGH_FMT_BF16 || g.bufs[b].pitch < 32;
        for (int i : m) used = used || g.ops[i].in_buf == (int)b;
        if (!used) scratch = (int)b;
    }
    CHECK(scratch >= 0, "%s: no scratch buffer", path);
    {
        Prog r = g;
        r.ops.push_back(conv1x1(pred0, scratch));
        NetPlan pr;
        CHECK(r.plan(&pr) == VGH_OK, "%s: second reader: %s", path, pr.err);
        std::vector<int> want;
        for (int i : m)
            if (g.ops[i].out_buf != pred0) want.push_back(i);
        CHECK(want.size() < m.size() && marked(pr) == want, "%s: a second reader of buffer %d leaves %zu marks, expected %zu", path, pred0, marked(pr).size(), want.size());
    }
    {  // ... and as a residual
        Prog r = g;
        vgh_op_desc d = conv1x1(scratch, scratch);
        d.res_buf = pred0;
        r.ops.push_back(d);
        NetPlan pr;
        CHECK(r.plan(&pr) == VGH_OK, "%s: residual reader: %s", path, pr.err);
        for (int i : marked(pr)) CHECK(g.ops[i].out_buf != pred0, "%s: op %d keeps its mark although buffer %d is added as a residual", path, i, pred0);
    }
    {  // a later op that rewrites the input of a marked op: its rows could not be computed afterwards
        Prog r = g;
        r.ops.push_back(conv1x1(scratch, some_bf16));
        NetPlan pr;
        CHECK(r.plan(&pr) == VGH_OK, "%s: late writer: %s", path, pr.err);
        for (int i : marked(pr)) CHECK(g.ops[i].in_buf != some_bf16, "%s: op %d keeps its mark although a later op rewrites its input", path, i);
        CHECK(marked(pr).size() < m.size(), "%s: late writer changes nothing", path);
    }
    {  // an op another lane waits for is not deferred (its event would never be recorded)
        Prog r = g;
        vgh_op_desc d = conv1x1(scratch, scratch);
        d.lane = 1 | ((m[0] + 1) << 8);
        r.ops.push_back(d);
        NetPlan pr;
        CHECK(r.plan(&pr) == VGH_OK, "%s: awaited op: %s", path, pr.err);
        CHECK(pr.ops[m[0]].ev_done == 1 && pr.ops[m[0]].deferrable == 0 && marked(pr).size() == m.size() - 1, "%s: an awaited op keeps its mark", path);
    }
}

static void check_state() {
    DeferState s;
    // switch off: forwards run everything, nothing is ever pending
    s.forward(3, s.skip());
    CHECK(!s.pending && s.take() == 0, "off: pending");
    s.on = true;
    // forward, run_deferred, forward, forward, run_deferred
    s.forward(3, s.skip());
    CHECK(s.pending && s.B == 3, "forward leaves the ops pending");
    CHECK(s.take() == 3 && !s.pending, "run_deferred takes the batch of that forward");
    CHECK(s.take() == 0, "run_deferred is idempotent");
    s.forward(4, s.skip());
    s.forward(5, s.skip());
    CHECK(s.pending && s.take() == 5, "the later forward's batch replaces the earlier one's");
    CHECK(s.take() == 0 && !s.pending, "nothing pending after the second run");
    // a forward that runs every op (the profiler) clears a pending mark; so does the switch turned off before the next forward
    s.forward(6, s.skip());
    s.forward(6, false);
    CHECK(!s.pending && s.take() == 0, "a dense forward leaves nothing pending");
    s.forward(7, s.skip());
    s.on = false;
    CHECK(s.pending && s.take() == 7, "turning the switch off does not drop what an earlier forward left pending");
    s.forward(8, s.skip());
    CHECK(!s.pending && s.take() == 0, "off again");
    s.on = true;
    s.forward(0, s.skip());
    CHECK(s.take() == 0, "an empty batch has nothing to run");
}

int main(int argc, char** argv) {
    CHECK(argc >= 2, "usage: deferred_plan_host FILE...");
    for (int i = 1; i < argc; ++i) check_program(argv[i]);
    check_state();
    printf("deferred plan host checks passed (%d checks)\n", checks);
    return 0;
}
