// Stand-alone check of the tower-deferrable marks of csrc/tower_plan.h (the second mark of vgh_net_set_defer) and of the chain traits of csrc/conv_tiles.h.
// tests/test_tower_plan_host.py writes the buffer and op descriptors of real programs (arch.build_program) to files and builds this with the host sanitizers (address,
// undefined); it makes no HIP call and runs on the CPU.  Usage: tower_plan_host FILE...   (one file per program)
//   file: int64 header [image_size, n_bufs, n_ops, n_weights, n_biases, sizeof(buf desc), sizeof(op desc), n_towers, n_preds, depth], int32 op indices of the expected
//         tower ops [n_towers] and of the expected deferrable 1x1 convs [n_preds], the vgh_buf_desc array, the vgh_op_desc array.  All-zero weights stand in.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../head_detector_amd/csrc/tower_plan.h"

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
    int image_size = 0, depth = 0;
    std::vector<vgh_buf_desc> bufs;
    std::vector<vgh_op_desc> ops;
    std::vector<float> weights;
    int64_t n_biases = 0;
    std::vector<int> towers, preds;
    // what vgh_net_create does: the plan, then the second mark on top of it
    int plan(NetPlan* p, TowerPlan* tp) const {
        const int rc = net_plan(image_size, 2, bufs.data(), (int)bufs.size(), ops.data(), (int)ops.size(), weights.data(), (int64_t)weights.size(), n_biases, true, p);
        if (rc == VGH_OK) net_plan_towers(bufs.data(), ops.data(), (int)ops.size(), p, tp);
        return rc;
    }
};

static Prog load(const char* path) {
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    int64_t h[10];
    CHECK(fread(h, sizeof(int64_t), 10, f) == 10, "%s: short header", path);
    CHECK(h[5] == (int64_t)sizeof(vgh_buf_desc) && h[6] == (int64_t)sizeof(vgh_op_desc), "%s: descriptor sizes", path);
    CHECK(h[1] > 0 && h[1] < 4096 && h[2] > 0 && h[2] < 4096 && h[3] > 0 && h[3] < (1ll << 28) && h[7] >= 0 && h[7] < 64 && h[8] >= 0 && h[8] < 64, "%s: implausible header", path);
    Prog g;
    g.image_size = (int)h[0];
    g.n_biases = h[4];
    g.depth = (int)h[9];
    std::vector<int32_t> e((size_t)(h[7] + h[8]));
    CHECK(fread(e.data(), 4, e.size(), f) == e.size(), "%s: short index lists", path);
    g.towers.assign(e.begin(), e.begin() + h[7]);
    g.preds.assign(e.begin() + h[7], e.end());
    g.bufs.resize((size_t)h[1]);
    g.ops.resize((size_t)h[2]);
    CHECK(fread(g.bufs.data(), sizeof(vgh_buf_desc), g.bufs.size(), f) == g.bufs.size(), "%s: short buffer table", path);
    CHECK(fread(g.ops.data(), sizeof(vgh_op_desc), g.ops.size(), f) == g.ops.size(), "%s: short op table", path);
    fclose(f);
    g.weights.assign((size_t)h[3], 0.0f);
    return g;
}

static std::vector<int> towers_of(const NetPlan& p) {
    std::vector<int> m;
    for (size_t i = 0; i < p.ops.size(); ++i)
        if (p.ops[i].tower) m.push_back((int)i);
    return m;
}
static std::vector<int> preds_of(const NetPlan& p) {
    std::vector<int> m;
    for (size_t i = 0; i < p.ops.size(); ++i)
        if (p.ops[i].deferrable) m.push_back((int)i);
    return m;
}
static bool has(const std::vector<int>& v, int x) {
    for (int y : v)
        if (y == x) return true;
    return false;
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

// after a change that takes the mark from op `victim`: it is unmarked, every op of the OTHER trees keeps its mark, the plan still holds together (every marked
// op sits in a tree, trees are self-consistent), and the old marks are what `want_preds` says
static void check_after(const char* path, const char* what, const Prog& g, const NetPlan& p0, const NetPlan& pr, const TowerPlan& tr, int victim, const std::vector<int>& want_preds) {
    CHECK(!pr.ops[victim].tower, "%s: %s: op %d keeps its tower mark", path, what, victim);
    const int tree0 = p0.ops[victim].tower;
    for (int i : g.towers)
        if (p0.ops[i].tower != tree0) CHECK(pr.ops[i].tower, "%s: %s: op %d of another level lost its mark", path, what, i);
    CHECK(preds_of(pr) == want_preds, "%s: %s: the deferrable marks changed", path, what);
    for (size_t i = 0; i < g.ops.size(); ++i) {
        if (!pr.ops[i].tower) continue;
        CHECK(pr.ops[i].tower >= 1 && pr.ops[i].tower <= (int)tr.trees.size(), "%s: %s: op %zu names no tree", path, what, i);
        CHECK(has(tr.trees[pr.ops[i].tower - 1].ops, (int)i), "%s: %s: op %zu is not in its tree", path, what, i);
    }
}

static void check_program(const char* path) {
    const Prog g = load(path);
    NetPlan p;
    TowerPlan tp;
    CHECK(g.plan(&p, &tp) == VGH_OK, "%s: the plan refuses the program: %s", path, p.err);
    const std::vector<int> m = towers_of(p);
    CHECK(!g.towers.empty() && m == g.towers, "%s: %zu tower ops marked, %zu expected (first marked %d)", path, m.size(), g.towers.size(), m.empty() ? -1 : m[0]);
    CHECK(preds_of(p) == g.preds && g.preds.size() == 9, "%s: the deferrable marks are not the nine prediction convs", path);
    for (int i : m) {
        const vgh_op_desc& d = g.ops[i];
        CHECK(d.ksize == 3 && d.stride == 1 && d.act == VGH_ACT_RELU && d.res_buf < 0 && !d.shuffle && g.bufs[d.in_buf].is_f32 == VGH_FMT_BF16 && g.bufs[d.out_buf].is_f32 == VGH_FMT_BF16 &&
                  !p.ops[i].b2b && !p.ops[i].ev_done && !p.ops[i].deferrable,
              "%s: op %d is marked but is no plain 3x3 tower conv", path, i);
    }
    // one tree per prediction buffer: a root no tree op writes, `depth` layers ascending in program order, grouped convs among them
    CHECK(tp.trees.size() == 3, "%s: %zu trees", path, tp.trees.size());
    size_t in_trees = 0;
    int grouped = 0;
    for (const TowerTree& t : tp.trees) {
        CHECK(t.depth == g.depth && (int)t.bufs.size() == t.depth + 1 && t.ops.size() == t.layer.size() && t.ops.size() <= (size_t)kMaxTowerOps, "%s: tree of buffer %d: depth %d", path, t.pred_buf, t.depth);
        CHECK(g.bufs[t.pred_buf].is_f32 == VGH_FMT_F32 && t.root_buf == t.bufs[0] && t.root_c1 > t.root_c0 && t.root_c1 <= g.bufs[t.root_buf].pitch, "%s: tree root", path);
        for (size_t k = 0; k < t.ops.size(); ++k) {
            const vgh_op_desc& d = g.ops[t.ops[k]];
            CHECK(t.layer[k] >= 1 && t.layer[k] <= t.depth && (k == 0 || (t.ops[k] > t.ops[k - 1] && t.layer[k] >= t.layer[k - 1])), "%s: tree order", path);
            CHECK(d.in_buf == t.bufs[t.layer[k] - 1] && d.out_buf == t.bufs[t.layer[k]], "%s: op %d does not link tensors %d -> %d of its tree", path, t.ops[k], t.layer[k] - 1, t.layer[k]);
            CHECK(d.out_buf != t.root_buf, "%s: op %d writes its tree's root", path, t.ops[k]);
            grouped += d.grp_cout != 0;
        }
        for (int j : g.preds)
            if (g.ops[j].out_buf == t.pred_buf) CHECK(g.ops[j].in_buf == t.bufs[t.depth], "%s: prediction conv %d does not read the last tensor", path, j);
        for (size_t j = 0; j < g.ops.size(); ++j) {  // the root's writers are flagged (the moved prediction guard), nobody else is
            const bool w = (g.ops[j].kind == VGH_OP_CONV || g.ops[j].kind == VGH_OP_STEM) && g.ops[j].out_buf == t.root_buf;
            if (w) CHECK(p.ops[j].writes_tower_root && (int)j < t.ops[0], "%s: op %zu writes a root without the flag, or behind the tree", path, j);
        }
        in_trees += t.ops.size();
    }
    CHECK(in_trees == m.size() && grouped >= 3, "%s: %zu ops in trees, %zu marked, %d grouped", path, in_trees, m.size(), grouped);
    int flagged = 0;
    for (size_t j = 0; j < g.ops.size(); ++j) flagged += p.ops[j].writes_tower_root;
    CHECK(flagged == 3, "%s: %d ops flagged as root writers", path, flagged);

    int scratch = -1;  // a bf16 buffer that no marked op touches, for the extra ops
    for (size_t b = 0; b < g.bufs.size() && scratch < 0; ++b) {
        bool used = g.bufs[b].is_f32 != VGH_FMT_BF16 || g.bufs[b].pitch < 32;
        for (int i : m) used = used || g.ops[i].in_buf == (int)b || g.ops[i].out_buf == (int)b;
        for (int i : g.preds) used = used || g.ops[i].in_buf == (int)b;
        if (!used) scratch = (int)b;
    }
    CHECK(scratch >= 0, "%s: no scratch buffer", path);
    const TowerTree& t0 = tp.trees[0];
    const int first = t0.ops[0];  // reads the root; its output is read by the tree's second layer
    {  // a second reader of a tower tensor
        Prog r = g;
        r.ops.push_back(conv1x1(g.ops[first].out_buf, scratch));
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: second reader: %s", path, pr.err);
        check_after(path, "second reader", g, p, pr, tr, first, g.preds);
    }
    {  // ... as a residual
        Prog r = g;
        vgh_op_desc d = conv1x1(scratch, scratch);
        d.res_buf = g.ops[first].out_buf;
        r.ops.push_back(d);
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: residual reader: %s", path, pr.err);
        check_after(path, "residual reader", g, p, pr, tr, first, g.preds);
    }
    {  // the op itself gains a residual
        Prog r = g;
        r.ops[first].res_buf = scratch;
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: own residual: %s", path, pr.err);
        check_after(path, "own residual", g, p, pr, tr, first, g.preds);
    }
    {  // an op another lane waits for
        Prog r = g;
        vgh_op_desc d = conv1x1(scratch, scratch);
        d.lane = 1 | ((first + 1) << 8);
        r.ops.push_back(d);
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: awaited op: %s", path, pr.err);
        CHECK(pr.ops[first].ev_done == 1, "%s: awaited op: no event", path);
        check_after(path, "awaited op", g, p, pr, tr, first, g.preds);
    }
    {  // a later writer of the root: the ops that read the root cannot be computed afterwards
        Prog r = g;
        r.ops.push_back(conv1x1(scratch, t0.root_buf));
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: late root writer: %s", path, pr.err);
        check_after(path, "late root writer", g, p, pr, tr, first, g.preds);
    }
    {  // a later writer of a tower tensor takes the marks of its writers (and the old rule takes the mark of a prediction conv whose input is rewritten)
        Prog r = g;
        const int lastbuf = t0.bufs[t0.depth];
        r.ops.push_back(conv1x1(scratch, lastbuf));
        NetPlan pr;
        TowerPlan tr;
        CHECK(r.plan(&pr, &tr) == VGH_OK, "%s: late tower writer: %s", path, pr.err);
        for (size_t k = 0; k < t0.ops.size(); ++k)
            if (g.ops[t0.ops[k]].out_buf == lastbuf && g.ops[t0.ops[k]].out_coff < 32) CHECK(!pr.ops[t0.ops[k]].tower, "%s: late tower writer: op %d keeps its mark", path, t0.ops[k]);
        CHECK(preds_of(pr).size() < g.preds.size(), "%s: late tower writer: the old rule did not react", path);
    }
    {  // 8-bit and fp16 programs have no bf16 -> bf16 towers: a format change takes every mark of the tree
        Prog r = g;
        r.bufs[g.ops[first].out_buf].is_f32 = VGH_FMT_F16;
        NetPlan pr;
        TowerPlan tr;
        if (r.plan(&pr, &tr) == VGH_OK) CHECK(!pr.ops[first].tower, "%s: an fp16 tower tensor keeps a mark", path);
    }
}

static void check_traits() {
    // the five families the benchmark's table puts the tower ops on, and their chains
    CHECK(chain_code(TileFamily::Igemm) == 1, "igemm: tap-major, bias last");
    CHECK(chain_code(TileFamily::Patch) == 0, "p: channel-block-major, bias last");
    CHECK(chain_code(TileFamily::PatchPipe) == 2, "q: channel-block-major, bias first");
    CHECK(chain_code(TileFamily::PingPongG) == 2 && chain_code(TileFamily::PingPongH) == 2 && chain_code(TileFamily::PingPongS) == 2, "g / h / s: channel-block-major, bias first");
    CHECK(chain_code(TileFamily::W) == -1 && chain_code(TileFamily::R) == -1 && chain_code(TileFamily::Stream) == -1 && chain_code(TileFamily::SplitIgemm) == -1 &&
              chain_code(TileFamily::SplitPatch) == -1 && chain_code(TileFamily::PingPongF16) == -1 && chain_code(TileFamily::PatchS2) == -1,
          "families without a reproduced chain run densely");
    // the pending state carries the towers with the generation
    DeferState s;
    s.on = true;
    s.forward(4, s.skip(), true, 2);
    CHECK(s.pending && s.towers && s.lanes == 2 && s.B == 4, "a forward that skips the towers leaves them pending");
    CHECK(s.take() == 4 && !s.pending && !s.towers, "run_deferred takes both");
    s.forward(4, s.skip());
    CHECK(s.pending && !s.towers && s.lanes == 1, "a forward that runs its towers leaves only the prediction convs pending");
    s.forward(4, false, true, 2);
    CHECK(!s.pending && !s.towers && s.take() == 0, "towers are never pending alone");
}

int main(int argc, char** argv) {
    CHECK(argc >= 2, "usage: tower_plan_host FILE...");
    for (int i = 1; i < argc; ++i) check_program(argv[i]);
    check_traits();
    printf("tower plan host checks passed (%d checks)\n", checks);
    return 0;
}
