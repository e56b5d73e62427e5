// Tower-deferrable ops (vgh_net_set_defer, second mark): the 3x3 convs that stand in front of the deferrable prediction convs (net_plan.h, net_op_deferrable) and
// whose outputs nothing else reads.  A deferring forward skips them too; the select computes the survivors' prediction rows from the window of the towers' ROOT
// tensor around each survivor (postproc.hip, survivor_towers_kernel), which shrinks by one ring per 3x3 layer.  Decided from the descriptors alone.  Host logic on
// plain data: no HIP include (tests/tower_plan_host.hip checks it under the host sanitizers).
//
// An op gets the mark when it is a 3x3 / stride-1 / ReLU conv from a bf16 to a bf16 buffer that stores whole cout tiles into one segment, with no residual, no
// shuffle, not in a back-to-back pair, not awaited through an event, not overhanging its pitch (grouped convs are fine), and
//   * every op that reads its output window is deferrable or tower-deferrable itself, there is at least one, and nobody else writes that window;
//   * its input window is either written completely by tower-deferrable ops, or untouched by them and by every later op of the program (a root).
// The marked ops in front of ONE prediction buffer form a tree: one root window, layers in program order.  A set that is no such tree loses its marks.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/vgh.h"
#include "net_plan.h"

constexpr int kMaxTowerOps = 8;    // tower-deferrable ops in front of one prediction buffer
constexpr int kMaxTowerDepth = 3;  // 3x3 layers between the root and the prediction convs: a (2 depth + 1)^2 window of the root per survivor

struct TowerTree {
    int pred_buf = -1;                 // the fp32 prediction buffer the tree ends in
    int root_buf = -1;                 // the bf16 tensor the tree starts from ...
    int root_c0 = 0, root_c1 = 0;      // ... and the channel window [c0, c1) of it that the first layer reads
    int depth = 0;                     // 3x3 layers
    std::vector<int> ops;              // program order; layer numbers ascend
    std::vector<int> layer;            // 1 .. depth, per op
    std::vector<int> bufs;             // bufs[t]: the tensor that the ops of layer t write (t = 1 .. depth; bufs[0] = root_buf)
};

struct TowerPlan {
    std::vector<int> tower;         // per op: 1 + index into `trees`, 0 = not tower-deferrable
    std::vector<int> writes_root;   // per op: it writes (part of) the root window of a tree -- in overlap mode it may not run before the previous select has read the root
    std::vector<TowerTree> trees;
};

namespace tower_detail {
// channel window a conv reads / writes
inline void in_window(const vgh_op_desc& d, int* c0, int* c1) {
    *c0 = d.in_coff;
    *c1 = d.in_coff + d.cin + (d.grp_cout ? (d.cout_pad / d.grp_cout - 1) * d.grp_in_stride : 0);
}
inline void out_window(const vgh_op_desc& d, int* c0, int* c1) {  // (ops with a second output segment are never marked; for the others this is what they write)
    *c0 = d.out_coff;
    *c1 = d.out_coff + (d.out_split < d.cout_pad ? d.out_split : d.cout_pad);
}
inline bool overlap(int a0, int a1, int b0, int b1) { return a0 < b1 && b0 < a1; }
inline bool writes(const vgh_op_desc& e, int buf, int c0, int c1) {
    if (e.kind == VGH_OP_STEM) return e.out_buf == buf;
    if (e.kind == VGH_OP_SPP_POOL) return e.in_buf == buf;  // (the pool writes behind the channels it reads)
    if (e.kind != VGH_OP_CONV || e.out_buf != buf) return false;
    if (e.out_split < e.cout_pad || e.shuffle) return true;  // two segments / shuffled store: take the whole pitch as written
    int w0, w1;
    out_window(e, &w0, &w1);
    return overlap(w0, w1, c0, c1);
}
}  // namespace tower_detail

// fused_or_awaited[i]: op i is part of a back-to-back pair, a later op waits for its event, or its K window overhangs the pitch (NetPlan::Op); deferrable[i]: today's mark
inline void tower_plan(const vgh_buf_desc* bufs, const vgh_op_desc* ops, int n_ops, const std::vector<char>& fused_or_awaited, const std::vector<int>& deferrable, TowerPlan* tp) {
    using namespace tower_detail;
    *tp = TowerPlan();
    tp->tower.assign(n_ops, 0);
    tp->writes_root.assign(n_ops, 0);
    std::vector<char> mark(n_ops, 0);
    for (int i = 0; i < n_ops; ++i) {
        const vgh_op_desc& d = ops[i];
        if (d.kind != VGH_OP_CONV || d.ksize != 3 || d.stride != 1 || d.act != VGH_ACT_RELU || fused_or_awaited[i]) continue;
        if (bufs[d.in_buf].is_f32 != VGH_FMT_BF16 || bufs[d.out_buf].is_f32 != VGH_FMT_BF16 || d.in_buf == d.out_buf) continue;
        if (d.res_buf >= 0 || d.shuffle || d.cout_store != d.cout_pad || d.out_split < d.cout_pad || d.out_coff + d.cout_pad > bufs[d.out_buf].pitch) continue;
        if (d.in_coff % 8 || bufs[d.in_buf].pitch % 8 || d.out_coff % 8 || bufs[d.out_buf].pitch % 8) continue;
        if (d.grp_cout && (d.grp_cout % 32 || d.cout_pad % d.grp_cout || d.grp_in_stride % 8)) continue;
        mark[i] = 1;
    }
    // which prediction buffer an op's output ends in (-1 none yet, -2 more than one)
    std::vector<int> pred(n_ops, -1);
    for (bool changed = true; changed;) {
        changed = false;
        for (int i = n_ops - 1; i >= 0; --i) {
            if (!mark[i]) continue;
            const vgh_op_desc& d = ops[i];
            int o0, o1, i0, i1;
            out_window(d, &o0, &o1);
            in_window(d, &i0, &i1);
            bool ok = true;
            int readers = 0, my_pred = -1;
            for (int j = 0; j < n_ops && ok; ++j) {
                const vgh_op_desc& e = ops[j];
                if (j == i || e.kind == VGH_OP_FORK) continue;
                if (writes(e, d.out_buf, o0, o1)) ok = false;  // a second writer of the window
                if (e.kind == VGH_OP_CONV && e.res_buf == d.out_buf) ok = false;
                if (e.kind == VGH_OP_CONV && e.in_buf == d.out_buf) {
                    int r0, r1;
                    in_window(e, &r0, &r1);
                    if (!overlap(r0, r1, o0, o1)) continue;
                    if (j < i) ok = false;  // a reader in front of its writer: last forward's values, not a tree
                    const int pj = deferrable[j] ? e.out_buf : mark[j] ? pred[j] : -2;
                    if (!(deferrable[j] || mark[j]) || pj == -2) ok = false;
                    else if (pj >= 0) {
                        if (my_pred >= 0 && my_pred != pj) ok = false;
                        my_pred = pj;
                    }
                    ++readers;
                }
            }
            ok = ok && readers > 0;
            // the input window: all of it from marked ops, or none of it and no later writer
            if (ok) {
                std::vector<char> covered(std::max(i1 - i0, 0), 0);
                bool any_marked = false, any_other_later = false;
                for (int j = 0; j < n_ops; ++j) {
                    if (j == i || !writes(ops[j], d.in_buf, i0, i1)) continue;
                    if (mark[j]) {
                        any_marked = true;
                        if (j > i) ok = false;
                        int w0, w1;
                        out_window(ops[j], &w0, &w1);
                        for (int c = std::max(w0, i0); c < std::min(w1, i1); ++c) covered[c - i0] = 1;
                    } else if (j > i) {
                        any_other_later = true;
                    }
                }
                if (any_marked) {
                    for (char c : covered) ok = ok && c;
                } else {
                    ok = ok && !any_other_later;
                }
            }
            if (!ok) {
                mark[i] = 0;
                changed = true;
            } else if (pred[i] != my_pred) {
                pred[i] = my_pred;
                changed = true;
            }
        }
    }
    // trees, one per prediction buffer
    std::vector<int> preds;
    for (int i = 0; i < n_ops; ++i)
        if (mark[i] && pred[i] >= 0 && std::find(preds.begin(), preds.end(), pred[i]) == preds.end()) preds.push_back(pred[i]);
    for (int pb : preds) {
        TowerTree t;
        t.pred_buf = pb;
        bool ok = true;
        std::vector<int> layer_of_buf;  // parallel to t.bufs
        t.bufs.push_back(-1);
        for (int i = 0; i < n_ops && ok; ++i) {
            if (!mark[i] || pred[i] != pb) continue;
            const vgh_op_desc& d = ops[i];
            int i0, i1;
            tower_detail::in_window(d, &i0, &i1);
            int lay = 0;
            for (size_t b = 1; b < t.bufs.size(); ++b)
                if (t.bufs[b] == d.in_buf) lay = (int)b;
            if (lay == 0) {  // reads the root
                bool from_marked = false;
                for (int j = 0; j < n_ops; ++j) from_marked = from_marked || (mark[j] && j != i && writes(ops[j], d.in_buf, i0, i1));
                if (from_marked) ok = false;  // its producers belong to another tree
                if (t.root_buf < 0) {
                    t.root_buf = d.in_buf;
                    t.root_c0 = i0;
                    t.root_c1 = i1;
                } else if (t.root_buf != d.in_buf || t.root_c0 != i0 || t.root_c1 != i1) {
                    ok = false;  // one root window per tree
                }
            }
            const int mine = lay + 1;
            if (mine > kMaxTowerDepth) ok = false;
            if (ok) {
                if ((int)t.bufs.size() <= mine) t.bufs.resize(mine + 1, -1);
                if (t.bufs[mine] < 0) t.bufs[mine] = d.out_buf;
                if (t.bufs[mine] != d.out_buf) ok = false;  // one tensor per layer
                for (int b = 0; b < mine && ok; ++b) ok = t.bufs[b] != d.out_buf;
                if (!t.layer.empty() && t.layer.back() > mine) ok = false;  // layers ascend in program order
                t.ops.push_back(i);
                t.layer.push_back(mine);
                t.depth = std::max(t.depth, mine);
            }
        }
        ok = ok && t.root_buf >= 0 && (int)t.ops.size() <= kMaxTowerOps && t.root_buf != pb;
        // every deferrable conv of the prediction buffer reads the last layer's tensor: the rows come from ONE pixel of it
        for (int j = 0; j < n_ops && ok; ++j)
            if (deferrable[j] && ops[j].out_buf == pb) ok = ops[j].in_buf == t.bufs[t.depth];
        if (ok) {
            t.bufs[0] = t.root_buf;
            for (int i : t.ops) tp->tower[i] = (int)tp->trees.size() + 1;
            tp->trees.push_back(t);
        }
    }
    for (const TowerTree& t : tp->trees)
        for (int j = 0; j < n_ops; ++j)
            if (tower_detail::writes(ops[j], t.root_buf, t.root_c0, t.root_c1)) tp->writes_root[j] = 1;
}

// the second mark of a planned program: fills NetPlan::Op::tower / writes_tower_root and returns the trees (vgh_net_create calls it right behind net_plan)
inline void net_plan_towers(const vgh_buf_desc* bufs, const vgh_op_desc* ops, int n_ops, NetPlan* p, TowerPlan* tp) {
    std::vector<char> fused(n_ops, 0);
    std::vector<int> deferrable(n_ops, 0);
    for (int i = 0; i < n_ops; ++i) {
        fused[i] = p->ops[i].b2b || p->ops[i].ev_done || p->ops[i].overhang_ok;
        deferrable[i] = p->ops[i].deferrable;
    }
    tower_plan(bufs, ops, n_ops, fused, deferrable, tp);
    for (int i = 0; i < n_ops; ++i) {
        p->ops[i].tower = tp->tower[i];
        p->ops[i].writes_tower_root = tp->writes_root[i];
    }
}
