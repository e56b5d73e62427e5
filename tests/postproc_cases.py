"""Planted inputs for the C entry points of csrc/postproc.hip (no GPU, no library): vgh_topk, vgh_nms + vgh_compact, vgh_topk_nms / utils.nms_batched / utils.nms,
vgh_head_decode + vgh_gather_candidates.  Every case has a builder, what oracle/postproc_oracle.py says for it, and a claim that asserts ON THAT RESULT that the
property the case is named for is present.  tests/test_postproc_cases_host.py runs every claim on the oracle's own result; tests/test_gpu_postproc_cases.py feeds the
cases to the device and compares with the same results.  Everything is seeded; every float input is finite unless the case is named for the opposite.

Ordering contract (include/vgh.h): a stable descending sort in which -0.0 == +0.0 and every NaN ranks above +inf, ties by ascending index (po.stable_topk);
the NMS visits exactly the rows that pass score >= conf (po._nms_one filters first, then takes the top-k)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import postproc_oracle as po

# a quiet-NaN bit pattern that no case contains: the guard bands and "nothing written" prefills of the GPU tests
SENTINEL_BITS = 0x7FC0DEAD
SENTINEL_I32 = 0x5A5A5A5A
NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC12345)  # both signs, two payloads


def f32_bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# vgh_topk
# ----------------------------------------------------------------------------------------------------------------------
# 9216 = 9 register slots x 1024 lanes is the last row the cached kernel holds, 9217 the first uncached one; 10243 makes rows start off 16-byte multiples;
# k = 1024 fills the sort network with no padding entry
TOPK_PAIRS = [(1, 1), (64, 64), (1025, 1024), (1500, 1000), (9216, 1), (9216, 1024), (9217, 7), (9217, 1024), (10243, 1000)]
TOPK_ROWS = ["distinct", "all_equal", "boundary_tie", "low_bits", "early_stop", "slot_edges", "signs", "nan"]
N_NAN = 12  # below k for the pairs with k >= 64, above it for k = 1 and 7


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([20240607, *key])


def slot_edge_indices(A: int) -> List[int]:
    """first / last lane of register slots 0, 1 and 8, the first index behind the cache, the last of the row -- those that exist, in this order"""
    out: List[int] = []
    for i in (0, 1023, 1024, 9215, 9216, A - 1):
        if 0 <= i < A and i not in out:
            out.append(i)
    return out


def _signs_layout(A: int, k: int) -> Tuple[int, int, int]:
    """(positives, zeros, negatives): where A > k the cut at k falls inside the run of zeros"""
    P = k // 2
    rem = A - P
    Z = min(rem, (k - P) + max(1, (A - k + 1) // 2)) if A > k else max(1, rem // 2)
    return P, Z, rem - Z


def topk_row(name: str, A: int, k: int) -> np.ndarray:
    rng = _rng(TOPK_ROWS.index(name), A, k)
    perm = rng.permutation(A)
    if name == "distinct":
        c = A // 3
        v = ((np.arange(A) - c) * (4.0 / A)).astype(np.float32)  # [-1.33, 2.67), spacing 4 / A >> one ulp
        if A >= 8:
            v[c], v[c - 1] = np.float32(1e-40), np.float32(-1e-40)  # subnormals of both signs (the exact 0 is gone)
        return v[perm]
    if name == "all_equal":
        return np.full(A, 0.625, dtype=np.float32)
    if name == "boundary_tie":
        by_rank = (2.0 - np.arange(A) * 2.0**-12).astype(np.float32)  # exact, distinct
        lo, hi = max(0, k - 3), min(A - 1, k + 5)
        by_rank[lo : hi + 1] = by_rank[lo]
        v = np.empty(A, dtype=np.float32)
        v[perm] = by_rank
        return v
    if name == "low_bits":
        return (np.float32(0.75).view(np.uint32) + perm.astype(np.uint32)).view(np.float32)  # np.nextafter steps upward from 0.75, in a seeded order
    if name == "early_stop":
        by_rank = np.concatenate([rng.uniform(0.5, 1.0, k), rng.uniform(0.0, 0.25, A - k)]).astype(np.float32)
        by_rank[:k] = np.clip(by_rank[:k], 0.5, np.nextafter(np.float32(1), np.float32(0)))
        by_rank[k:] = np.clip(by_rank[k:], 0.0, np.nextafter(np.float32(0.25), np.float32(0)))
        v = np.empty(A, dtype=np.float32)
        v[perm] = by_rank
        return v
    if name == "slot_edges":
        v = (0.5 - np.arange(A) * 2.0**-15).astype(np.float32)  # descending ramp, exact
        for j, i in enumerate(slot_edge_indices(A)):
            v[i] = np.float32(2.0 - 0.125 * j)
        return v
    if name == "signs":
        P, Z, N = _signs_layout(A, k)
        pos = (1.0 + np.arange(P) * 2.0**-11).astype(np.float32)
        if P:
            pos[0] = np.inf
        neg = (-1.0 - np.arange(N) * 2.0**-11).astype(np.float32)
        if N:
            neg[-1] = -np.inf
        zero_bits = np.where(rng.integers(0, 2, Z) == 1, 0x80000000, 0).astype(np.uint32)
        if Z >= 4:  # in index order: -0 before +0 and +0 before -0, whatever the draw
            zero_bits[:4] = (0x80000000, 0, 0, 0x80000000)
        v = np.empty(A, dtype=np.float32)
        others = rng.permutation(np.concatenate([pos, neg]))
        zpos = np.sort(rng.choice(A, Z, replace=False))
        mask = np.zeros(A, dtype=bool)
        mask[zpos] = True
        v.view(np.uint32)[zpos] = zero_bits
        v[~mask] = others
        return v
    if name == "nan":
        v = rng.uniform(-2.0, 2.0, A).astype(np.float32)
        at = np.sort(rng.choice(A, min(N_NAN, A), replace=False))
        v.view(np.uint32)[at] = [NAN_PATTERNS[(j * 3 + 1) % 4] for j in range(len(at))]
        return v
    raise KeyError(name)


def topk_scores(A: int, k: int) -> np.ndarray:
    """[len(TOPK_ROWS), A] float32: one row per image"""
    return np.stack([topk_row(n, A, k) for n in TOPK_ROWS])


def topk_reference(scores: np.ndarray, k: int) -> np.ndarray:
    """[B, k] int64: po.stable_topk of every row"""
    return np.stack([po.stable_topk(torch.from_numpy(r.copy()), k).numpy() for r in scores])


def radix_passes(row: np.ndarray, k: int) -> int:
    """How many of its 8 passes the radix select of csrc/postproc.hip runs on this row (it stops at the first pass whose selected bin holds exactly the remaining
    count).  A restatement of the select on the contract's keys, used by the claims only: the answer itself always comes from po.stable_topk."""
    u = f32_bits(row).astype(np.uint64)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FFFFFFF, np.where(u == 0x80000000, 0, u))  # NaN above +inf; -0 == +0
    key = np.where(u >> 31, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)
    comp = (key << np.uint64(32)) | (~np.arange(len(row), dtype=np.uint64) & np.uint64(0xFFFFFFFF))
    kk = k
    for p in range(8):
        bins = ((comp >> np.uint64(56 - 8 * p)) & np.uint64(255)).astype(np.int64)
        hist = np.bincount(bins, minlength=256)
        above = 0
        for t in range(255, -1, -1):
            if above < kk <= above + hist[t]:
                break
            above += hist[t]
        comp = comp[bins == t]
        if kk == above + hist[t]:
            return p + 1
        kk -= above
    return 8


def topk_claim(name: str, row: np.ndarray, k: int, idx: np.ndarray) -> None:
    """asserts on po.stable_topk's answer `idx` [k] that the row holds what it is named for"""
    A = len(row)
    idx = np.asarray(idx, dtype=np.int64)
    bits = f32_bits(row)
    sel = row[idx]
    assert len(np.unique(idx)) == k
    if name not in ("nan",):
        assert np.isfinite(row).all() or name == "signs"
    if name == "distinct":
        assert len(np.unique(bits)) == A and (np.diff(sel) < 0).all()
        if A >= 8:
            sub = np.abs(row) < np.finfo(np.float32).tiny
            assert (row < 0).any() and (row > 1).any() and (sub & (row > 0)).any() and (sub & (row < 0)).any()
    elif name == "all_equal":
        assert idx.tolist() == list(range(k)) and len(np.unique(bits)) == 1
        assert A == k or radix_passes(row, k) >= 7  # the index bits decide: the select runs into the low index bytes (all 8 passes unless the cut is a bin edge)
    elif name == "boundary_tie":
        tied = np.flatnonzero(row == sel[-1])
        lo = max(0, k - 3)
        if A >= 2:
            assert len(tied) == min(A - 1, k + 5) - lo + 1 >= 2
        if A > k:
            assert len(tied) > k - lo >= 1  # copies on both sides of the cut
        assert idx[lo:].tolist() == tied[: k - lo].tolist()  # the lowest indices win, in ascending order
        assert (np.diff(sel[: lo + 1]) < 0).all()
    elif name == "low_bits":
        assert len(np.unique(bits)) == A and len(np.unique(bits >> 14)) == 1 and (np.diff(sel) < 0).all()  # the top 18 key bits separate nothing
        assert radix_passes(row, k) >= (3 if A > k else 1)
    elif name == "early_stop":
        assert ((row >= 0.5) & (row < 1.0)).sum() == k and ((row >= 0.0) & (row < 0.25)).sum() == A - k
        # the early exit is taken: a whole bin is selected before the index bits are reached.  (With these contents it is the FIRST pass: the keys of [0.5, 1) and of
        # [0, 0.25) already differ in their top byte, sign-flip bit + 7 exponent bits.)
        assert radix_passes(row, k) == 1
        assert set(idx.tolist()) == set(np.flatnonzero(row >= 0.5).tolist())
    elif name == "slot_edges":
        e = slot_edge_indices(A)
        m = min(k, len(e))
        assert idx[:m].tolist() == e[:m]
        assert idx[m:].tolist() == [i for i in range(A) if i not in e][: k - m]
    elif name == "signs":
        P, Z, N = _signs_layout(A, k)
        zeros = np.flatnonzero(row == 0)
        assert len(zeros) == Z and (row > 0).sum() == P and (row < 0).sum() == N
        assert (P == 0 or np.isposinf(row).sum() == 1) and (N == 0 or np.isneginf(row).sum() == 1)
        n_sel = min(Z, k - P)
        assert idx[P : P + n_sel].tolist() == zeros[:n_sel].tolist()  # the two zeros tie: ascending index whatever the sign
        if A > k:
            assert 1 <= n_sel < Z and P + n_sel == k  # the cut falls inside the run of zeros
        if Z >= 4 and n_sel >= 4:
            zb = bits[zeros[:n_sel]] >> 31
            assert ((zb[:-1] == 1) & (zb[1:] == 0)).any() and ((zb[:-1] == 0) & (zb[1:] == 1)).any()  # -0 ranked before +0 and the other way round
    elif name == "nan":
        nan_at = np.flatnonzero(np.isnan(row))
        assert len(nan_at) == min(N_NAN, A)
        pats = set(bits[nan_at].tolist())
        assert pats <= set(NAN_PATTERNS) and (len(nan_at) < 4 or pats == set(NAN_PATTERNS))
        m = min(k, len(nan_at))
        assert idx[:m].tolist() == nan_at[:m].tolist()  # every NaN first, in index order, whatever its sign or payload
        assert np.isfinite(sel[m:]).all() and (np.diff(sel[m:]) <= 0).all()
    else:
        raise KeyError(name)


# ----------------------------------------------------------------------------------------------------------------------
# vgh_nms + vgh_compact
# ----------------------------------------------------------------------------------------------------------------------
NMS_SIZES = [(0, 4), (1, 1), (63, 63), (64, 100), (65, 1), (1000, 100), (1023, 2048), (1024, 1024)]
NMS_SHAPES = ["disjoint", "identical", "alternating_chain"]


def keep_positions(boxes: np.ndarray, scores: np.ndarray, conf: float, iou: float, keep_k: int) -> Tuple[np.ndarray, int]:
    """po.nms_torchvision output -> what vgh_nms writes: ([keep_k] int32 positions into the n_in rows, -1 behind the count; count).  The filter is a mask: the rows
    that fail score >= conf are taken out before torchvision's loop sees anything, wherever they stand."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        rows = np.flatnonzero(scores >= np.float32(conf))
    kept = rows[po.nms_torchvision(boxes[rows], scores[rows], iou)][:keep_k]
    out = np.full(keep_k, -1, dtype=np.int32)
    out[: len(kept)] = kept
    return out, len(kept)


def _disjoint(n: int) -> np.ndarray:
    i = np.arange(n)
    x, y = 20.0 * (i % 40), 20.0 * (i // 40)
    return np.stack([x, y, x + 10.0, y + 12.0], 1).astype(np.float32)


def _descending(n: int, hi: float = 0.99, lo: float = 0.6) -> np.ndarray:
    return np.linspace(hi, lo, n).astype(np.float32) if n > 1 else np.full(n, hi, dtype=np.float32)


def _chain(n: int) -> np.ndarray:
    """10 wide, 3 apart: IoU(i, i+1) = 7 / 13 > 0.5, IoU(i, i+2) = 4 / 16"""
    x = 3.0 * np.arange(n)
    return np.stack([x, np.zeros(n), x + 10.0, np.full(n, 10.0)], 1).astype(np.float32)


def nms_cases() -> Dict[str, dict]:
    """name -> dict(boxes [B,n,4], scores [B,n], conf, iou, keep_k, claim): ``claim(keep [B,keep_k], counts [B])`` asserts on keep_positions' answer"""
    cases: Dict[str, dict] = {}

    def add(name, boxes, scores, conf, iou, keep_k, claim):
        boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
        assert boxes.shape[:2] == scores.shape and boxes.shape[2] == 4
        cases[name] = dict(boxes=boxes, scores=scores, conf=conf, iou=iou, keep_k=keep_k, claim=claim)

    for n, kk in NMS_SIZES:
        boxes = np.stack([_disjoint(n), np.tile(np.float32([5, 5, 25, 30]), (n, 1)).reshape(n, 4), _chain(n)])
        scores = np.tile(_descending(n), (3, 1))

        def sizes(keep, counts, n=n, kk=kk):
            assert counts.tolist() == [min(n, kk), min(n, 1), min((n + 1) // 2, kk)]
            assert keep[0, : counts[0]].tolist() == list(range(counts[0]))  # disjoint: only the keep_k cut bites
            assert keep[1, : counts[1]].tolist() == [0][: counts[1]]  # identical: one round suppresses rows in every ballot word
            assert keep[2, : counts[2]].tolist() == list(range(0, 2 * counts[2], 2))  # the chain: exactly the even ranks, one round each
            for b in range(3):
                assert (keep[b, counts[b] :] == -1).all()

        add(f"sizes_{n}_{kk}", boxes, scores, 0.5, 0.5, kk, sizes)

    # A (62) suppresses B (63), B would have suppressed C (64); A and C overlap by 4 / 16 only.  The three straddle the first word boundary.
    n = 70
    boxes = _disjoint(n)
    boxes[:, 1] += 100.0
    boxes[:, 3] += 100.0
    boxes[62:65] = _chain(3)

    def dead(keep, counts, n=n, boxes=boxes):
        assert counts.tolist() == [n - 1] and 63 not in keep[0] and 62 in keep[0] and 64 in keep[0]
        assert keep_positions(boxes[63:65], [0.9, 0.8], 0.5, 0.5, 2)[1] == 1  # alive, B does suppress C

    add("dead_suppressor", boxes[None], _descending(n)[None], 0.5, 0.5, 100, dead)

    # thresholds: one fixed set
    T = np.float32(
        [
            [0, 0, 10, 10],      # 0
            [0, 0, 10, 10],      # 1  exact duplicate of 0: IoU exactly 1
            [0, 0, 10, 8],       # 2  IoU 0.8 with 0
            [0, 0, 10, 5],       # 3  IoU exactly 0.5 with 0
            [50, 50, 50, 50],    # 4  zero area
            [50, 50, 50, 50],    # 5  zero area, same place: 0 / 0
            [100, 0, 110, 10],   # 6
            [110, 0, 120, 10],   # 7  touches 6: intersection 0
            [230, 210, 200, 200],  # 8  inverted: x2 < x1, y2 < y1 (area +300 from two negative sides)
            [200, 200, 230, 210],  # 9  the same corners the right way round
            [300, 300, 310, 310],  # 10 alone
            [0, 1, 10, 11],      # 11 IoU 9 / 11 with 0
        ]
    )
    ts = np.float32([0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55, 0.5, 0.45, 0.4])

    def thr_claim(expect_keep):
        def claim(keep, counts):
            assert keep[0, : counts[0]].tolist() == expect_keep and (keep[0, counts[0] :] == -1).all()

        return claim

    all12 = list(range(12))
    for tag, iou, conf, expect in [
        ("iou_0", 0.0, -np.inf, [0, 4, 5, 6, 7, 8, 9, 10]),          # any positive overlap suppresses; touching (IoU 0) and 0 / 0 do not
        ("iou_1", 1.0, -np.inf, all12),                                # IoU exactly 1 is not > 1
        ("iou_negative", -0.5, -np.inf, [0]),                          # IoU 0 > -0.5: row 0 suppresses every other row, the zero-area ones included (0 / 100)
        ("iou_nan", np.nan, -np.inf, all12),
        ("conf_equal_score", 0.5, float(ts[5]), [0, 3, 4, 5]),         # >=: row 5 passes, row 6 does not
        ("conf_minus_inf", 0.5, -np.inf, [0, 3, 4, 5, 6, 7, 8, 9, 10]),
        ("conf_plus_inf", 0.5, np.inf, []),
        ("conf_nan", 0.5, np.nan, []),
    ]:
        add(f"thresholds_{tag}", T[None], ts[None], conf, iou, 16, thr_claim(expect))

    # nan_head: 5 NaN rows where vgh_topk puts them, each on top of a valid row; the scores behind descend through conf
    n = 70
    boxes = _disjoint(n)
    boxes[0:5] = boxes[5:10]
    scores = np.empty(n, dtype=np.float32)
    scores[5:] = np.linspace(0.95, 0.2, n - 5)
    scores.view(np.uint32)[0:5] = [NAN_PATTERNS[j % 4] for j in range(5)]
    n_pass = int((scores[5:] >= 0.5).sum())

    def nan_head(keep, counts, n=n, n_pass=n_pass):
        assert 5 < n_pass < n - 5 and counts.tolist() == [n_pass]
        assert keep[0, :n_pass].tolist() == list(range(5, 5 + n_pass))  # no NaN row kept, no valid row suppressed by one, the last valid rows not dropped

    add("nan_head", boxes[None], scores[None], 0.5, 0.5, 100, nan_head)
    return cases


def nms_reference(case: dict) -> Tuple[np.ndarray, np.ndarray]:
    """(keep [B,keep_k] int32, counts [B] int32)"""
    outs = [keep_positions(b, s, case["conf"], case["iou"], case["keep_k"]) for b, s in zip(case["boxes"], case["scores"])]
    B, kk = len(outs), case["keep_k"]
    return np.stack([o[0] for o in outs]).reshape(B, kk), np.asarray([o[1] for o in outs], dtype=np.int32)


def compact_reference(boxes, scores, flame, keep):
    """vgh_compact: rows picked by keep, zeros behind the count.  flame may be None."""
    B, kk = keep.shape
    ob, os_ = np.zeros((B, kk, 4), np.float32), np.zeros((B, kk), np.float32)
    of = None if flame is None else np.zeros((B, kk, flame.shape[2]), np.float32)
    for b in range(B):
        m = keep[b] >= 0
        ob[b, m], os_[b, m] = boxes[b, keep[b, m]], scores[b, keep[b, m]]
        if of is not None:
            of[b, m] = flame[b, keep[b, m]]
    return ob, os_, of


# ----------------------------------------------------------------------------------------------------------------------
# vgh_topk_nms / utils.nms_batched / utils.nms
# ----------------------------------------------------------------------------------------------------------------------
def _crowd(rng, n: int, clusters: int) -> np.ndarray:
    c = rng.uniform(50, 600, (clusters, 2))
    which = rng.integers(0, clusters, n)
    ctr = c[which] + rng.uniform(-6, 6, (n, 2))
    wh = rng.uniform(30, 40, (n, 2))
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)


def topk_nms_cases() -> Dict[str, dict]:
    """name -> dict(boxes [B,n,4], scores [B,n], conf, iou, pre_k, keep_k, claim): ``claim(ref)`` on topk_nms_reference's answer"""
    cases: Dict[str, dict] = {}
    rng = _rng(77)
    B, n = 2, 300
    boxes = np.stack([_crowd(rng, n, 25) for _ in range(B)])
    scores = rng.choice(np.linspace(0.3, 0.95, 14).astype(np.float32), (B, n))

    def ties(ref, scores=scores):
        for b, (rb, rs, rows) in enumerate(ref):
            assert 10 < len(rs) <= 100 and len(np.unique(rs)) < len(rs)  # survivors share scores: the index decides among them
            assert (np.diff(rs) <= 0).all() and (np.diff(rows) < 0).any()  # gathered from rows that are NOT in input order
            assert (scores[b] < 0.5).any() and len(rs) < (scores[b] >= 0.5).sum()  # the filter and the suppression both bite

    cases["unsorted_ties"] = dict(boxes=boxes, scores=scores, conf=0.5, iou=0.5, pre_k=1000, keep_k=100, claim=ties)

    n = 1500
    boxes = np.stack([_disjoint(n)[rng.permutation(n)] for _ in range(B)])
    scores = np.empty((B, n), dtype=np.float32)
    for b in range(B):
        by_rank = np.concatenate([np.linspace(0.999, 0.5, 1200), np.linspace(0.499, 0.01, n - 1200)]).astype(np.float32)
        scores[b, rng.permutation(n)] = by_rank

    def more(ref, sc=scores, keep_k=100):
        for b, (rb, rs, rows) in enumerate(ref):
            assert (sc[b] >= 0.5).sum() == 1200 and len(rs) == keep_k
            order = np.argsort(-np.where(np.isnan(sc[b]), -np.inf, sc[b]), kind="stable")
            assert rows.tolist() == order[:keep_k].tolist()  # disjoint boxes: the keep_k best FINITE scores, nothing else

    cases["more_than_pre_k"] = dict(boxes=boxes, scores=scores, conf=0.5, iou=0.5, pre_k=1000, keep_k=100, claim=more)

    sc_nan = scores.copy()
    for b in range(B):  # ten of the rows that fail the filter anyway become NaN: the set of rows that pass is unchanged
        at = rng.choice(np.flatnonzero(scores[b] < 0.5), 10, replace=False)
        sc_nan[b].view(np.uint32)[at] = [NAN_PATTERNS[j % 4] for j in range(10)]

    def displaced(ref, keep_k):
        more(ref, sc_nan, keep_k)
        for b, (rb, rs, rows) in enumerate(ref):
            assert np.isnan(sc_nan[b]).sum() == 10 and np.isfinite(rs).all()

    cases["nan_displaces"] = dict(boxes=boxes, scores=sc_nan, conf=0.5, iou=0.5, pre_k=1000, keep_k=100, claim=lambda ref: displaced(ref, 100))
    # the same with every candidate slot visible in the result: ten NaN rows among the 1000 candidates would push the valid ranks 990 .. 999 out
    cases["nan_displaces_keep_all"] = dict(boxes=boxes, scores=sc_nan, conf=0.5, iou=0.5, pre_k=1000, keep_k=1000, claim=lambda ref: displaced(ref, 1000))

    # widths: a small crowd for the flame_width / keep_k > k / NULL variants
    n = 50
    boxes = np.stack([_crowd(rng, n, 12) for _ in range(B)])
    scores = rng.uniform(0.3, 0.99, (B, n)).astype(np.float32)

    def small(ref):
        for rb, rs, rows in ref:
            assert 3 < len(rs) < 40

    cases["widths"] = dict(boxes=boxes, scores=scores, conf=0.5, iou=0.5, pre_k=1000, keep_k=64, claim=small)
    return cases


WIDTHS = [1, 7, 413, 500, None]  # flame_width of the "widths" case; None: flame NULL on both sides


def flame_rows(B: int, n: int, width: int, seed: int = 5) -> np.ndarray:
    return _rng(seed, B, n, width).standard_normal((B, n, width)).astype(np.float32)


def topk_nms_reference(case: dict):
    """per image (boxes [m,4], scores [m], ORIGINAL row of each survivor [m]) from po._nms_one: filter, then top-k, then the NMS.  The row numbers ride through
    _nms_one in the place of the flame tensor (exact in float64)."""
    out = []
    for b, s in zip(case["boxes"], case["scores"]):
        rows = torch.arange(len(s), dtype=torch.float64)[:, None]
        rb, rs, rr = po._nms_one(torch.from_numpy(b.copy()), torch.from_numpy(s.copy())[:, None], rows, case["conf"], case["iou"], case["pre_k"], case["keep_k"])
        out.append((rb.numpy(), rs.numpy(), rr[:, 0].numpy().astype(np.int64)))
    return out


def topk_nms_slabs(case: dict, ref, flame):
    """the slabs vgh_topk_nms writes: boxes [B,keep_k,4], scores [B,keep_k], flame [B,keep_k,W] or None, counts [B]; zeros behind the count"""
    B, kk = len(ref), case["keep_k"]
    ob, os_ = np.zeros((B, kk, 4), np.float32), np.zeros((B, kk), np.float32)
    of = None if flame is None else np.zeros((B, kk, flame.shape[2]), np.float32)
    counts = np.zeros(B, np.int32)
    for b, (rb, rs, rows) in enumerate(ref):
        m = len(rs)
        counts[b] = m
        ob[b, :m], os_[b, :m] = case["boxes"][b, rows], case["scores"][b, rows]
        assert np.array_equal(ob[b, :m], rb) and np.array_equal(os_[b, :m], rs)
        if of is not None:
            of[b, :m] = flame[b, rows]
    return ob, os_, of, counts


# ----------------------------------------------------------------------------------------------------------------------
# vgh_head_decode + vgh_gather_candidates
# ----------------------------------------------------------------------------------------------------------------------
PRED_CLS, PRED_FLAME = 68, 72  # VGH_PRED_CLS_OFF, VGH_PRED_FLAME_OFF
PAD_FILL = 7.7e30  # finite; in the unused and pad channels of every prediction row: it must not leak into any output
LIVE_PAIRS = [(128, 64), (300, 100), (0, 0), (1, 1)]
# name -> (levels (h, w), strides, B, extra pitch per level)
GEOMETRIES = {
    "one_anchor": ([(1, 1)], [32], 1, [0]),
    "non_square": ([(3, 7), (2, 3)], [8, 16], 3, [0, 0]),
    "four_levels": ([(9, 5), (5, 3), (3, 2), (1, 1)], [4, 8, 16, 32], 2, [0, 0, 0, 0]),
    "pitches": ([(20, 20), (10, 10), (5, 5)], [8, 16, 32], 2, [3, 8, 17]),
}
# per side: (kind, expected distance in cells)
_DFL_SIDES = [("bin0", 0.0), ("bin16", 16.0), ("bin8", 8.0), ("uniform", 8.0), ("large_equal", 8.0)]
_CLS = [(100.0, 1.0), (-100.0, 0.0), (0.0, 0.5)]


def _dfl_side(kind: str) -> np.ndarray:
    if kind.startswith("bin"):
        v = np.full(17, -100.0, dtype=np.float32)
        v[int(kind[3:])] = 100.0
        return v
    return np.full(17, 0.0 if kind == "uniform" else 1e4, dtype=np.float32)


def decode_case(geometry: str, S: int, E: int) -> dict:
    """Prediction tensors [B,h,w,pitch] per level (randn * 1.5 in the live channels, PAD_FILL elsewhere) with plants at the first and the last anchor of every level,
    and the float64 oracle: boxes [B,A,4], scores [B,A], flame [B,A,413].  ``plants``: list of dict(b, a, level, ay, ax, sides, cls, sign, scale)."""
    sizes, strides, B, extra = GEOMETRIES[geometry]
    live = PRED_FLAME + S + E + 13
    g = torch.Generator().manual_seed(1000 * S + E + len(sizes))
    preds, plants, start, q = [], [], 0, 0
    for lvl, ((h, w), ex) in enumerate(zip(sizes, extra)):
        pitch = live + ex
        t = torch.full((B, h, w, pitch), PAD_FILL, dtype=torch.float32)
        t[..., :69] = torch.randn(B, h, w, 69, generator=g) * 1.5
        t[..., PRED_FLAME:live] = torch.randn(B, h, w, live - PRED_FLAME, generator=g) * 1.5
        for b in range(B):
            for ay, ax in dict.fromkeys([(0, 0), (h - 1, w - 1)]):
                sides = [_DFL_SIDES[(q + s) % 5] for s in range(4)]
                cls = _CLS[q % 3]
                sign, scale = (1.0 if q % 2 == 0 else -1.0), (-8.0 if q % 2 == 0 else 6.0)
                row = t[b, ay, ax]
                for s, (kind, _) in enumerate(sides):
                    row[s * 17 : s * 17 + 17] = torch.from_numpy(_dfl_side(kind))
                row[PRED_CLS] = cls[0]
                row[PRED_FLAME : PRED_FLAME + min(S, 3)] = 20.0 * sign  # tanh saturates: exactly +-3
                row[PRED_FLAME + S : PRED_FLAME + S + min(E, 3)] = -20.0 * sign
                o_tr = PRED_FLAME + S + E + 9
                row[o_tr : o_tr + 3] = torch.tensor([-5000.25, -12345.5, -3.0e4])
                row[o_tr + 3] = scale
                plants.append(dict(b=b, a=start + ay * w + ax, level=lvl, ay=ay, ax=ax, sides=sides, cls=cls, sign=sign, scale=scale))
                q += 1
        preds.append(t)
        start += h * w
    olevels = []
    for t in preds:
        nchw = t.double().permute(0, 3, 1, 2)
        o = PRED_FLAME
        fl = po.assemble_flame_channels(nchw[:, o : o + S], nchw[:, o + S : o + S + E], nchw[:, o + S + E : o + S + E + 6], nchw[:, o + S + E + 6 : o + S + E + 9],
                                        nchw[:, o + S + E + 9 : o + S + E + 12], nchw[:, o + S + E + 12 : o + S + E + 13])
        olevels.append((nchw[:, :68], nchw[:, 68:69], fl))
    rb, rs, rf = po.ndfl_decode(olevels, strides)
    return dict(geometry=geometry, sizes=sizes, strides=strides, B=B, S=S, E=E, A=start, preds=preds, pitches=[live + ex for ex in extra], plants=plants,
                boxes=rb, scores=rs[..., 0], flame=rf)


def decode_claim(case: dict) -> None:
    """asserts on the float64 oracle that every plant shows what it was planted for, at the anchor it was planted at"""
    S, E, strides = case["S"], case["E"], case["strides"]
    assert torch.isfinite(case["boxes"]).all() and torch.isfinite(case["flame"]).all() and float(case["flame"].abs().max()) < 1e9  # PAD_FILL reached nothing
    assert case["A"] == sum(h * w for h, w in case["sizes"])
    seen = set()
    for p in case["plants"]:
        st = strides[p["level"]]
        cx, cy = (p["ax"] + 0.5) * st, (p["ay"] + 0.5) * st  # a swapped ax / ay or h / w puts the box elsewhere on a non-square level
        d = [s[1] * st for s in p["sides"]]
        want = torch.tensor([cx - d[0], cy - d[1], cx + d[2], cy + d[3]], dtype=torch.float64)
        assert (case["boxes"][p["b"], p["a"]] - want).abs().max() < 1e-9, (p, case["boxes"][p["b"], p["a"]], want)
        assert abs(float(case["scores"][p["b"], p["a"]]) - p["cls"][1]) < 1e-12
        f = case["flame"][p["b"], p["a"]]
        assert (f[: min(S, 3)] == 3.0 * p["sign"]).all() and (f[300 : 300 + min(E, 3)] == -3.0 * p["sign"]).all()
        assert (f[S:300] == 0).all() and (f[300 + E : 400] == 0).all()
        assert float(f[409]) == -5000.25 + cx and float(f[410]) == -12345.5 + cy and float(f[411]) == -3.0e4
        assert abs(float(f[412]) / (np.exp(p["scale"]) / 0.05 * st) - 1.0) < 1e-12
        seen.update(k for k, _ in p["sides"])
        seen.add(p["cls"][0])
    if len(case["plants"]) >= 5:
        assert seen >= {"bin0", "bin16", "bin8", "uniform", "large_equal", 100.0, -100.0, 0.0}


def gather_indices(case: dict) -> Dict[int, torch.Tensor]:
    """k -> idx [B,k] int64 for k in {1, 5, A}: the last anchor; the level-edge anchors with one index repeated; every anchor in po.decoding_topk's order"""
    A, B = case["A"], case["B"]
    starts = np.cumsum([0] + [h * w for h, w in case["sizes"]])
    edges = [0, int(starts[1]) - 1, A - 1, int(starts[-2]), 0]  # first / last of level 0, last of all, first of the last level, the first again
    out = {1: torch.full((B, 1), A - 1, dtype=torch.int64), 5: torch.tensor(edges, dtype=torch.int64).repeat(B, 1)}
    for b in range(1, B):
        out[5][b] = out[5][b].flip(0)
    out[A] = po.decoding_topk(case["boxes"], case["scores"][..., None], case["flame"], A)[3]
    return out


def gather_reference(case: dict, idx: torch.Tensor):
    B = case["B"]
    return torch.stack([case["boxes"][b, idx[b]] for b in range(B)]), torch.stack([case["flame"][b, idx[b]] for b in range(B)])


# seeded crowd for the helper check of the host test
def helper_crowd(seed: int = 11, n: int = 400):
    rng = _rng(seed)
    boxes = _crowd(rng, n, 30)
    scores = np.sort(rng.uniform(0.05, 0.99, n).astype(np.float32))[::-1].copy()
    return boxes, scores

