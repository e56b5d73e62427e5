"""No GPU: every planted case of tests/postproc_cases.py is what its name says -- each claim runs on the oracle's own result (oracle/postproc_oracle.py), so the
device comparison of tests/test_gpu_postproc_cases.py can never be over an empty case -- and the helper that turns nms_torchvision output into vgh_nms's keep_idx
positions agrees with _nms_one."""
import numpy as np
import pytest
import torch

import postproc_cases as pc
from oracle import postproc_oracle as po


@pytest.mark.parametrize("A,k", pc.TOPK_PAIRS)
def test_topk_rows_hold_what_they_are_named_for(A, k):
    scores = pc.topk_scores(A, k)
    assert scores.shape == (len(pc.TOPK_ROWS), A) and scores.dtype == np.float32
    assert np.array_equal(pc.f32_bits(scores), pc.f32_bits(pc.topk_scores(A, k)))  # deterministic
    assert not (pc.f32_bits(scores) == pc.SENTINEL_BITS).any()
    ref = pc.topk_reference(scores, k)
    for b, name in enumerate(pc.TOPK_ROWS):
        pc.topk_claim(name, scores[b], k, ref[b])


def test_stable_topk_order_of_the_special_values():
    """the order the contract is written from: every NaN first by index, +inf, ..., the two zeros tied, ..., -inf"""
    nan = np.float32(np.nan)
    v = torch.tensor([0.5, -0.0, nan, 0.0, np.inf, 0.5, -nan, -np.inf, 0.0, -0.0])
    assert po.stable_topk(v, 10).tolist() == [2, 6, 4, 0, 5, 1, 3, 8, 9, 7]


def test_nms_cases_hold_what_they_are_named_for():
    cases = pc.nms_cases()
    assert {f"sizes_{n}_{k}" for n, k in pc.NMS_SIZES} <= set(cases) and {"dead_suppressor", "nan_head"} <= set(cases)
    assert sum(n.startswith("thresholds_") for n in cases) == 8
    for name, c in cases.items():
        keep, counts = pc.nms_reference(c)
        c["claim"](keep, counts)
        if name != "nan_head":
            assert np.isfinite(c["scores"]).all(), name
            assert (np.diff(c["scores"], axis=1) <= 0).all(), name  # the documented precondition of vgh_nms
        assert np.isfinite(c["boxes"]).all()


def test_keep_positions_equals_nms_one_on_a_crowd():
    boxes, scores = pc.helper_crowd()
    for conf, iou, keep_k in [(0.5, 0.5, 100), (0.05, 0.3, 1000), (0.9, 0.7, 5)]:
        keep, count = pc.keep_positions(boxes, scores, conf, iou, keep_k)
        rb, rs, rf = po._nms_one(torch.from_numpy(boxes), torch.from_numpy(scores)[:, None], torch.arange(len(scores), dtype=torch.float64)[:, None], conf, iou, 1000, keep_k)
        assert count == len(rs) > 1 and (keep[count:] == -1).all()
        assert rf[:, 0].long().tolist() == keep[:count].tolist()
        assert np.array_equal(boxes[keep[:count]], rb.numpy()) and np.array_equal(scores[keep[:count]], rs.numpy())
    assert count < 20 or keep_k == 5


def test_topk_nms_cases_hold_what_they_are_named_for():
    cases = pc.topk_nms_cases()
    assert set(cases) == {"unsorted_ties", "more_than_pre_k", "nan_displaces", "nan_displaces_keep_all", "widths"}
    for name, c in cases.items():
        ref = pc.topk_nms_reference(c)
        c["claim"](ref)
        assert np.isfinite(c["scores"]).all() or name.startswith("nan_"), name
        fl = pc.flame_rows(len(ref), c["boxes"].shape[1], 7)
        ob, os_, of, counts = pc.topk_nms_slabs(c, ref, fl)  # (asserts that the rows gathered from the ORIGINAL tensors are _nms_one's)
        assert (counts > 0).all() and of.shape == (len(ref), c["keep_k"], 7)
    c = cases["more_than_pre_k"]
    assert c["boxes"].shape[1] == 1500 and c["pre_k"] == 1000 and c["keep_k"] == 100


@pytest.mark.parametrize("geometry", list(pc.GEOMETRIES))
def test_decode_cases_hold_what_they_are_named_for(geometry):
    for S, E in pc.LIVE_PAIRS:
        case = pc.decode_case(geometry, S, E)
        pc.decode_claim(case)
        sizes, strides, B, extra = pc.GEOMETRIES[geometry]
        assert all(t.shape == (B, h, w, p) for t, (h, w), p in zip(case["preds"], sizes, case["pitches"]))
        assert all(p >= 72 + S + E + 13 for p in case["pitches"]) and max(strides) <= 32
        assert all(torch.isfinite(t).all() for t in case["preds"])
        idx = pc.gather_indices(case)
        assert set(idx) == {1, 5, case["A"]} and case["A"] <= 1024
        for k, ix in idx.items():
            assert ix.shape == (B, k) and int(ix.min()) >= 0 and int(ix.max()) < case["A"]
        assert len(set(idx[5][0].tolist())) < 5  # one index repeated
        assert sorted(idx[case["A"]][0].tolist()) == list(range(case["A"]))
        gb, gf = pc.gather_reference(case, idx[5])
        assert gb.shape == (B, 5, 4) and gf.shape == (B, 5, 413)
