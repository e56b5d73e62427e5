"""GPU (-m gpu): the C entry points of csrc/postproc.hip on the planted cases of tests/postproc_cases.py -- vgh_topk, vgh_nms + vgh_compact, vgh_topk_nms (also through
utils.nms_batched / utils.nms), vgh_head_decode + vgh_gather_candidates -- against oracle/postproc_oracle.py.  Plain tensors in, no engine, no FLAME model.

Integer outputs and floats that are copies (indices, counts, keep positions, gathered boxes, scores, FLAME rows) compare BITWISE.  Computed floats use the bars of
test_gpu_parity.py::test_head_decode_and_gather_vs_oracle against the float64 oracle: boxes 2e-4 px (strides <= 32), scores 2e-6, FLAME |d| / (|ref| + 1) < 1e-5, the
zero-padded channels exactly 0.  Every output is a Guarded buffer: 64 sentinel elements in front and behind, the payload prefilled with the same sentinel (a NaN bit
pattern no case contains), so a write out of bounds, a row left unwritten and "nothing written" on a refusal are all visible.  The workspace of vgh_topk_nms is exactly
vgh_topk_nms_workspace_bytes(...) between such bands.

Wall seconds per test on an MI355X box (uploads, CPU oracle and comparisons included; ~2 s of imports once per process): see SECONDS_MEASURED."""
import functools

import numpy as np
import pytest
import torch

import postproc_cases as pc

pytestmark = pytest.mark.gpu

VGH_ERR_INVALID = -1
GUARD = 64

# wall seconds of the slowest case of each test, from `pytest --durations=0` on an MI355X box; the whole file (45 cases): 2.5 s
SECONDS_MEASURED = {"test_topk_planted_rows": 0.09, "test_topk_without_the_scores_output": 0.005, "test_nms_and_compact_planted": 0.05, "test_compact_without_flame": 0.02,
                    "test_topk_nms_planted": 0.08, "test_utils_nms_is_image_0_only": 0.005, "test_topk_nms_flame_widths": 0.11, "test_topk_nms_refusals_write_nothing": 0.005,
                    "test_head_decode_and_gather_planted": 0.03, "test_head_decode_and_gather_refusals_write_nothing": 0.005}


def _dev():
    return torch.device("cuda", 0)


def _sp():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """[GUARD | n | GUARD] 4-byte elements on the device, every one of them the sentinel until somebody writes"""

    def __init__(self, n, kind):
        self.n, self.bits = int(n), (pc.SENTINEL_BITS if kind == "f" else pc.SENTINEL_I32)
        self.raw = torch.full((GUARD + self.n + GUARD,), self.bits, dtype=torch.int32, device=_dev())
        self.ptr = self.raw.data_ptr() + 4 * GUARD

    def i32(self, *shape):
        a = self.raw[GUARD : GUARD + self.n].cpu().numpy()
        return a.reshape(shape) if shape else a

    def u32(self, *shape):
        return self.i32(*shape).view(np.uint32)

    def f32(self, *shape):
        return self.i32(*shape).view(np.float32)

    def guards_intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:GUARD] == self.bits).all() and (r[GUARD + self.n :] == self.bits).all())

    def untouched(self):
        return bool((self.raw == self.bits).all())

    def complete(self):
        """no payload element still holds the sentinel: every row was written"""
        return not bool((self.raw[GUARD : GUARD + self.n] == self.bits).any())


def _up(a):
    """numpy -> device, bit for bit; an empty array still gets a valid pointer"""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.float32, device=_dev())
    return torch.from_numpy(a).to(_dev())


def _bits(a):
    return pc.f32_bits(a)


# ======================================================================================================
# vgh_topk
# ======================================================================================================
@pytest.mark.parametrize("A,k", pc.TOPK_PAIRS)
def test_topk_planted_rows(gpu_lib, A, k):
    scores = pc.topk_scores(A, k)
    B = len(scores)
    ref = pc.topk_reference(scores, k)
    d = _up(scores)
    idx, out = Guarded(B * k, "i"), Guarded(B * k, "f")
    assert gpu_lib.vgh_topk(d.data_ptr(), B, A, k, idx.ptr, out.ptr, _sp()) == 0
    got_idx, got_bits = idx.i32(B, k), out.u32(B, k)
    assert idx.guards_intact() and out.guards_intact()
    bad = [name for b, name in enumerate(pc.TOPK_ROWS) if not np.array_equal(got_idx[b], ref[b])]
    assert not bad, f"(A, k) = {(A, k)}: order differs from po.stable_topk on rows {bad}"
    bad = [name for b, name in enumerate(pc.TOPK_ROWS) if not np.array_equal(got_bits[b], _bits(scores[b][ref[b]]))]
    assert not bad, f"(A, k) = {(A, k)}: topk_scores are not the original bits on rows {bad}"
    for b, name in enumerate(pc.TOPK_ROWS):
        pc.topk_claim(name, scores[b], k, got_idx[b])


def test_topk_without_the_scores_output(gpu_lib):
    A, k = 1500, 1000
    scores = pc.topk_scores(A, k)
    B = len(scores)
    d = _up(scores)
    idx = Guarded(B * k, "i")
    assert gpu_lib.vgh_topk(d.data_ptr(), B, A, k, idx.ptr, None, _sp()) == 0
    assert np.array_equal(idx.i32(B, k), pc.topk_reference(scores, k)) and idx.guards_intact()


# ======================================================================================================
# vgh_nms + vgh_compact
# ======================================================================================================
@functools.lru_cache(maxsize=None)
def _nms_cases():
    return pc.nms_cases()


def _run_nms(lib, c):
    B, n = c["scores"].shape
    kk = c["keep_k"]
    db, ds = _up(c["boxes"]), _up(c["scores"])
    keep, counts = Guarded(B * kk, "i"), Guarded(B, "i")
    assert lib.vgh_nms(db.data_ptr(), ds.data_ptr(), B, n, float(c["conf"]), float(c["iou"]), kk, keep.ptr, counts.ptr, _sp()) == 0
    assert keep.guards_intact() and counts.guards_intact()
    return db, ds, keep, counts


@pytest.mark.parametrize("name", list(pc.nms_cases()))
def test_nms_and_compact_planted(gpu_lib, name):
    c = _nms_cases()[name]
    B, n = c["scores"].shape
    kk = c["keep_k"]
    ref_keep, ref_counts = pc.nms_reference(c)
    db, ds, keep, counts = _run_nms(gpu_lib, c)
    got_keep, got_counts = keep.i32(B, kk), counts.i32(B)
    assert got_counts.tolist() == ref_counts.tolist(), (name, got_counts, ref_counts)
    assert np.array_equal(got_keep, ref_keep), (name, got_keep[:, :12], ref_keep[:, :12])
    c["claim"](got_keep, got_counts)
    # vgh_compact on the device's own keep_idx: rows copied verbatim, zeros behind the count out to keep_k
    flame = pc.flame_rows(B, n, 413)
    df = _up(flame)
    ob, os_, of = Guarded(B * kk * 4, "f"), Guarded(B * kk, "f"), Guarded(B * kk * 413, "f")
    assert gpu_lib.vgh_compact(db.data_ptr(), ds.data_ptr(), df.data_ptr(), B, n, keep.ptr, kk, ob.ptr, os_.ptr, of.ptr, _sp()) == 0
    rb, rs, rf = pc.compact_reference(c["boxes"], c["scores"], flame, ref_keep)
    assert np.array_equal(ob.u32(B, kk, 4), _bits(rb)) and np.array_equal(os_.u32(B, kk), _bits(rs)) and np.array_equal(of.u32(B, kk, 413), _bits(rf))
    assert ob.guards_intact() and os_.guards_intact() and of.guards_intact()
    assert np.array_equal(keep.i32(B, kk), ref_keep) and counts.i32(B).tolist() == ref_counts.tolist()  # (compact reads them only)


def test_compact_without_flame(gpu_lib):
    c = _nms_cases()["sizes_1000_100"]
    B, n = c["scores"].shape
    kk = c["keep_k"]
    ref_keep, _ = pc.nms_reference(c)
    db, ds, keep, counts = _run_nms(gpu_lib, c)
    ob, os_ = Guarded(B * kk * 4, "f"), Guarded(B * kk, "f")
    assert gpu_lib.vgh_compact(db.data_ptr(), ds.data_ptr(), None, B, n, keep.ptr, kk, ob.ptr, os_.ptr, None, _sp()) == 0
    rb, rs, _ = pc.compact_reference(c["boxes"], c["scores"], None, ref_keep)
    assert np.array_equal(ob.u32(B, kk, 4), _bits(rb)) and np.array_equal(os_.u32(B, kk), _bits(rs))
    assert ob.guards_intact() and os_.guards_intact() and keep.guards_intact() and counts.guards_intact()


# ======================================================================================================
# vgh_topk_nms / utils.nms_batched / utils.nms
# ======================================================================================================
@functools.lru_cache(maxsize=None)
def _tn_cases():
    cases = pc.topk_nms_cases()
    return {name: (c, pc.topk_nms_reference(c)) for name, c in cases.items()}


class _TopkNmsCall:
    """one vgh_topk_nms call on Guarded outputs and an exact-size Guarded workspace"""

    def __init__(self, lib, boxes, scores, flame, width, conf, iou, pre_k, keep_k, B=None, n=None, ws_offset=0, out_flame=True, ws_sizes=None):
        B0, n0 = scores.shape
        self.B, self.n = (B0 if B is None else B), (n0 if n is None else n)
        nbytes = int(lib.vgh_topk_nms_workspace_bytes(*(ws_sizes or (max(self.B, 1), max(self.n, 1), pre_k, max(keep_k, 1)))))
        assert nbytes % 4 == 0
        self.ws = Guarded(nbytes // 4, "i")
        assert self.ws.ptr % 16 == 0
        kk = max(keep_k, 1)
        self.ob, self.os, self.counts = Guarded(B0 * kk * 4, "f"), Guarded(B0 * kk, "f"), Guarded(B0, "i")
        self.of = Guarded(B0 * kk * (width or 1), "f")
        self.keep = (_up(boxes), _up(scores), None if flame is None else _up(flame))
        self.rc = lib.vgh_topk_nms(self.keep[0].data_ptr(), self.keep[1].data_ptr(), None if flame is None else self.keep[2].data_ptr(), width or 0, self.B, self.n,
                                   float(conf), float(iou), pre_k, keep_k, self.ws.ptr + ws_offset, self.ob.ptr, self.os.ptr, self.of.ptr if out_flame else None,
                                   self.counts.ptr, _sp())
        torch.cuda.synchronize()

    def outputs(self):
        return self.ob, self.os, self.of, self.counts

    def assert_nothing_written(self):
        assert all(g.untouched() for g in (self.ob, self.os, self.of, self.counts, self.ws))

    def assert_guards(self):
        assert all(g.guards_intact() for g in (self.ob, self.os, self.of, self.counts, self.ws))


def _assert_slabs(call, c, ref, flame, kk):
    B = len(ref)
    rb, rs, rf, rc = pc.topk_nms_slabs(c, ref, flame)
    assert call.rc == 0
    call.assert_guards()
    assert call.counts.i32(B).tolist() == rc.tolist(), (call.counts.i32(B), rc)
    assert np.array_equal(call.ob.u32(B, kk, 4), _bits(rb)) and np.array_equal(call.os.u32(B, kk), _bits(rs))
    if flame is not None:
        assert np.array_equal(call.of.u32(B, kk, flame.shape[2]), _bits(rf))
    else:
        assert call.of.untouched()


@pytest.mark.parametrize("name", ["unsorted_ties", "more_than_pre_k", "nan_displaces", "nan_displaces_keep_all"])
def test_topk_nms_planted(gpu_lib, name):
    from head_detector_amd.utils import nms_batched

    c, ref = _tn_cases()[name]
    B, n = c["scores"].shape
    kk = c["keep_k"]
    flame = pc.flame_rows(B, n, 413)
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], flame, 413, c["conf"], c["iou"], c["pre_k"], kk)
    _assert_slabs(call, c, ref, flame, kk)
    # the facade: the same call on the caller's tensors, scores [B,n,1]
    ob, os_, of, counts = nms_batched(_up(c["boxes"]), _up(c["scores"])[..., None], _up(flame), c["conf"], c["iou"], top_k=c["pre_k"], keep_top_k=kk)
    rb, rs, rf, rc = pc.topk_nms_slabs(c, ref, flame)
    assert counts.cpu().numpy().tolist() == rc.tolist()
    assert np.array_equal(_bits(ob.cpu().numpy()), _bits(rb)) and np.array_equal(_bits(os_.cpu().numpy()), _bits(rs)) and np.array_equal(_bits(of.cpu().numpy()), _bits(rf))


def test_utils_nms_is_image_0_only(gpu_lib):
    from head_detector_amd.utils import nms

    c, ref = _tn_cases()["unsorted_ties"]
    B, n = c["scores"].shape
    flame = pc.flame_rows(B, n, 413)
    assert not np.array_equal(ref[0][2], ref[1][2])  # image 1 differs
    b0, s0, f0 = nms(_up(c["boxes"]), _up(c["scores"])[..., None], _up(flame), c["conf"], c["iou"], top_k=c["pre_k"], keep_top_k=c["keep_k"])
    rb, rs, rows = ref[0]
    assert np.array_equal(_bits(b0.cpu().numpy()), _bits(rb)) and np.array_equal(_bits(s0.cpu().numpy()), _bits(rs)) and np.array_equal(_bits(f0.cpu().numpy()), _bits(flame[0, rows]))


@pytest.mark.parametrize("width", pc.WIDTHS)
def test_topk_nms_flame_widths(gpu_lib, width):
    c, ref = _tn_cases()["widths"]
    B, n = c["scores"].shape
    kk = c["keep_k"]
    assert kk > min(c["pre_k"], n)  # keep_k > k: the slab is longer than the candidate list
    flame = None if width is None else pc.flame_rows(B, n, width)
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], flame, width, c["conf"], c["iou"], c["pre_k"], kk, out_flame=flame is not None)
    _assert_slabs(call, c, ref, flame, kk)


def test_topk_nms_refusals_write_nothing(gpu_lib):
    c, _ = _tn_cases()["widths"]
    B, n = c["scores"].shape
    fl = pc.flame_rows(B, n, 7)
    a = dict(conf=0.5, iou=0.5, pre_k=1000, keep_k=8)
    # flame on one side only
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], fl, 7, out_flame=False, **a)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], None, 7, out_flame=True, **a)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    # min(pre_k, n) = 1025
    big_b, big_s = np.tile(c["boxes"][:, :1], (1, 1025, 1)), np.tile(c["scores"][:, :1], (1, 1025))
    call = _TopkNmsCall(gpu_lib, big_b, big_s, None, None, 0.5, 0.5, 1025, 8, out_flame=False)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    # a workspace 8 bytes off the 16-byte grid
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], None, None, out_flame=False, ws_offset=8, **a)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    # n = 0, keep_k = 0
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], None, None, out_flame=False, n=0, **a)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], None, None, 0.5, 0.5, 1000, 0, out_flame=False)
    assert call.rc == VGH_ERR_INVALID
    call.assert_nothing_written()
    # B = 0 is not an error, and writes nothing
    call = _TopkNmsCall(gpu_lib, c["boxes"], c["scores"], None, None, out_flame=False, B=0, **a)
    assert call.rc == 0
    call.assert_nothing_written()


# ======================================================================================================
# vgh_head_decode + vgh_gather_candidates
# ======================================================================================================
def _levels(case, dp, n=None, pitches=None):
    from head_detector_amd import _lib

    n = len(dp) if n is None else n
    pitches = pitches or case["pitches"]
    lv = [_lib.HeadLevel(dp[i].data_ptr(), case["sizes"][i][0], case["sizes"][i][1], pitches[i], case["strides"][i]) for i in range(len(dp))]
    while len(lv) < 5:
        lv.append(lv[-1])
    return (_lib.HeadLevel * 5)(*lv)


def _decode(lib, case):
    B, A = case["B"], case["A"]
    dp = [t.to(_dev()).contiguous() for t in case["preds"]]
    lv = _levels(case, dp)
    boxes, scores = Guarded(B * A * 4, "f"), Guarded(B * A, "f")
    assert lib.vgh_head_decode(lv, len(dp), B, boxes.ptr, scores.ptr, _sp()) == 0
    assert boxes.guards_intact() and scores.guards_intact() and boxes.complete() and scores.complete()
    return dp, lv, boxes, scores


@pytest.mark.parametrize("geometry", list(pc.GEOMETRIES))
def test_head_decode_and_gather_planted(gpu_lib, geometry):
    for S, E in pc.LIVE_PAIRS:
        case = pc.decode_case(geometry, S, E)
        pc.decode_claim(case)
        B, A, nl = case["B"], case["A"], len(case["sizes"])
        dp, lv, boxes, scores = _decode(gpu_lib, case)
        gb, gs = torch.from_numpy(boxes.f32(B, A, 4).copy()), torch.from_numpy(scores.f32(B, A).copy())
        eb, es = float((gb.double() - case["boxes"]).abs().max()), float((gs.double() - case["scores"]).abs().max())
        print(f"[postproc cases] {geometry} S={S} E={E}: boxes {eb:.2e} px, scores {es:.2e}")
        assert eb < 2e-4, (geometry, S, E, eb)
        assert es < 2e-6, (geometry, S, E, es)
        for k, idx in pc.gather_indices(case).items():
            didx = idx.to(torch.int32).to(_dev())
            rb, rf = pc.gather_reference(case, idx)
            for with_flame in (True, False) if k == 5 else (True,):
                ob, of = Guarded(B * k * 4, "f"), Guarded(B * k * 413, "f")
                assert gpu_lib.vgh_gather_candidates(lv, nl, B, A, S, E, boxes.ptr, didx.data_ptr(), k, ob.ptr, of.ptr if with_flame else None, _sp()) == 0
                assert ob.guards_intact() and of.guards_intact() and ob.complete()
                own = torch.stack([gb[b, idx[b]] for b in range(B)])
                assert np.array_equal(ob.u32(B, k, 4), _bits(own.numpy()))  # copies of the decode's rows
                assert float((torch.from_numpy(ob.f32(B, k, 4).copy()).double() - rb).abs().max()) < 2e-4
                if not with_flame:
                    assert of.untouched()
                    continue
                assert of.complete()
                gf = torch.from_numpy(of.f32(B, k, 413).copy())
                d = float(((gf.double() - rf).abs() / (rf.abs() + 1.0)).max())
                assert d < 1e-5, (geometry, S, E, k, d)
                assert bool((gf[..., S:300] == 0).all()) and bool((gf[..., 300 + E : 400] == 0).all())  # (empty for S = 300 / E = 100)
        assert boxes.guards_intact() and scores.guards_intact()


def test_head_decode_and_gather_refusals_write_nothing(gpu_lib):
    S, E = 128, 64
    case = pc.decode_case("non_square", S, E)
    B, A, nl = case["B"], case["A"], len(case["sizes"])
    dp = [t.to(_dev()).contiguous() for t in case["preds"]]
    lv = _levels(case, dp)
    boxes, scores = Guarded(B * A * 4, "f"), Guarded(B * A, "f")
    ob, of = Guarded(B * 5 * 4, "f"), Guarded(B * 5 * 413, "f")
    didx = pc.gather_indices(case)[5].to(torch.int32).to(_dev())
    src = torch.zeros(B * A * 4, device=_dev())

    def gather(levels=lv, n_levels=nl, A_=A, S_=S, E_=E):
        return gpu_lib.vgh_gather_candidates(levels, n_levels, B, A_, S_, E_, src.data_ptr(), didx.data_ptr(), 5, ob.ptr, of.ptr, _sp())

    short = [p for p in case["pitches"]]
    short[-1] = 72 + S + E + 13 - 1
    assert gather(A_=A + 1) == VGH_ERR_INVALID and gather(A_=A - 1) == VGH_ERR_INVALID  # A not matching the levels
    assert gather(levels=_levels(case, dp, pitches=short)) == VGH_ERR_INVALID  # pitch too small by one
    assert gather(n_levels=0) == VGH_ERR_INVALID and gather(n_levels=5) == VGH_ERR_INVALID
    assert gather(S_=301) == VGH_ERR_INVALID and gather(E_=101) == VGH_ERR_INVALID
    for n_levels, levels in ((0, lv), (5, lv), (nl, _levels(case, dp, pitches=[case["pitches"][0], 68]))):  # decode: its own smallest pitch is 69
        assert gpu_lib.vgh_head_decode(levels, n_levels, B, boxes.ptr, scores.ptr, _sp()) == VGH_ERR_INVALID
    torch.cuda.synchronize()
    assert all(g.untouched() for g in (boxes, scores, ob, of))
    assert gather() == 0  # the same arguments, none of them wrong
    assert ob.complete() and of.complete()
