"""GPU (-m gpu): the select stage on DESIGNED candidates, and the contract between the candidate stage, the network and the select.

The network is not run for the planted cases: tests/select_fixture.py writes the level prediction tensors (exact whole-bin boxes, chosen scores with exact ties, random
FLAME channels) straight into the net's fp32 prediction buffers, ``eng.candidates`` decodes them and ``eng.select`` -- nms_select_kernel, lazy gather included --
runs on a candidate set whose every property tests/test_select_cases_host.py has checked against the oracle.  Tolerances are those of
test_head_decode_and_gather_vs_oracle (2e-4 px, 2e-6, 1e-5 relative on |x| + 1) for the candidate stage; everything behind it is torch.equal.

The stage-order tests pin the enforced contract of csrc/detect.hip: a lazily gathered batch can be selected any number of times while the net's forward generation
stands, and is refused -- on the host, before any launch -- once a forward has been queued, when rows have no source, or when lazy and eager rows are mixed."""
import ctypes as C

import pytest
import torch

import select_fixture as sf

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _engine(S, max_batch, keep_k=100, **kw):
    from head_detector_amd.engine import VGHeadsEngine

    return VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=max_batch, seed=3, keep_top_k=keep_k, **kw)


def _pred_views(eng):
    """Writable views of the level prediction buffers, f32 [arena_batch, h, w, pitch] (the level table engine.py builds above ``buffer()``)."""
    from head_detector_amd.engine import _alias

    return [_alias(eng.lib.vgh_net_buffer(eng._net, lv["buf"]), (eng.arena_batch, lv["h"], lv["w"], lv["pitch"]), "<f4", eng.device) for lv in eng.program.levels]


def _plant(eng, preds, lo=0, n=None):
    """Images [lo, lo + n) of the planted tensors into prediction rows [0, n)."""
    n = preds[0].shape[0] - lo if n is None else n
    assert n <= eng.arena_batch
    torch.cuda.synchronize()
    for view, t in zip(_pred_views(eng), preds):
        assert view.shape[1:] == t.shape[1:]
        view[:n].copy_(t[lo : lo + n].to(eng.device))
    torch.cuda.synchronize()


def _settle(eng):
    eng.join()
    torch.cuda.synchronize()


def _select(eng, B, conf=sf.CONF, iou=sf.IOU, cap=0):
    """vgh_detector_select with the head list (n_heads, head_image; no FLAME decode) -> host copies of everything it writes."""
    from head_detector_amd import _lib
    from head_detector_amd.engine import _alias

    kk = eng.keep_k
    o, det = eng._detect_out(B, None, None)
    n_heads = torch.full((1,), -7, dtype=torch.int32, device=eng.device)
    head_image = torch.full((B * kk,), -1, dtype=torch.int32, device=eng.device)
    o.n_heads_dev, o.head_image_dev, o.head_capacity = n_heads.data_ptr(), head_image.data_ptr(), cap
    _settle(eng)
    _lib.check(eng.lib.vgh_detector_select(eng._det, B, float(conf), float(iou), C.byref(o), eng._sp()))
    _settle(eng)
    head_row = _alias(eng.lib.vgh_detector_scratch(eng._det, _lib.SCRATCH_HEAD_ROW), (eng.max_batch * kk,), "<i4", eng.device)
    return dict(boxes=det.boxes.cpu(), scores=det.scores.cpu(), flame=det.flame_params.cpu(), counts=det.counts.cpu(), n_heads=int(n_heads.item()),
                head_image=head_image.cpu(), head_row=head_row[: B * kk].cpu())


def _equal_outputs(a, b, where):
    n = a["n_heads"]
    assert n == b["n_heads"], where
    for k in ("boxes", "scores", "flame", "counts"):
        assert torch.equal(a[k], b[k]), (where, k)
    assert torch.equal(a["head_image"], b["head_image"]) and torch.equal(a["head_row"][:n], b["head_row"][:n]), where


def _check_against_oracle(got, ref, B, keep_k, cap, where):
    """``got`` (``_select``) against ``ref`` = postprocess_batched per image: counts, kept rows, zeros behind the count, the image-major head list cut at ``cap``."""
    counts = [r[0].shape[0] for r in ref]
    assert got["counts"].tolist() == counts, (where, got["counts"].tolist(), counts)
    for b in range(B):
        n = counts[b]
        assert torch.equal(got["boxes"][b, :n], ref[b][0]) and torch.equal(got["scores"][b, :n], ref[b][1]) and torch.equal(got["flame"][b, :n], ref[b][2]), (where, b)
        assert not bool(got["boxes"][b, n:].any()) and not bool(got["scores"][b, n:].any()) and not bool(got["flame"][b, n:].any()), (where, b)
    images = [b for b, c in enumerate(counts) for _ in range(c)]
    rows = [b * keep_k + i for b, c in enumerate(counts) for i in range(c)]
    n = min(len(images), cap) if cap > 0 else len(images)
    assert got["n_heads"] == n, (where, got["n_heads"], n)
    assert got["head_image"][:n].tolist() == images[:n] and got["head_row"][:n].tolist() == rows[:n], where
    assert bool((got["head_image"][n:] == -1).all()), where  # nothing written behind the capacity / the count


def _mid_image_capacity(counts):
    """A head capacity that ends inside an image (the first one with two or more survivors; with keep_k = 1 there is none: one head short of the total)."""
    at = 0
    for c in counts:
        if c >= 2 and at > 0:
            return at + c // 2
        at += c
    return max(1, at - 1)


# (image size, keep_top_k): 525 anchors (pre_k = A) and 1344 (pre_k = 1000); keep_k 1, the default 100, and pre_k
CONFIGS = [(160, 1), (160, 100), (160, 525), (256, 1), (256, 100), (256, 1000)]


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_planted_cases_candidates_and_select_vs_oracle(gpu_lib, S, keep_k, overlap):
    """Every planted case as one batch: the candidate stage against ndfl_decode / decoding_topk, the eager select against postprocess_batched of the engine's own
    candidates (at IoU 0.5 and at 0.45, with a head capacity that ends inside an image, twice through the detector: the ticket is back at zero), and the lazy route
    bit for bit against the eager one -- with the candidate FLAME tensor poisoned, which the lazy route must not read."""
    B = len(sf.CASE_NAMES)
    eng = _engine(S, B, keep_k)
    eng.set_overlap(overlap)
    geo = sf.geometry_of(eng.program)
    assert eng.pre_k == min(1000, geo.A) and eng.keep_k == keep_k
    cs = sf.build_case_set(geo, eng.pre_k, keep_k)
    (rb, rs, rf), (obb, oss, off, oidx) = sf.oracle_view(cs)
    # ---- candidate stage, eager ----
    _plant(eng, cs.preds)
    eng.candidates(B, lazy_flame=False)
    _settle(eng)
    assert float((eng.boxes_all[:B].cpu() - rb).abs().max()) < 2e-4
    assert float((eng.scores_all[:B].cpu() - rs[..., 0]).abs().max()) < 2e-6
    assert torch.equal(eng.idx[:B].cpu().long(), oidx)  # the top-k order is exact, ties by ascending anchor index
    cs.patch_boxes(eng.cand_boxes)  # the inverted boxes, over their planted ranks
    _settle(eng)
    cb, csc, cf = eng.cand_boxes[:B].cpu(), eng.cand_scores[:B].cpu(), eng.cand_flame[:B].cpu()
    assert float((cb - obb).abs().max()) < 2e-4 and float((csc - oss[..., 0]).abs().max()) < 2e-6
    d = (cf - off).abs() / (off.abs() + 1.0)
    assert float(d.max()) < 1e-5, float(d.max())
    assert float(cf[..., geo.shape_c:300].abs().max()) == 0.0 and float(cf[..., 300 + geo.expr_c : 400].abs().max()) == 0.0  # dead shape / expression channels
    # the planted boxes are whole bins: exact in fp32 on both sides, so the IoU-at-the-threshold and tie cases reach the select as the host test checked them
    assert torch.equal(cb, obb)
    # ---- select, eager ----
    eager = {}
    for iou in (sf.IOU, sf.IOU_ALT):
        ref = sf.oracle_select(cs, cb, csc, cf, sf.CONF, iou)
        counts = [r[0].shape[0] for r in ref]
        assert counts == [r[0].shape[0] for r in sf.oracle_select(cs, obb, oss, off, sf.CONF, iou)]  # and the oracle's own candidates give the same survivors
        assert 0 in counts and max(counts) == keep_k
        for rnd in range(2):
            got = _select(eng, B, sf.CONF, iou)
            _check_against_oracle(got, ref, B, keep_k, 0, (iou, rnd))
        eager[iou] = got
        cap = _mid_image_capacity(counts)
        assert 0 < cap < sum(counts)
        eager[iou, "cap"] = _select(eng, B, sf.CONF, iou, cap=cap)
        _check_against_oracle(eager[iou, "cap"], ref, B, keep_k, cap, (iou, "cap", cap))
    # ---- lazy route: same planted buffers, candidate FLAME rows poisoned ----
    eng.cand_flame.fill_(float("nan"))
    _settle(eng)
    eng.candidates(B, lazy_flame=True)
    _settle(eng)
    assert bool(torch.isnan(eng.cand_flame).all())  # the lazy candidate stage writes no candidate vector
    cs.patch_boxes(eng.cand_boxes)
    for iou in (sf.IOU, sf.IOU_ALT):
        for rnd in range(2):  # any number of selects on one lazy candidate stage
            _equal_outputs(_select(eng, B, sf.CONF, iou), eager[iou], ("lazy", iou, rnd))
        cap = _mid_image_capacity(eager[iou]["counts"].tolist())
        _equal_outputs(_select(eng, B, sf.CONF, iou, cap=cap), eager[iou, "cap"], ("lazy", iou, "cap"))
    eng.set_overlap(False)
    eng.close()


def test_select_head_list_over_more_than_1024_images(gpu_lib):
    """The last-block scan of nms_select_kernel with two images per thread (per = 2 needs B > 1024): 1100 random planted images at the smallest image size the program
    accepts (32 px: 21 anchors), filled in arena-sized eager chunks with candidates(n, at).  Sized from detect.hip's allocations: 1100 images x (21 anchors x 5 floats
    + 21 candidates x (1 + 1 + 4 + 413) + 8 x 3 ints) x 4 bytes = 39 MB, and 14.6 MB of output slabs: no share of HBM worth the name, so B is not reduced."""
    S, B, arena, keep_k = 32, 1100, 64, 8
    eng = _engine(S, B, keep_k, arena_batch=arena)
    assert eng.arena_batch == arena and eng.pre_k == 21
    geo = sf.geometry_of(eng.program)
    cs = sf.build_random_set(geo, eng.pre_k, keep_k, B)
    _, (obb, oss, off, oidx) = sf.oracle_view(cs)
    for at in range(0, B, arena):
        n = min(arena, B - at)
        _plant(eng, cs.preds, at, n)
        eng.candidates(n, at=at)
    _settle(eng)
    assert torch.equal(eng.idx[:B].cpu().long(), oidx)
    cb, csc, cf = eng.cand_boxes[:B].cpu(), eng.cand_scores[:B].cpu(), eng.cand_flame[:B].cpu()
    assert torch.equal(cb, obb) and float((csc - oss[..., 0]).abs().max()) < 2e-6
    ref = sf.oracle_select(cs, cb, csc, cf)
    counts = [r[0].shape[0] for r in ref]
    assert counts == [r[0].shape[0] for r in sf.oracle_select(cs, obb, oss, off)] and counts.count(0) > 100 and counts.count(keep_k) > 100
    for rnd in range(2):
        _check_against_oracle(_select(eng, B), ref, B, keep_k, 0, rnd)
    b = next(i for i in range(700, B) if counts[i] >= 2)  # a capacity that ends inside an image far into the scan
    cap = sum(counts[:b]) + counts[b] // 2
    _check_against_oracle(_select(eng, B, cap=cap), ref, B, keep_k, cap, ("cap", cap))
    eng.close()


# ======================================================================================================
# stage order
# ======================================================================================================
def _images(B, S, seed):
    return torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _snap(det, with_heads=True):
    keys = ("boxes", "scores", "flame_params", "counts") + (("vertices_3d", "head_pose", "head_image") if with_heads else ())
    return {k: getattr(det, k).clone() for k in keys}


def _same(a, b, where):
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k)


def _sentinel(eng):
    for t in (eng.out_boxes, eng.out_scores, eng.out_flame):
        t.fill_(-3.0)
    eng.counts.fill_(-3)
    _settle(eng)


def _untouched(eng):
    _settle(eng)
    return all(bool((t == -3).all()) for t in (eng.out_boxes, eng.out_scores, eng.out_flame, eng.counts))


def test_second_select_after_detect_uses_the_lazy_source_again(gpu_lib, flame_model):
    """detect(x, conf_a) gathers lazily; a following select(B, conf_b) on the same candidates must equal a fresh eager forward_candidates + select(conf_b) bit for bit
    (boxes, scores, 413-vectors, counts, vertices, pose).  Before the select kept its source state, the second select compacted candidate FLAME rows the lazy stage
    had never written -- here the rows of ANOTHER batch, put there first -- and returned them without an error."""
    from head_detector_amd.flame import FLAMELayer

    S, B = 256, 3
    xa, other = _images(B, S, 31), _images(B, S, 32)
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=B * 100)
    eng = _engine(S, B)
    scores = eng.model(xa)[1]
    conf_a, conf_b = float(scores[:, 4, 0].max()), float(scores[:, 40, 0].max())
    assert conf_b < conf_a
    eng.model(other)  # the candidate FLAME tensor now holds another batch's vectors
    first = _snap(eng.detect(xa, confidence_threshold=conf_a, flame=fl))
    det = eng.select(B, confidence_threshold=conf_b, flame=fl)
    _settle(eng)
    second = _snap(det)
    det = eng.select(B, confidence_threshold=conf_a, flame=fl)  # and back: as often as the caller likes
    _settle(eng)
    third = _snap(det)
    eng.forward_candidates(xa)
    det = eng.select(B, confidence_threshold=conf_b, flame=fl)
    _settle(eng)
    ref = _snap(det)
    assert int(ref["counts"].sum()) >= int(first["counts"].sum()) > 0
    _same(second, ref, "select(conf_b) after detect(conf_a)")
    _same(third, first, "select(conf_a) again")
    eng.close()


def test_lazy_rows_followed_by_an_eager_chunk_never_return_stale_rows(gpu_lib):
    """Lazy candidates(n, at=0), then eager candidates(m, at=n), then select(n + m): every row is right or the call raises -- it raises (the kernel gathers all survivors of
    a launch one way).  The lazy rows alone, and the batch once every chunk is eager, select fine."""
    from head_detector_amd._lib import VghError

    S, keep_k, n, m = 160, 100, 3, 3
    names = ("all_valid", "ties", "level_edges", "conf_equal", "iou_exact", "empty")
    eng = _engine(S, n + m, keep_k)
    geo = sf.geometry_of(eng.program)
    cs = sf.build_case_set(geo, eng.pre_k, keep_k, names=names)
    _plant(eng, cs.preds)
    eng.candidates(n + m, lazy_flame=False)  # rows [0, 6): an older batch, so no row is without a source
    eng.cand_flame.fill_(float("nan"))
    _settle(eng)
    eng.candidates(n, at=0, lazy_flame=True)
    eng.candidates(m, at=n, lazy_flame=False)  # prediction rows [0, 3) -- the same three images -- into candidate rows [3, 6)
    _settle(eng)
    cb, csc, cf = eng.cand_boxes[:n + m].cpu(), eng.cand_scores[:n + m].cpu(), eng.cand_flame[n:n + m].cpu()
    _sentinel(eng)
    try:
        got = _select(eng, n + m)
    except VghError as e:
        assert "mix" in str(e) and _untouched(eng)
    else:  # (an implementation that gathers the lazy rows eagerly instead: then every row has to be right)
        ref = sf.oracle_select(cs, cb, csc, torch.cat([cf, cf]))
        _check_against_oracle(got, ref, n + m, keep_k, 0, "lazy + eager")
    lazy_only = _select(eng, n)
    _check_against_oracle(lazy_only, sf.oracle_select(cs, cb[n:], csc[n:], cf), n, keep_k, 0, "the lazy rows alone")
    eng.candidates(n, at=0, lazy_flame=False)
    _check_against_oracle(_select(eng, n + m), sf.oracle_select(cs, cb, csc, torch.cat([cf, cf])), n + m, keep_k, 0, "all eager")
    # rows that no candidate stage has filled since a shorter lazy one replaced theirs
    eng.candidates(n, lazy_flame=True)
    eng.candidates(1, lazy_flame=True)
    _sentinel(eng)
    with pytest.raises(VghError, match="no valid source"):
        _select(eng, n)
    assert _untouched(eng)
    eng.close()


def test_select_of_rows_nobody_filled_is_refused(gpu_lib):
    from head_detector_amd._lib import VghError

    eng = _engine(160, 4)
    cs = sf.build_case_set(sf.geometry_of(eng.program), eng.pre_k, 100, names=("ties", "conf_equal"))
    _plant(eng, cs.preds)
    _sentinel(eng)
    with pytest.raises(VghError, match="no valid source"):
        _select(eng, 2)
    eng.candidates(2)
    with pytest.raises(VghError, match="no valid source"):
        _select(eng, 3)
    assert _untouched(eng)
    ref = sf.oracle_select(cs, eng.cand_boxes[:2].cpu(), eng.cand_scores[:2].cpu(), eng.cand_flame[:2].cpu())
    assert [r[0].shape[0] for r in ref] == [3, 3]  # (S = 160: three tie groups; two clear candidates and the one at the threshold)
    _check_against_oracle(_select(eng, 2), ref, 2, 100, 0, "the filled rows")
    eng.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_forward_between_lazy_candidates_and_select_is_refused(gpu_lib, use_graph):
    """Lazy candidates, then a forward of ANOTHER batch (eager launch or hipGraph replay), then the select: VghError on the host, nothing launched (the outputs keep their
    sentinel).  The engine recovers: the batch now in the arena decodes and selects as usual."""
    from head_detector_amd._lib import VghError

    S, B = 320, 2  # (the engine test_latency_lanes_are_invisible replays as a graph)
    xa, xb = _images(B, S, 41), _images(B, S, 42)
    eng = _engine(S, B)
    conf = float(eng.model(xb)[1][:, 20, 0].max())
    ref_b = _snap(eng.detect(xb, confidence_threshold=conf), with_heads=False)
    assert int(ref_b["counts"].sum()) > 0
    eng.forward_net(xa, use_graph=use_graph)
    eng.candidates(B, lazy_flame=True)
    eng.forward_net(xb if not use_graph else xa, use_graph=use_graph)  # (a replay re-runs the captured batch: the generation moves all the same)
    _sentinel(eng)
    with pytest.raises(VghError, match="forward"):
        eng.select(B, confidence_threshold=conf)
    assert _untouched(eng)
    if use_graph:
        eng.forward_net(xb)
    eng.candidates(B, lazy_flame=True)
    det = eng.select(B, confidence_threshold=conf)
    _settle(eng)
    _same(_snap(det, with_heads=False), ref_b, "after the refusal")
    # an EAGER candidate stage owns its vectors: a forward in between is fine
    eng.forward_net(xb)
    eng.candidates(B, lazy_flame=False)
    eng.forward_net(xa, use_graph=use_graph)
    det = eng.select(B, confidence_threshold=conf)
    _settle(eng)
    _same(_snap(det, with_heads=False), ref_b, "eager candidates, forward, select")
    # detect() through the graph keeps working (replay, lazy decode, select: one generation)
    _same(_snap(eng.detect(xb, confidence_threshold=conf, use_graph=use_graph), with_heads=False), ref_b, "detect")
    eng.close()


def test_overlap_mode_refuses_a_lazy_select_queued_behind_the_next_forward(gpu_lib):
    """Overlap mode: forward N + 1 queued before the lazy select N -- the guard event of select N would be recorded after that forward was let through -- is refused; the
    orderings test_overlap_mode_is_race_free_and_identical uses (select N before forward N + 1; eager candidates with the select anywhere) keep working."""
    from head_detector_amd._lib import VghError

    S, B = 256, 2
    xa, xb = _images(B, S, 51), _images(B, S, 52)
    eng = _engine(S, B)
    conf = float(eng.model(xa)[1][:, 20, 0].max())
    ref_a = _snap(eng.detect(xa, confidence_threshold=conf), with_heads=False)
    ref_b = _snap(eng.detect(xb, confidence_threshold=conf), with_heads=False)
    assert int(ref_a["counts"].sum()) > 0 and not torch.equal(ref_a["boxes"], ref_b["boxes"])
    eng.set_overlap(True)
    eng.forward_net(xa)
    eng.candidates(B, lazy_flame=True)
    eng.forward_net(xb)
    _sentinel(eng)
    with pytest.raises(VghError, match="forward"):
        eng.select(B, confidence_threshold=conf)
    assert _untouched(eng)
    for lazy in (True, False, True):
        eng.forward_net(xa)
        eng.candidates(B, lazy_flame=lazy)
        da = eng.select(B, confidence_threshold=conf)
        eng.forward_net(xb)
        _settle(eng)
        _same(_snap(da, with_heads=False), ref_a, ("select before the next forward", lazy))
        eng.candidates(B, lazy_flame=lazy)
        db = eng.select(B, confidence_threshold=conf)
        _settle(eng)
        _same(_snap(db, with_heads=False), ref_b, ("next batch", lazy))
    eng.forward_net(xa)
    eng.candidates(B, lazy_flame=False)
    eng.forward_net(xb)
    da = eng.select(B, confidence_threshold=conf)  # eager candidates: their select may follow the next forward
    _settle(eng)
    _same(_snap(da, with_heads=False), ref_a, "eager select behind the next forward")
    _same(_snap(eng.detect(xb, confidence_threshold=conf), with_heads=False), ref_b, "detect in overlap mode")
    eng.set_overlap(False)
    eng.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_an_abandoned_lazy_batch_is_not_an_error(gpu_lib, overlap):
    """A lazy batch that is never selected, then a normal detect(): it works."""
    S, B = 256, 2
    xa, xb = _images(B, S, 61), _images(B, S, 62)
    eng = _engine(S, B)
    conf = float(eng.model(xb)[1][:, 20, 0].max())
    ref_b = _snap(eng.detect(xb, confidence_threshold=conf), with_heads=False)
    eng.set_overlap(overlap)
    for _ in range(2):
        eng.forward_candidates(xa, lazy_flame=True)  # abandoned
        _same(_snap(eng.detect(xb, confidence_threshold=conf), with_heads=False), ref_b, "detect after an abandoned lazy batch")
    eng.set_overlap(False)
    eng.close()
