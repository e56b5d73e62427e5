"""GPU (-m gpu): the deferred FLAME towers (csrc/tower_plan.h, the second mark of vgh_net_set_defer) and the survivor kernel that walks them (csrc/postproc.hip,
survivor_towers_kernel).

With the lazy FLAME gather on, a forward skips the 3x3 convs of the FLAME towers as well as the final 1x1 convs, and the select computes the survivors' prediction
rows from the (2 depth + 1)^2 window of the towers' root tensor (the pose channels of heads.headN.stems) around each survivor.  Everything here is torch.equal: the
kernel runs, per op, the summation chain of the tile the dense launch would have run on (conv_tiles.h, kChainTrait).  B = 3, keep_top_k = every anchor, threshold 0,
IoU 1: every anchor is a survivor, so every position of every map -- corners, edges, the 2 x 2 map whose windows leave the map on all four sides, interior anchors
of the 12 x 12 map with a full 7 x 7 window -- is compared.  The FLAME channels of the prediction rows AND the tower tensors (f0, f1, f2) are poisoned with NaN
first: what a deferred detect returns cannot have come from them, and they still hold the poison afterwards.

L has three 3x3 layers per level (21 tower ops, 7 x 7 windows), M has two (12 tower ops, 5 x 5 windows)."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

FO = 72  # VGH_PRED_FLAME_OFF
B = 3
NAN16 = 0x7FC0  # bf16 NaN


def _anchors(S):
    return (S // 8) ** 2 + (S // 16) ** 2 + (S // 32) ** 2


_engines = {}


def _dev():
    return torch.device("cuda", 0)


def _images(S, seed=7):
    return torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(_dev())


@pytest.fixture(scope="module")
def engines(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine, _alias

    def get(variant, S):
        if (variant, S) not in _engines:
            eng = VGHeadsEngine(variant, image_size=S, max_batch=B, seed=5, keep_top_k=_anchors(S), latency_lanes=False)
            P = eng.program
            # writable views, taken ONCE while nothing is pending (vgh_net_buffer runs pending convs): the prediction rows and the tower tensors
            eng.pred_views = [_alias(eng.lib.vgh_net_buffer(eng._net, lv["buf"]), (B, lv["h"] * lv["w"], lv["pitch"]), "<f4", eng.device) for lv in P.levels]
            eng.tower_bufs = [i for i, bf in enumerate(P.bufs) if re.fullmatch(r"heads\.head\d\.f\d", bf["name"])]
            eng.tower_views = [_alias(eng.lib.vgh_net_buffer(eng._net, i), (B, P.bufs[i]["h"] * P.bufs[i]["w"], P.bufs[i]["pitch"]), "<i2", eng.device) for i in eng.tower_bufs]
            eng.tower_ops = [i for i, op in enumerate(P.ops) if op["kind"] == 1 and op["ksize"] == 3 and op["out_buf"] in eng.tower_bufs]
            assert len(eng.tower_ops) == {"vgg_heads_l": 21, "vgg_heads_m": 12}[variant]  # (the program the cases below assume; the plan's marks: tests/tower_plan_host.hip)
            _engines[variant, S] = eng
        eng = _engines[variant, S]
        eng.join()
        eng.set_overlap(False)
        eng.set_split(1)
        eng.set_defer(True)
        eng._set_lazy_flame(False)
        return eng

    yield get
    for eng in _engines.values():
        eng.close()
    _engines.clear()


@pytest.fixture(scope="module")
def flame(flame_model):
    from head_detector_amd.flame import FLAMELayer

    return FLAMELayer(model=flame_model, device=_dev(), max_heads=B * _anchors(160))


def _settle(eng):
    eng.join()
    torch.cuda.synchronize()


def _poison(eng):
    _settle(eng)
    W = eng.program.shape_c + eng.program.expr_c + 13
    for v in eng.pred_views:
        v[:, :, FO:FO + W].fill_(float("nan"))
    for v in eng.tower_views:
        v.fill_(NAN16)
    _settle(eng)


def _all_or_none(flags, what):
    assert len(set(flags)) == 1, (what, flags)
    return flags[0]


def _flame_rows_nan(eng):
    _settle(eng)
    W = eng.program.shape_c + eng.program.expr_c + 13
    nan = [bool(torch.isnan(v[:, :, FO:FO + W]).all()) for v in eng.pred_views]
    some = [bool(torch.isnan(v[:, :, FO:FO + W]).any()) for v in eng.pred_views]
    assert nan == some
    return _all_or_none(nan, "prediction rows")


def _towers_poisoned(eng):
    """True: every tower tensor still holds the poison everywhere (no tower op has run); False: none of them holds any."""
    _settle(eng)
    full = [bool((v == NAN16).all()) for v in eng.tower_views]
    # a dense tower writes every channel of its tensor (ReLU outputs: never the NaN pattern)
    some = [bool((v == NAN16).any()) for v in eng.tower_views]
    assert full == some, (full, some)
    return _all_or_none(full, "tower tensors")


def _snap(det):
    return {k: getattr(det, k).clone() for k in ("boxes", "scores", "flame_params", "counts", "vertices_3d", "head_pose", "head_image")}


def _same(a, b, where):
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k)


def _detect(eng, x, flame, conf, iou=1.0, **kw):
    det = eng.detect(x, confidence_threshold=conf, iou_threshold=iou, flame=flame, **kw)
    _settle(eng)
    return _snap(det)


def _family(tile):
    """Kernel family of a tile name: the letter in front of its geometry, implicit GEMM without one."""
    return tile[0] if tile[0].isalpha() else "igemm"


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("variant,S", [("vgg_heads_l", 64), ("vgg_heads_l", 96), ("vgg_heads_m", 64), ("vgg_heads_m", 96)])
def test_every_position_of_every_map(engines, flame, variant, S, split):
    eng = engines(variant, S)
    assert eng.pre_k == eng.A == _anchors(S)
    x = _images(S)
    eng.set_split(split)
    out = {}
    for allow in (False, True):
        eng.set_defer(allow)
        _poison(eng)
        out[allow] = _detect(eng, x, flame, 0.0)
        assert _flame_rows_nan(eng) == allow
        assert _towers_poisoned(eng) == allow  # the forward skipped the towers (or not) and the select did not need them
    assert out[True]["counts"].tolist() == [_anchors(S)] * B  # every anchor of every level survived
    _same(out[True], out[False], "every anchor")
    # a graph replay skips what its capture skipped, and an eager buffer read completes the towers first
    if split == 1:
        eng.set_defer(True)
        _poison(eng)
        _same(_detect(eng, x, flame, 0.0, use_graph=True), out[False], "graph replay")
        assert _towers_poisoned(eng)
        eng.set_defer(False)
        eng.forward_net(x)
        dense = [eng.buffer(b, B) for b in eng.tower_bufs]
        eng.set_defer(True)
        _poison(eng)
        eng._set_lazy_flame(True)
        eng.forward_net(x)
        assert _towers_poisoned(eng)
        got = [eng.buffer(b, B) for b in eng.tower_bufs[-1:]]  # the LAST tensor of a tree: every pending op in front of it runs first
        assert torch.equal(got[0], dense[-1]) and not _towers_poisoned(eng)
        assert all(torch.equal(eng.buffer(b, B), d) for b, d in zip(eng.tower_bufs, dense))


# the tiles the benchmark's table (tuning/conv_cfg.json, b64x2 keys) names for the tower shapes: every one of these families has to be walked at least once
BENCH_FAMILIES = {"g", "s", "q", "p", "igemm"}
CHAIN_CONFIGS = [("vgg_heads_l", 64), ("vgg_heads_m", 96), ("vgg_heads_l", 160)]  # 160: maps of 20^2 / 10^2 / 5^2, which admit the s tiles


def _walk_every_tile(eng, flame, S, seen):
    P, x = eng.program, _images(S, 23)
    names = eng.cfg_names()
    ops = eng.tower_ops
    try:
        for c, name in enumerate(names):
            on = [i for i in ops if eng.cfg_ok(c, P.ops[i])]
            if not on:
                continue
            for i in ops:
                eng.set_cfg(i, c if i in on else -1)
            tiles = eng.op_tiles()
            forced = [i for i in on if tiles[i] == name]  # (a tile that cannot run the op at this map size is replaced by the automatic one)
            if not forced:
                continue
            fams = {_family(tiles[i]) for i in ops}
            out = {}
            for allow in (False, True):
                eng.set_defer(allow)
                _poison(eng)
                out[allow] = _detect(eng, x, flame, 0.0)
            skipped = _towers_poisoned(eng)
            assert _flame_rows_nan(eng)
            _same(out[True], out[False], name)
            if skipped:
                seen["sparse"] |= fams
            else:
                seen["dense"].add(_family(name))
    finally:
        for i in ops:
            eng.set_cfg(i, -1)
        eng.set_defer(True)


def test_every_chain(engines, flame):
    """The tower ops forced onto every tile of the table that admits them, on all of CHAIN_CONFIGS: detections with and without deferral are equal, tile by tile.  A
    tile of a family whose chain the kernel reproduces leaves the tower tensors untouched; any other family makes the forward run its towers densely -- never an
    approximation.  Every family the benchmark's table names for the tower shapes is walked at least once, and none of them runs densely."""
    seen = {"sparse": set(), "dense": set()}
    for variant, S in CHAIN_CONFIGS:
        _walk_every_tile(engines(variant, S), flame, S, seen)
    assert BENCH_FAMILIES <= seen["sparse"], seen
    assert not (seen["dense"] & BENCH_FAMILIES), seen


@pytest.mark.parametrize("variant,S", [("vgg_heads_l", 96), ("vgg_heads_m", 64)])
def test_ragged_counts(engines, variant, S):
    """Planted survivors: disjoint boxes, scores that put exactly n rows of image 0 above the threshold (n = 0, 1, 31, 32, 33 and the capacity; seven fewer per image
    behind it), a random anchor behind every candidate row.  The rows equal the dense ones; rows at and past the count are zero."""
    eng = engines(variant, S)
    x, k = _images(S, 11), eng.pre_k
    KEEP = eng.keep_k
    assert KEEP == k == _anchors(S)
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.randperm(eng.A, generator=g) for _ in range(B)]).to(torch.int32).to(eng.device)
    j = torch.arange(k, dtype=torch.float32)
    boxes = torch.stack([16 * j, 0 * j, 16 * j + 8, 0 * j + 8], dim=1).expand(B, k, 4).contiguous().to(eng.device)
    scores = torch.stack([1.0 - (j + 7 * b) / 1024 for b in range(B)]).to(eng.device)

    def count(n, b):
        return max(0, min(KEEP, n - 7 * b))

    eng._set_lazy_flame(True)
    _poison(eng)
    eng.forward_net(x)
    eng.candidates(B, lazy_flame=True)
    _settle(eng)
    eng.idx[:B].copy_(idx)
    eng.cand_boxes[:B].copy_(boxes)
    eng.cand_scores[:B].copy_(scores)
    got = {}
    for n in (0, 1, 31, 32, 33, KEEP):
        det = eng.select(B, confidence_threshold=2.0 if n == 0 else 1.0 - (n - 1) / 1024, iou_threshold=0.5)
        _settle(eng)
        assert det.counts.tolist() == [count(n, b) for b in range(B)], n
        got[n] = det.flame_params.clone()
    assert _flame_rows_nan(eng) and _towers_poisoned(eng)  # nothing ran the convs
    # dense rows: an eager candidate stage behind that forward runs every pending op
    eng.candidates(B, lazy_flame=False)
    _settle(eng)
    assert not _flame_rows_nan(eng) and not _towers_poisoned(eng)
    inv = torch.argsort(eng.idx[:B].long(), dim=1)
    rows = torch.gather(inv, 1, idx.long())
    ref = torch.gather(eng.cand_flame[:B], 1, rows[:, :, None].expand(B, k, eng.cand_flame.shape[2]))[:, :KEEP].clone()
    assert not bool(torch.isnan(ref).any())
    for n, r in got.items():
        for b in range(B):
            c = count(n, b)
            assert torch.equal(r[b, :c], ref[b, :c]), (n, b)
            assert not bool(r[b, c:].any()), (n, b)


def test_overlap_race(engines, flame):
    """Overlap mode, two lanes: forwards and selects interleaved as the benchmark's step does, the select of batch i on the side stream under the forward of batch
    i + 1 -- which has other images, so a forward that rewrote the towers' root before the select had read it would change that batch's detections.  Then the same
    with the switch turned off between two steps: the forward behind a deferring one runs its towers, and still may not write the root early.
    A smoke test of the interleaving, not a proof of the ordering: at these sizes the root's writer of forward i + 1 is queued behind a whole backbone and neck, long
    after the small select i has finished, so a misplaced wait would rarely show here.  The deterministic part -- which ops carry the root-writer flag -- is held by
    tests/tower_plan_host.hip; where the executor waits is writes_guarded in csrc/net.hip."""
    S = 96
    eng = engines("vgg_heads_l", S)
    xs = [_images(S, 31), _images(S, 37)]
    eng.set_defer(True)
    eng.set_split(2)
    ref = [_detect(eng, x, flame, 0.0) for x in xs]  # serial: the select on the caller's stream
    assert not torch.equal(ref[0]["flame_params"], ref[1]["flame_params"])
    eng.set_overlap(True)
    dets = []
    slots = [eng.new_output_slot(flame, B) for _ in range(24)]  # a private set of result buffers per step: nothing below has to wait for a copy
    _poison(eng)
    for i in range(20):
        eng.forward_net(xs[i % 2])
        eng.candidates(B, lazy_flame=True)
        dets.append(eng.select(B, confidence_threshold=0.0, iou_threshold=1.0, flame=flame, slot=slots[i]))
    _settle(eng)
    assert _towers_poisoned(eng)
    for i, det in enumerate(dets):
        _same(_snap(det), ref[i % 2], ("step", i))
    # deferring, dense, deferring, dense: no join in between
    dets = []
    for i in range(4):
        eng.set_defer(i % 2 == 0)
        eng.forward_net(xs[i % 2])
        eng.candidates(B, lazy_flame=True)
        dets.append(eng.select(B, confidence_threshold=0.0, iou_threshold=1.0, flame=flame, slot=slots[20 + i]))
    _settle(eng)
    assert not _towers_poisoned(eng)
    for i, det in enumerate(dets):
        _same(_snap(det), ref[i % 2], ("switched step", i))
    eng.set_defer(True)
    eng.set_overlap(False)
    eng.set_split(1)
