"""GPU (-m gpu): the deferred FLAME prediction convs (include/vgh.h, vgh_detector_set_lazy_flame) and the survivor-row kernel of csrc/postproc.hip.

With the lazy FLAME gather on, forwards skip the final 1x1 convs of the FLAME towers and the select computes the survivors' rows from the convs' inputs.  Everything
here is torch.equal: a 1x1 conv is pointwise, the kernel runs the implicit-GEMM tiles' MFMA chain (same instruction, k-blocks ascending, bias added in fp32
afterwards), so a row computed alone is the row of the dense op bit for bit -- for every tile of the table that can run those ops, which differ in staging and store
pattern, not in that chain.  L and M at 64 and 96 px: 84 and 189 anchors (top-k clamps to the anchor count), all three levels, B = 3, u8 input."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FO = 72  # VGH_PRED_FLAME_OFF
B = 3


def _anchors(S):  # keep_top_k = every anchor: with a threshold of 0 and no suppression all of them survive, the 4 / 9 of the coarsest level included
    return (S // 8) ** 2 + (S // 16) ** 2 + (S // 32) ** 2  # 84 = 2 x 32 + 20 and 189 = 5 x 32 + 29: whole and ragged 32-row groups of the survivor kernel


CONFIGS = [("vgg_heads_l", 64), ("vgg_heads_l", 96), ("vgg_heads_m", 64), ("vgg_heads_m", 96)]
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
            # writable views of the level prediction buffers, f32 [B, h * w, pitch], taken ONCE while nothing is pending (vgh_net_buffer runs pending convs)
            eng.pred_views = [_alias(eng.lib.vgh_net_buffer(eng._net, lv["buf"]), (B, lv["h"] * lv["w"], lv["pitch"]), "<f4", eng.device) for lv in eng.program.levels]
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

    return FLAMELayer(model=flame_model, device=_dev(), max_heads=B * _anchors(96))


def _settle(eng):
    eng.join()
    torch.cuda.synchronize()


def _poison(eng):
    """NaN into the FLAME channels of the dense prediction rows: a deferring forward does not write them, a lazy select behind it does not read them."""
    _settle(eng)
    W = eng.program.shape_c + eng.program.expr_c + 13  # (the pitch may round up behind them: channels no op writes, zero since the arena was created)
    for v in eng.pred_views:
        v[:, :, FO:FO + W].fill_(float("nan"))
    _settle(eng)


def _flame_rows_nan(eng):
    """True: every FLAME channel still holds the poison (the nine convs have not run); False: none does; anything in between is an error."""
    _settle(eng)
    W = eng.program.shape_c + eng.program.expr_c + 13
    nan = [bool(torch.isnan(v[:, :, FO:FO + W]).all()) for v in eng.pred_views]
    some = [bool(torch.isnan(v[:, :, FO:FO + W]).any()) for v in eng.pred_views]
    assert nan == some and len(set(nan)) == 1, (nan, some)
    return nan[0]


def _snap(det):
    return {k: getattr(det, k).clone() for k in ("boxes", "scores", "flame_params", "counts", "vertices_3d", "head_pose", "head_image")}


def _same(a, b, where):
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k)


def _detect(eng, x, flame, conf, iou=1.0, **kw):
    det = eng.detect(x, confidence_threshold=conf, iou_threshold=iou, flame=flame, **kw)
    _settle(eng)
    return _snap(det)


def _starts(eng):
    starts, at = [], 0
    for lv in eng.program.levels:
        starts.append(at)
        at += lv["h"] * lv["w"]
    return starts


def _survivor_levels(eng, counts):
    """Levels of the anchors the last select kept (through the top-k index rows and the keep positions it left in the detector's scratch)."""
    starts = _starts(eng)
    seen = set()
    idx, keep = eng.idx[:B].cpu(), eng.keep_idx[:B].cpu()
    for b in range(B):
        for j in range(int(counts[b])):
            a = int(idx[b, int(keep[b, j])])
            seen.add(max(l for l, s in enumerate(starts) if a >= s))
    return seen


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("variant,S", CONFIGS)
def test_detect_is_the_same_with_and_without_deferral(engines, flame, variant, S, split, overlap):
    eng = engines(variant, S)
    assert eng.pre_k == eng.A == sum(lv["h"] * lv["w"] for lv in eng.program.levels)
    x = _images(S)
    eng.set_split(split)
    eng.set_overlap(overlap)
    out = {}
    for allow in (False, True):
        eng.set_defer(allow)
        _poison(eng)
        out[allow, "many"] = _detect(eng, x, flame, 0.0)
        assert _flame_rows_nan(eng) == allow  # the forward skipped the nine convs (or not) and the lazy select did not need them
        if allow:
            levels = _survivor_levels(eng, out[allow, "many"]["counts"].tolist())
        out[allow, "none"] = _detect(eng, x, flame, 2.0)
    total = int(out[True, "many"]["counts"].sum())
    assert total >= 20 and levels == {0, 1, 2}, (total, levels)
    assert int(out[True, "none"]["counts"].sum()) == 0
    _same(out[True, "many"], out[False, "many"], "survivors on every level")
    _same(out[True, "none"], out[False, "none"], "no survivors")


@pytest.mark.parametrize("variant,S", CONFIGS)
def test_survivor_rows_equal_the_dense_rows_for_every_tile(engines, variant, S):
    """The survivor-row kernel on PLANTED survivors -- disjoint boxes, scores that put exactly n rows of image 0 above the threshold (n = 0, 1, 31, 32, 33 and the
    capacity; seven fewer per image behind it), a random anchor behind every candidate row -- against the dense rows, with the nine convs forced onto every tile of the
    table that can run them.  Both sides hand the rows to the same fix-up (flame_channel), so equal vectors are equal rows up to what the fix-up keeps of them: the
    13 transform channels pass through as they are (translation and scale in a strictly monotone form), shape and expression through tanh."""
    eng = engines(variant, S)
    P, x, k = eng.program, _images(S, 11), eng.pre_k
    KEEP = eng.keep_k
    assert KEEP == k == _anchors(S)
    ops = [i for i, op in enumerate(P.ops) if op["kind"] == 1 and op["ksize"] == 1 and P.bufs[op["out_buf"]]["is_f32"] == 1 and op["out_coff"] >= FO]
    assert len(ops) == 9
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.randperm(eng.A, generator=g) for _ in range(B)]).to(torch.int32).to(eng.device)  # every anchor once per image: all levels among the survivors
    j = torch.arange(k, dtype=torch.float32)
    boxes = torch.stack([16 * j, 0 * j, 16 * j + 8, 0 * j + 8], dim=1).expand(B, k, 4).contiguous().to(eng.device)
    scores = torch.stack([1.0 - (j + 7 * b) / 1024 for b in range(B)]).to(eng.device)  # exact in fp32, descending

    def count(n, b):
        return max(0, min(KEEP, n - 7 * b))

    # ---- the kernel's rows: from the towers' outputs of a DEFERRED forward, the dense FLAME channels poisoned ----
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
        assert torch.equal(eng.keep_idx[0, :count(n, 0)].cpu(), torch.arange(count(n, 0), dtype=torch.int32))
        got[n] = det.flame_params.clone()
    assert _flame_rows_nan(eng)  # nothing ran the convs: the vectors above cannot have come from dense rows

    # ---- dense rows: an eager candidate stage behind that forward (it runs the pending convs), then forwards that run the convs themselves on every tile ----
    def dense_vectors():
        eng.candidates(B, lazy_flame=False)
        _settle(eng)
        assert not _flame_rows_nan(eng)
        inv = torch.argsort(eng.idx[:B].long(), dim=1)  # pre_k = A: every anchor is a candidate; inv[b, a] = its candidate row
        rows = torch.gather(inv, 1, idx.long())
        return torch.gather(eng.cand_flame[:B], 1, rows[:, :, None].expand(B, k, eng.cand_flame.shape[2]))[:, :KEEP].clone()

    refs = {"pending convs run by the eager stage": dense_vectors()}
    names = eng.cfg_names()
    admitted = {c: [i for i in ops if eng.cfg_ok(c, P.ops[i])] for c in range(len(names))}  # (a tile takes the ops whose cout_pad its cout tile divides)
    admitted = {c: on for c, on in admitted.items() if on}
    assert len(admitted) >= 8 and all(any(i in on for on in admitted.values()) for i in ops), admitted
    for c, on in admitted.items():
        for i in ops:
            eng.set_cfg(i, c if i in on else -1)
        assert all(eng.op_tiles()[i] == names[c] for i in on)
        _poison(eng)
        eng.forward_net(x)
        refs[names[c]] = dense_vectors()
    for i in ops:
        eng.set_cfg(i, -1)
    for name, ref in refs.items():
        assert not bool(torch.isnan(ref).any()), name
        for n, rows in got.items():
            for b in range(B):
                c = count(n, b)
                assert torch.equal(rows[b, :c], ref[b, :c]), (name, n, b)
                assert not bool(rows[b, c:].any()), (name, n, b)  # zeros at and past the count


@pytest.mark.parametrize("variant,S", CONFIGS[:1] + CONFIGS[3:])
def test_eager_stages_run_the_pending_convs_first(engines, flame, variant, S):
    """A deferred forward followed by an eager candidate stage is legal and gives today's candidates; so do model() and a batch in arena chunks."""
    from head_detector_amd.engine import VGHeadsEngine

    eng = engines(variant, S)
    x = _images(S, 13)
    eng.set_defer(False)
    ref = [t.clone() for t in eng.model(x)]
    eng.set_defer(True)
    eng._set_lazy_flame(True)
    _poison(eng)
    eng.forward_net(x)
    assert _flame_rows_nan(eng)
    eng.cand_flame.fill_(float("nan"))
    eng.candidates(B, lazy_flame=False)
    assert not _flame_rows_nan(eng)
    assert torch.equal(eng.cand_flame[:B], ref[2]) and torch.equal(eng.cand_boxes[:B], ref[0]) and torch.equal(eng.cand_scores[:B].unsqueeze(-1), ref[1])
    eng._set_lazy_flame(True)
    eng.forward_net(x)  # left pending, then replaced by model()'s own forward
    got = eng.model(x)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # lazy candidates, an eager chunk behind them (at > 0 reads dense rows), then the lazy rows alone: the select reads the rows the eager stage completed
    many = _detect(eng, x, flame, 0.0)
    _poison(eng)
    eng.forward_net(x)
    eng.candidates(B - 1, lazy_flame=True)
    assert _flame_rows_nan(eng)
    eng.candidates(1, at=B - 1, lazy_flame=False)
    assert not _flame_rows_nan(eng)
    det = eng.select(B - 1, confidence_threshold=0.0, iou_threshold=1.0, flame=flame)
    _settle(eng)
    assert torch.equal(det.flame_params, many["flame_params"][:B - 1]) and torch.equal(det.counts, many["counts"][:B - 1])
    # B > arena_batch: chunks gather eagerly whatever the switch says
    small = VGHeadsEngine(variant, image_size=S, max_batch=B, seed=5, keep_top_k=eng.keep_k, latency_lanes=False, arena_batch=2)
    assert small.arena_batch == 2
    chunked = _detect(small, x, flame, 0.0)
    small.close()
    _same(chunked, many, "arena chunks")


@pytest.mark.parametrize("variant,S", CONFIGS[1:3])
def test_two_selects_then_a_stale_one_is_refused(engines, flame, variant, S):
    from head_detector_amd._lib import VghError

    eng = engines(variant, S)
    x = _images(S, 17)
    scores = eng.model(x)[1]
    conf = float(scores[:, eng.pre_k // 3, 0].max())
    ref = {}
    eng.set_defer(False)
    for c in (0.0, conf):
        ref[c] = _detect(eng, x, flame, c)
    assert int(ref[conf]["counts"].sum()) < int(ref[0.0]["counts"].sum())
    eng.set_defer(True)
    eng._set_lazy_flame(True)
    _poison(eng)
    eng.forward_net(x)
    eng.candidates(B, lazy_flame=True)
    for c in (0.0, conf, 0.0):
        det = eng.select(B, confidence_threshold=c, iou_threshold=1.0, flame=flame)
        _settle(eng)
        _same(_snap(det), ref[c], c)
    assert _flame_rows_nan(eng)
    eng.forward_net(x)
    with pytest.raises(VghError, match="forward"):
        eng.select(B, confidence_threshold=conf, iou_threshold=1.0, flame=flame)
    eng.candidates(B, lazy_flame=True)  # the engine recovers
    det = eng.select(B, confidence_threshold=conf, iou_threshold=1.0, flame=flame)
    _settle(eng)
    _same(_snap(det), ref[conf], "after the refusal")


@pytest.mark.parametrize("variant,S", CONFIGS[:1] + CONFIGS[3:])
def test_graph_replay_profile_and_buffers(engines, flame, variant, S):
    eng = engines(variant, S)
    x = _images(S, 19)
    levels = [lv["buf"] for lv in eng.program.levels]
    eng.set_defer(False)
    ref = _detect(eng, x, flame, 0.0)
    eng.forward_net(x)
    dense = [eng.buffer(b, B) for b in levels]
    eng.set_defer(True)
    # a replayed graph skips what its capture skipped
    for rnd in range(2):
        _poison(eng)
        _same(_detect(eng, x, flame, 0.0, use_graph=True), ref, ("graph", rnd))
        assert _flame_rows_nan(eng)
    _same(_detect(eng, x, flame, 0.0), ref, "eager launch")
    # dense buffers are handed out complete
    _poison(eng)
    eng.forward_net(x)
    assert _flame_rows_nan(eng)
    got = [eng.buffer(b, B) for b in levels]
    assert all(torch.equal(a, b) for a, b in zip(got, dense))
    # the profiler runs every op
    _poison(eng)
    eng.forward_net(x)
    assert _flame_rows_nan(eng)
    _poison(eng)
    prof = eng.profile_ops(x)
    assert len(prof) == len(eng.program.ops) and all(torch.equal(eng.buffer(b, B), d) for b, d in zip(levels, dense))
