"""CPU: the planted select cases (tests/select_fixture.py) do what their names claim.  Every property is read from the ORACLE's outputs on the planted
tensors (ndfl_decode -> decoding_topk -> nms_torchvision / postprocess_batched), never from a kernel: this is the check of the inputs that
tests/test_gpu_select_contract.py then feeds to nms_select_kernel and the lazy gather."""
import numpy as np
import pytest
import torch

import select_fixture as sf
from head_detector_amd import arch

# (image size, keep_k): an anchor count below 1000 (pre_k = A = 525) and one above (1344, pre_k = 1000); keep_k 1, the default 100, and pre_k
CONFIGS = [(160, 1), (160, 100), (160, 525), (256, 1), (256, 100), (256, 1000)]
_GEO = {}


def _geo(S):
    if S not in _GEO:
        _GEO[S] = sf.geometry_of(arch.build_program("vgg_heads_m", arch.random_state_dict("vgg_heads_m", 0), S))
    return _GEO[S]


_SETS = {}


def _set(S, keep_k):
    if (S, keep_k) not in _SETS:
        geo = _geo(S)
        cs = sf.build_case_set(geo, min(1000, geo.A), keep_k)
        _SETS[(S, keep_k)] = (cs,) + sf.oracle_view(cs)
    return _SETS[(S, keep_k)]


def _kept_anchors(cs, cand, b, iou=sf.IOU):
    """(ranks NMS keeps before the cut, their anchor ids) of image b."""
    bb, ss, _, idx = cand
    keep = sf.oracle_keep(bb[b], ss[b], sf.CONF, iou)
    return keep, idx[b][torch.from_numpy(keep)].tolist()


def test_geometries_are_the_ones_the_issue_asks_for():
    assert _geo(160).A == 525 < 1000 < _geo(256).A == 1344
    for S in (160, 256):
        assert [lv["stride"] for lv in _geo(S).levels] == [8, 16, 32] and _geo(S).levels[0]["pitch"] >= 72 + _geo(S).shape_c + _geo(S).expr_c + 13


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_decoded_boxes_are_whole_bins_and_scores_are_separated(S, keep_k):
    """The decode is exact on the planted logits: every box edge is an odd multiple of half its level's stride (exactly, in fp32), scores that are meant to differ
    differ by far more than the 2e-6 the kernel's sigmoid may be off, and the candidates come out sorted."""
    cs, (rb, rs, rf), (bb, ss, ff, idx) = _set(S, keep_k)
    geo = cs.geo
    for l, lv in enumerate(geo.levels):
        e = rb[:, geo.starts[l] : geo.starts[l + 1]].double() / (lv["stride"] / 2)
        assert torch.equal(e, e.round()) and bool((e.long() % 2 == 1).all()), l
    s = ss[..., 0]
    assert bool((s[:, :-1] >= s[:, 1:]).all())
    d = (s[:, :-1] - s[:, 1:])
    rel = d / s[:, :-1]
    assert bool(((d == 0) | (rel > 1e-4)).all()), float(rel[d > 0].min())  # a tie, or more than 800 fp32 ulps (1.2e-7 relative each)
    assert float(rf[..., geo.shape_c:300].abs().max()) == 0.0 and float(rf[..., 300 + geo.expr_c : 400].abs().max()) == 0.0


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_empty(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    b = cs.case("empty").image
    assert float(cand[1][b].max()) < sf.CONF
    assert sf.oracle_select(cs, *cand[:3])[b][0].shape[0] == 0


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_all_valid(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    b = cs.case("all_valid").image
    assert float(cand[1][b].min()) >= sf.CONF  # every one of the pre_k candidates is valid
    keep, _ = _kept_anchors(cs, cand, b)
    assert len(keep) == cs.pre_k  # nothing suppresses anything ...
    boxes = cand[0][b].numpy()
    worst = max(float(sf.iou_f32(boxes[i], boxes[j])) for i in range(0, cs.pre_k, 7) for j in range(i + 1, min(cs.pre_k, i + 40)))
    assert worst <= 0.25  # ... (a sample of the pairs: tiles overlap by at most a quarter)
    out = sf.oracle_select(cs, *cand[:3])[b]
    assert out[0].shape[0] == keep_k and torch.equal(out[1], cand[1][b, :keep_k, 0])  # the keep_k cut is what bites


@pytest.mark.parametrize("S,keep_k", CONFIGS)
@pytest.mark.parametrize("name,extra", [("exact_keep_k", 0), ("keep_k_plus_1", 1)])
def test_cases_around_keep_k(S, keep_k, name, extra):
    cs, _, cand = _set(S, keep_k)
    c = cs.case(name)
    keep, anchors = _kept_anchors(cs, cand, c.image)
    want = min(keep_k + extra, cs.pre_k)  # (keep_k == pre_k: there cannot be more survivors than candidates)
    assert len(keep) == want and sorted(anchors) == c.note["survivors"]
    n_valid = int((cand[1][c.image, :, 0] >= sf.CONF).sum())
    assert n_valid == want + len(c.note["duplicates"]) and (len(c.note["duplicates"]) > 0 or want == cs.pre_k)  # NMS had duplicates to remove
    out = sf.oracle_select(cs, *cand[:3])[c.image]
    assert out[0].shape[0] == min(want, keep_k)
    if extra and want > keep_k:
        assert float(out[1].min()) > float(cand[1][c.image, keep[-1], 0])  # the lowest survivor fell to the cut


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_ties(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("ties")
    geo = cs.geo
    bb, ss, _, idx = cand
    keep, anchors = _kept_anchors(cs, cand, c.image)
    rank = {int(a): r for r, a in enumerate(idx[c.image].tolist())}
    groups = c.note["groups"]
    assert len(groups) >= 2 + (geo.levels[2]["h"] >= 4)
    for g in groups:
        assert len(g) >= 3 and len({geo.locate(a)[0] for a in g}) == 2  # at least three members, on both sides of a level boundary
        assert len({float(ss[c.image, rank[a], 0]) for a in g}) == 1    # one score
        assert [rank[a] for a in g] == list(range(rank[g[0]], rank[g[0]] + len(g))) and g == sorted(g)  # the oracle ranks them by ascending anchor index
        for i in g:
            for j in g:
                if i != j:
                    assert sf.iou_f32(bb[c.image, rank[i]].numpy(), bb[c.image, rank[j]].numpy()) > np.float32(sf.IOU)
        assert g[0] in anchors and not any(a in anchors for a in g[1:])  # the lowest anchor index survives, alone
        assert not torch.equal(cand[2][c.image, rank[g[0]]], cand[2][c.image, rank[g[-1]]])  # (another member would be another row)
    assert len(keep) == len(groups)


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_iou_exact(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("iou_exact")
    bb, _, _, idx = cand
    rank = {int(a): r for r, a in enumerate(idx[c.image].tolist())}
    pairs = c.note["pairs"]
    iou = {k: sf.iou_f32(bb[c.image, rank[hi]].numpy(), bb[c.image, rank[lo]].numpy()) for k, (hi, lo) in pairs.items()}
    thr, alt = np.float32(sf.IOU), np.float32(sf.IOU_ALT)
    assert iou["exact"].tobytes() == thr.tobytes()  # bit for bit
    assert iou["alt"].tobytes() == alt.tobytes() and float(alt) != 0.45  # 9 / 20 rounds, and rounds to the float the threshold rounds to
    assert thr < iou["above"] < thr + np.float32(1e-3) and thr - np.float32(2e-3) < iou["below"] < thr
    _, anchors = _kept_anchors(cs, cand, c.image)
    gone = [k for k, (hi, lo) in pairs.items() if lo not in anchors]
    assert gone == ["above"] and all(hi in anchors for hi, _ in pairs.values())  # at 0.5: exactly at the threshold is kept (strict >), just above goes
    _, anchors = _kept_anchors(cs, cand, c.image, iou=sf.IOU_ALT)
    assert sorted(k for k, (hi, lo) in pairs.items() if lo not in anchors) == ["above", "below", "exact"]  # at 0.45 only the 9 / 20 pair stays whole


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_degenerate(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("degenerate")
    bb, ss, _, idx = cand
    n = c.note
    rank = {int(a): r for r, a in enumerate(idx[c.image].tolist())}
    assert [rank[a] for a in (*n["points"], n["container"], n["zero_width"], n["tile"], n["tile_dup"])] == [0, 1, 2, 3, 4, 5]
    assert tuple(r for r, _ in c.box_patch) == n["inverted_ranks"] == (6, 7, 8) and int((ss[c.image, :, 0] >= sf.CONF).sum()) == 9
    b = bb[c.image].numpy()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert area[0] == 0 and area[1] == 0 and area[3] == 0 and b[3, 3] > b[3, 1]  # two points, a zero-width line
    assert b[6, 2] < b[6, 0] and area[6] < 0 and (b[6] == b[7]).all()           # an x-inverted box, twice
    assert b[8, 2] < b[8, 0] and b[8, 3] < b[8, 1] and area[8] > 0              # inverted both ways: a positive "area"
    assert np.isnan(sf.iou_f32(b[0], b[1]))                                      # 0 / 0
    assert sf.iou_f32(b[6], b[7]) == 0 and np.signbit(sf.iou_f32(b[6], b[7]))    # 0 / negative
    assert sf.iou_f32(b[4], b[5]) == 1
    keep, _ = _kept_anchors(cs, cand, c.image)
    assert keep.tolist() == [0, 1, 2, 3, 4, 6, 7, 8]  # NaN and -0 are not > threshold: kept; only the proper duplicate goes


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_conf_equal(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("conf_equal")
    _, ss, _, idx = cand
    rank = {int(a): r for r, a in enumerate(idx[c.image].tolist())}
    assert float(ss[c.image, rank[c.note["at_conf"]], 0]) == sf.CONF and rank[c.note["at_conf"]] == 2 and rank[c.note["below"]] == 3
    assert 0.499 < float(ss[c.image, 3, 0]) < sf.CONF
    keep, anchors = _kept_anchors(cs, cand, c.image)
    assert len(keep) == 3 and c.note["at_conf"] in anchors and c.note["below"] not in anchors  # >=
    out = sf.oracle_select(cs, *cand[:3])[c.image]
    assert out[0].shape[0] == min(3, keep_k) and (keep_k < 3 or float(out[1][-1]) == sf.CONF)


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_level_edges(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("level_edges")
    s = cs.geo.starts
    assert c.note["edges"] == [s[0], s[1] - 1, s[1], s[2] - 1, s[2], s[3] - 1]
    _, anchors = _kept_anchors(cs, cand, c.image)
    assert sorted(anchors) == c.note["edges"]  # the first and the last anchor of every level survive, nothing else is valid


@pytest.mark.parametrize("S,keep_k", CONFIGS)
def test_case_ballot_words(S, keep_k):
    cs, _, cand = _set(S, keep_k)
    c = cs.case("ballot_words")
    bb, ss, _, idx = cand
    n = c.note
    b = bb[c.image].numpy()
    assert float(ss[c.image].min()) >= sf.CONF  # all pre_k candidates valid: the last rank is reachable
    ranks = idx[c.image].tolist()
    last = cs.pre_k - 1
    assert [ranks[r] for r in (63, 64, 65, 127, 128, last)] == [n["rank63"], n["rank64"], n["rank65"], n["rank127"], n["rank128"], n["rank_last"]]
    keep, _ = _kept_anchors(cs, cand, c.image)
    kept = set(keep.tolist())
    thr = np.float32(sf.IOU)
    assert 63 in kept and 64 not in kept and 65 in kept and 127 in kept and 128 not in kept and last in kept
    # 64 falls to 63 and to nobody before it (the suppression crosses the word boundary); 65 overlaps 64 above the threshold and survives only because 64 is gone
    assert sf.iou_f32(b[63], b[64]) > thr and all(not sf.iou_f32(b[k], b[64]) > thr for k in kept if k < 63)
    assert sf.iou_f32(b[64], b[65]) > thr and all(not sf.iou_f32(b[k], b[65]) > thr for k in kept if k < 65)
    assert sf.iou_f32(b[127], b[128]) > thr and all(not sf.iou_f32(b[k], b[128]) > thr for k in kept if k < 127)
    assert len(kept) <= 100  # the last rank is inside the default keep_k
    assert set(idx[c.image][torch.from_numpy(keep)].tolist()) >= set(n["leaders"])
    out = sf.oracle_select(cs, *cand[:3])[c.image]
    if keep_k >= 100:
        assert torch.equal(out[0][-1], bb[c.image, last])


def test_random_set_for_many_images_has_empty_and_full_images():
    """The many-image set at the smallest image size (32 px: 21 anchors): counts from 0 up to the keep_k cut, so a head list over them is not trivial."""
    geo = sf.geometry_of(arch.build_program("vgg_heads_m", arch.random_state_dict("vgg_heads_m", 0), 32))
    assert geo.A == 21
    cs = sf.build_random_set(geo, 21, 8, 1100)
    _, cand = sf.oracle_view(cs)
    counts = [r[0].shape[0] for r in sf.oracle_select(cs, *cand[:3])]
    assert counts.count(0) > 100 and counts.count(8) > 100 and len(set(counts)) == 9
