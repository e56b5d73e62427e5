"""Planted candidate sets for the select stage (tests/test_select_cases_host.py on the CPU, tests/test_gpu_select_contract.py on the GPU).

Given the geometry of an engine's program (levels, pitches, strides, live shape / expression channels) ``build_case_set`` writes float32 prediction tensors
[B, h, w, pitch] per level -- what the network would leave in its fp32 prediction buffers -- that force a CHOSEN candidate set on the post-network stages:

* DFL logits with one dominant bin per side: DFL_HI for the bin, DFL_LO for the other sixteen.  exp(DFL_LO - DFL_HI) = exp(-200) is below half the smallest fp32
  subnormal (1.4e-45 = exp(-103.3)), so every other bin's exp is exactly 0 in fp32, the softmax is exactly one-hot, the decoded distance is the whole bin and the
  box is ((x + 0.5 -+ bins) * stride): half-integers times a power of two, exact in fp32 in the oracle and in the kernel alike.
* class logits chosen per anchor.  Distinct logits are more than 1e-4 apart in relative score (over 800 fp32 ulps: the kernel's and torch's sigmoid differ in
  the last ulps only, the top-k ORDER is the same); repeated logits give exact score ties (the same function of the same input on either side); logit 0 is score 0.5
  exactly on both sides (1 / (1 + 1)).
* random raw FLAME channels.

What a box can be: x1 = cx - l * stride, x2 = cx + r * stride with l, r in 0..16 and cx the anchor's centre, so a box always contains its anchor's centre (distances
are never negative: an INVERTED box cannot come out of the decode) and its edges sit at (k + 0.5) * stride.  Two anchors of one level can carry the identical box;
anchors of different levels cannot (edges = 4 mod 8, 8 mod 16, 16 mod 32).  Inverted boxes are therefore planted one stage later, by overwriting rows of the candidate
box tensor between the candidate stage and the select (``Case.box_patch``) -- the select reads its boxes from that tensor in the lazy and in the eager route.

``oracle_view`` is the oracle's reading of the same tensors: ndfl_decode over assemble_flame_channels (the assembly of test_head_decode_and_gather_vs_oracle), then
decoding_topk; ``oracle_select`` is postprocess_batched.  Every property a case is named for is asserted from those outputs in tests/test_select_cases_host.py."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from head_detector_amd.arch import PRED_CLS_OFF, PRED_FLAME_OFF
from oracle import postproc_oracle as po

DFL_HI, DFL_LO = 100.0, -100.0
BG_TOP = -4.0  # background logits lie in (BG_TOP - 3, BG_TOP]: scores below 0.018
CASE_NAMES = ("empty", "all_valid", "exact_keep_k", "keep_k_plus_1", "ties", "iou_exact", "degenerate", "conf_equal", "level_edges", "ballot_words")
CONF, IOU = 0.5, 0.5  # the thresholds the cases are built for (iou_exact also holds a pair for IOU_ALT)
IOU_ALT = 0.45        # 9 / 20: not a binary fraction -- the kernel's fp32 division has to round it to the very float the threshold rounds to


@dataclass
class Geometry:
    levels: List[dict]  # dict(h, w, pitch, stride) per level, level-major anchor order
    shape_c: int
    expr_c: int

    @property
    def starts(self) -> List[int]:
        s = [0]
        for lv in self.levels:
            s.append(s[-1] + lv["h"] * lv["w"])
        return s

    @property
    def A(self) -> int:
        return self.starts[-1]

    def anchor(self, level: int, x: int, y: int) -> int:
        lv = self.levels[level]
        assert 0 <= x < lv["w"] and 0 <= y < lv["h"], (level, x, y)
        return self.starts[level] + y * lv["w"] + x

    def locate(self, a: int) -> Tuple[int, int, int]:
        """anchor index -> (level, x, y)"""
        l = max(i for i in range(len(self.levels)) if a >= self.starts[i])
        p = a - self.starts[l]
        return l, p % self.levels[l]["w"], p // self.levels[l]["w"]

    def bins_for(self, a: int, box) -> Tuple[int, int, int, int]:
        """The (l, t, r, b) whole bins with which anchor ``a`` decodes to ``box`` (x1, y1, x2, y2 in pixels); asserts that the box is reachable from there."""
        l, x, y = self.locate(a)
        st = self.levels[l]["stride"]
        cx, cy = (x + 0.5) * st, (y + 0.5) * st
        d = [(cx - box[0]) / st, (cy - box[1]) / st, (box[2] - cx) / st, (box[3] - cy) / st]
        assert all(float(v).is_integer() and 0 <= v <= po.REG_MAX for v in d), (a, (l, x, y), box, d)
        return tuple(int(v) for v in d)

    def tile(self, a: int) -> Tuple[float, float, float, float]:
        """One stride wide, up and left of the anchor's centre (bins 1, 1, 0, 0).  The tiles of one level are disjoint; tiles of neighbouring levels overlap with
        IoU <= 1/4, two levels apart <= 1/16: no tile suppresses another at IOU."""
        l, x, y = self.locate(a)
        st = self.levels[l]["stride"]
        return ((x - 0.5) * st, (y - 0.5) * st, (x + 0.5) * st, (y + 0.5) * st)


def geometry_of(program) -> Geometry:
    """The part of an engine's program (head_detector_amd.arch.Program) the post-network stages see."""
    return Geometry([dict(h=lv["h"], w=lv["w"], pitch=lv["pitch"], stride=lv["stride"]) for lv in program.levels], program.shape_c, program.expr_c)


@dataclass
class Image:
    """One planted image: whole DFL bins and a class logit per anchor."""
    bins: np.ndarray   # [A, 4] int (l, t, r, b)
    logit: np.ndarray  # [A] float32


@dataclass
class Case:
    name: str
    image: int                                   # row of the case set's batch
    note: Dict[str, object] = field(default_factory=dict)  # what the host test checks (anchor ids, expected counts: INPUT facts, asserted against the oracle there)
    box_patch: List[Tuple[int, Tuple[float, float, float, float]]] = field(default_factory=list)  # (candidate rank, box) written over the candidate boxes before the select


@dataclass
class CaseSet:
    geo: Geometry
    pre_k: int
    keep_k: int
    preds: List[torch.Tensor]  # per level f32 [B, h, w, pitch]
    cases: List[Case]

    @property
    def B(self) -> int:
        return self.preds[0].shape[0]

    def case(self, name: str) -> Case:
        return next(c for c in self.cases if c.name == name)

    def patch_boxes(self, cand_boxes: torch.Tensor) -> None:
        """The planted candidate-box overrides (inverted boxes), in place, on a [B, pre_k, 4] candidate tensor of the oracle or of the engine."""
        for c in self.cases:
            for rank, box in c.box_patch:
                cand_boxes[c.image, rank] = torch.tensor(box, dtype=cand_boxes.dtype, device=cand_boxes.device)


def _background(geo: Geometry, rng: np.random.Generator) -> Image:
    """Every anchor a tile with a distinct logit below the threshold, in a seeded order."""
    A = geo.A
    bins = np.tile(np.array([1, 1, 0, 0]), (A, 1))
    logit = (BG_TOP - 3.0 * rng.permutation(A) / A).astype(np.float32)
    return Image(bins, logit)


def _descending(n: int, hi: float = 3.0, lo: float = 0.05) -> np.ndarray:
    """n distinct logits from hi down to lo whose SCORES are evenly spaced (all > 0.5): for the n <= 1344 used here neighbours are >= 1.6e-4 apart in score."""
    s = np.linspace(1.0 / (1.0 + np.exp(-hi)), 1.0 / (1.0 + np.exp(-lo)), n)
    return np.log(s / (1.0 - s)).astype(np.float32)


def _put(img: Image, geo: Geometry, a: int, box, logit: float) -> None:
    img.bins[a] = geo.bins_for(a, box)
    img.logit[a] = np.float32(logit)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------------
def _case_empty(geo, pre_k, keep_k, rng):
    return _background(geo, rng), {}


def _case_all_valid(geo, pre_k, keep_k, rng):
    """Every anchor a valid tile with its own score: the pre_k candidates are all >= CONF, nothing suppresses anything (tile IoU <= 1/4), the keep_k cut is all that bites."""
    img = _background(geo, rng)
    img.logit[rng.permutation(geo.A)] = _descending(geo.A)
    return img, {}


def _survivors(geo, pre_k, keep_k, rng, n_surv):
    """n_surv valid tiles that all survive, plus up to 16 lower-scored exact duplicates (the same tile decoded from the anchor to its left) that NMS removes."""
    img = _background(geo, rng)
    order = rng.permutation(geo.A)
    surv = order[:n_surv]
    img.logit[surv] = _descending(n_surv, 3.0, 1.0)
    taken = set(int(a) for a in surv)
    dups = []
    for a in surv:
        l, x, y = geo.locate(int(a))
        if x == 0 or len(dups) >= min(16, pre_k - n_surv):
            continue
        left = geo.anchor(l, x - 1, y)
        if left in taken:
            continue
        taken.add(left)
        _put(img, geo, left, geo.tile(int(a)), 0.9 - 0.02 * len(dups))
        dups.append(left)
    return img, dict(survivors=sorted(int(a) for a in surv), duplicates=dups)


def _case_exact_keep_k(geo, pre_k, keep_k, rng):
    return _survivors(geo, pre_k, keep_k, rng, keep_k)


def _case_keep_k_plus_1(geo, pre_k, keep_k, rng):
    """keep_k + 1 survivors before the cut -- or pre_k of them when keep_k == pre_k: more survivors than candidates cannot exist."""
    return _survivors(geo, pre_k, keep_k, rng, min(keep_k + 1, pre_k))


def _case_ties(geo, pre_k, keep_k, rng):
    """Groups of equal scores whose boxes overlap above IOU, with members on both sides of a level boundary: which member survives is decided by the tie rule alone
    (ascending anchor index = the lower level first).  Group g sits around pixel (64 g + 32, 32) for the level 0 | 1 boundary; one more group straddles level 1 | 2.
    Inside a group the boxes differ (levels cannot share a box), so the wrong survivor is a visibly different row."""
    img = _background(geo, rng)
    groups = []
    L = geo.levels
    n01 = max(1, min(3, L[0]["w"] * L[0]["stride"] // 64))
    for g in range(n01):  # two level-0 anchors with the box [12, 36]^2 + 64 g and one level-1 anchor with [8, 40]^2 + 64 g: IoU 576 / 1024 = 0.5625
        ox = 64 * g
        a0, a1 = geo.anchor(0, (ox + 16) // 8, 2), geo.anchor(0, (ox + 24) // 8, 3)
        b1 = geo.anchor(1, (ox + 16) // 16, 1)
        lg = 2.0 - 0.25 * g
        _put(img, geo, a0, (ox + 12, 12, ox + 36, 36), lg)
        _put(img, geo, a1, (ox + 12, 12, ox + 36, 36), lg)
        _put(img, geo, b1, (ox + 8, 8, ox + 40, 40), lg)
        groups.append([a0, a1, b1])
    if len(L) >= 3 and L[2]["h"] >= 4:  # level 1 | 2, around pixel (64, 96): level-1 [24, 104] x [72, 120] twice and level-2 [16, 112] x [80, 112]
        c0, c1 = geo.anchor(1, 2, 5), geo.anchor(1, 4, 6)
        d2 = geo.anchor(2, 1, 3)
        box1, box2 = (24, 72, 104, 120), (16, 80, 112, 112)  # inter 80 x 32 = 2560; union 3840 + 3072 - 2560 = 4352: IoU 0.588
        _put(img, geo, c0, box1, 1.0)
        _put(img, geo, c1, box1, 1.0)
        _put(img, geo, d2, box2, 1.0)
        groups.append([c0, c1, d2])
    return img, dict(groups=groups)


def _case_iou_exact(geo, pre_k, keep_k, rng):
    """Pairs on level 0, far from each other (units of the level's stride u = 8 px; the higher score first):
      exact  : 2u x 2u and the 2u x 1u half of it            IoU  2 /  4  = IOU exactly           -> both kept (strict >)
      above  : 32u x 32u and a 27u x 19u box inside it       IoU 513 / 1024 = 0.50098             -> the second suppressed
      below  : 32u x 32u and a 30u x 17u box inside it       IoU 510 / 1024 = 0.49805             -> both kept
      alt    : 4u x 5u and a 3u x 3u box inside it           IoU  9 / 20  = IOU_ALT after rounding -> both kept at IOU and at IOU_ALT
    The big pairs sit in opposite corners of the image and reach out of it (boxes are not clipped)."""
    img = _background(geo, rng)
    u = geo.levels[0]["stride"]
    W, H = geo.levels[0]["w"], geo.levels[0]["h"]
    assert W >= 20 and H >= 20
    pairs = {}

    def pair(name, a_hi, box_hi, a_lo, box_lo, lg):
        _put(img, geo, a_hi, box_hi, lg)
        _put(img, geo, a_lo, box_lo, lg - 0.1)
        pairs[name] = (a_hi, a_lo)

    # exact: around anchor (9, 9) in the middle
    pair("exact", geo.anchor(0, 9, 9), (8.5 * u, 8.5 * u, 10.5 * u, 10.5 * u), geo.anchor(0, 8, 8), (8.5 * u, 8.5 * u, 10.5 * u, 9.5 * u), 3.0)
    # alt: around anchor (14, 9)
    pair("alt", geo.anchor(0, 14, 9), (12.5 * u, 7.5 * u, 16.5 * u, 12.5 * u), geo.anchor(0, 13, 8), (12.5 * u, 7.5 * u, 15.5 * u, 10.5 * u), 2.5)
    # above: top-left corner, the big box [-15.5u, 16.5u]^2 from anchor (0, 0); the 27u x 19u one from anchor (1, 1)
    pair("above", geo.anchor(0, 0, 0), (-15.5 * u, -15.5 * u, 16.5 * u, 16.5 * u), geo.anchor(0, 1, 1), (-14.5 * u, -14.5 * u, 12.5 * u, 4.5 * u), 2.0)
    # below: bottom-right corner, mirrored
    x, y = W - 1, H - 1
    pair("below", geo.anchor(0, x, y), ((x - 15.5) * u, (y - 15.5) * u, (x + 16.5) * u, (y + 16.5) * u), geo.anchor(0, x - 1, y - 1),
         ((x - 14.5) * u, (y - 14.5) * u, (x + 15.5) * u, (y + 2.5) * u), 1.5)
    return img, dict(pairs=pairs)


def _case_degenerate(geo, pre_k, keep_k, rng):
    """Zero-area boxes from the decode (all bins 0: a point; zero width with a height) and, through ``box_patch``, inverted ones.  With torchvision's arithmetic two
    points overlap 0 / (0 + 0 - 0) = NaN, which is not > IOU: both stay.  Duplicates of an x-inverted box (negative area, zero intersection: -0) both stay too, while
    the duplicate of a proper box goes."""
    img = _background(geo, rng)
    u = geo.levels[0]["stride"]
    p0, p1 = geo.anchor(0, 2, 2), geo.anchor(0, 2, 3)      # two points ...
    q0 = geo.anchor(0, 3, 3)                                # ... a proper box that contains both
    z0 = geo.anchor(0, 6, 2)                                # zero width, two strides high
    r0, r1 = geo.anchor(0, 10, 10), geo.anchor(0, 9, 10)    # a proper tile and its exact duplicate
    i0, i1, i2 = geo.anchor(0, 14, 2), geo.anchor(0, 15, 2), geo.anchor(0, 16, 2)  # ranks that the patch turns into inverted boxes
    for a, lg in ((p0, 3.0), (p1, 2.9)):
        img.bins[a] = (0, 0, 0, 0)
        img.logit[a] = lg
    _put(img, geo, q0, (0.5 * u, 0.5 * u, 4.5 * u, 4.5 * u), 2.8)
    img.bins[z0] = (0, 1, 0, 1)
    img.logit[z0] = 2.7
    _put(img, geo, r0, geo.tile(r0), 2.6)
    _put(img, geo, r1, geo.tile(r0), 2.5)
    for a, lg in ((i0, 2.4), (i1, 2.3), (i2, 2.2)):
        img.logit[a] = lg  # (their decoded tiles are replaced)
    # ranks follow the logits above: 0..5 as planted, the inverted ones at ranks 6, 7, 8
    x_inv = (20.0 * u, 2.0 * u, 18.0 * u, 4.0 * u)       # x2 < x1
    xy_inv = (24.0 * u, 6.0 * u, 22.0 * u, 4.0 * u)      # both inverted: a positive "area", an empty intersection with itself
    patch = [(6, x_inv), (7, x_inv), (8, xy_inv)]
    return img, dict(points=(p0, p1), container=q0, zero_width=z0, tile=r0, tile_dup=r1, inverted_ranks=(6, 7, 8)), patch


def _case_conf_equal(geo, pre_k, keep_k, rng):
    """A candidate whose score IS the threshold (logit 0 -> 0.5 on both sides) behind two clear ones, and one just below it (logit -0.001)."""
    img = _background(geo, rng)
    hi0, hi1, eq, lo = geo.anchor(0, 1, 1), geo.anchor(1, 1, 1), geo.anchor(0, 5, 5), geo.anchor(0, 7, 7)
    img.logit[hi0], img.logit[hi1], img.logit[eq], img.logit[lo] = 2.0, 1.0, 0.0, -0.001
    return img, dict(at_conf=eq, below=lo)


def _case_level_edges(geo, pre_k, keep_k, rng):
    """Survivors on the first and on the last anchor of every level (find_level at a == start[l] and a == start[l + 1] - 1), nothing else valid."""
    img = _background(geo, rng)
    s = geo.starts
    edges = sorted(set([s[l] for l in range(len(geo.levels))] + [s[l + 1] - 1 for l in range(len(geo.levels))]))
    img.logit[rng.permutation(edges)] = _descending(len(edges), 2.0, 1.0)
    return img, dict(edges=edges)


def _case_ballot_words(geo, pre_k, keep_k, rng):
    """pre_k valid candidates whose RANKS are chosen, so that suppression crosses the 64-candidate words of the kernel's ballots:
      rank 63 is kept and suppresses rank 64 (the first bit of the next word); rank 65 overlaps 64 above IOU but 63 below it, so it is KEPT because 64 is gone;
      rank 127 is kept and suppresses rank 128; the LAST rank, pre_k - 1, is a small box nothing overlaps: kept.
    The image is cut into R x R regions (R = 64 px, 32 below 256 px).  Every level-0 / level-1 anchor of a region carries the region's box -- level 0 [Ri - 4, Ri + R + 4]^2,
    level 1 [Ri - 8, Ri + R + 8]^2, IoU ((R + 8) / (R + 16))^2 >= 0.69; neighbouring regions' boxes overlap by an 8-px strip, IoU <= 0.11 -- and the region's LEADER has
    the lowest rank in it: the leaders survive (fewer than 100 with the level-2 tiles that fill up a pre_k == A geometry), every other member is suppressed."""
    L = geo.levels
    S = L[0]["w"] * L[0]["stride"]
    R = 64 if S >= 256 else 32
    assert S % R == 0 and S // R >= 3 and L[0]["stride"] == 8 and L[1]["stride"] == 16, "ballot_words needs a stride-8/16 pyramid of at least 3 x 3 regions"
    img = _background(geo, rng)
    nr = S // R
    regions = [(i, j) for j in range(nr) for i in range(nr)]

    def members(i, j):
        m0 = [geo.anchor(0, x, y) for y in range(j * R // 8, (j + 1) * R // 8) for x in range(i * R // 8, (i + 1) * R // 8)]
        m1 = [geo.anchor(1, x, y) for y in range(j * R // 16, (j + 1) * R // 16) for x in range(i * R // 16, (i + 1) * R // 16)]
        return m0, m1

    def box0(i, j):
        return (R * i - 4, R * j - 4, R * i + R + 4, R * j + R + 4)

    def box1(i, j):
        return (R * i - 8, R * j - 8, R * i + R + 8, R * j + R + 8)

    rank_of: Dict[int, int] = {}      # anchor -> rank
    box_of: Dict[int, tuple] = {}
    # the two special regions: the last column (the shifted boxes of ranks 64 / 65 leave the image, no neighbour to meet), rows 0 and 1
    ra, rb = (nr - 1, 0), (nr - 1, 1)
    wb = (R + 8) // 8                          # the region box in level-0 bins
    s = -(-wb // 6)                            # shift in bins: IoU(63, 64) = (w - s) / (w + s) > 1/2  <=>  s < w / 3;  IoU(63, 65) = (w - 2s) / (w + 2s) <= 1/2  <=>  s >= w / 6
    assert wb / 6 <= s < wb / 3
    a0, _ = members(*ra)
    right = [a for a in a0 if geo.locate(a)[1] == (ra[0] + 1) * R // 8 - 1]  # the region's right-most level-0 column: its centres lie inside the shifted boxes too
    l63, m64, m65 = right[0], right[1], right[2]
    bx = box0(*ra)
    rank_of.update({l63: 63, m64: 64, m65: 65})
    box_of.update({l63: bx, m64: (bx[0] + 8 * s, bx[1], bx[2] + 8 * s, bx[3]), m65: (bx[0] + 16 * s, bx[1], bx[2] + 16 * s, bx[3])})
    b0, _ = members(*rb)
    l127, m128 = b0[0], b0[1]
    rank_of.update({l127: 127, m128: 128})
    box_of.update({l127: box0(*rb), m128: box0(*rb)})
    # the last rank: a level-0 tile inside an ordinary region (IoU with the region's boxes <= 64 / 1600)
    normal = [r for r in regions if r not in (ra, rb)]
    last = members(*normal[-1])[0][-1]
    rank_of[last] = pre_k - 1
    box_of[last] = geo.tile(last)
    # leaders of the ordinary regions: ranks 0 .. len(normal) - 1 (< 63)
    assert len(normal) < 63
    pool = []
    for r_i, reg in enumerate(normal):
        m0, m1 = members(*reg)
        m0 = [a for a in m0 if a != last]
        rank_of[m0[0]] = r_i
        box_of[m0[0]] = box0(*reg)
        pool += [(a, box0(*reg)) for a in m0[1:]] + [(a, box1(*reg)) for a in m1]
    for reg, used in ((ra, (l63, m64, m65)), (rb, (l127, m128))):  # the special regions' other members: behind their leader
        m0, m1 = members(*reg)
        pool += [(a, box0(*reg)) for a in m0 if a not in used] + [(a, box1(*reg)) for a in m1]
    pool = [pool[k] for k in rng.permutation(len(pool))]
    special_low = {63: None, 64: None, 65: None, 127: None, 128: None}
    free = [r for r in range(len(normal), pre_k - 1) if r not in special_low]
    # ranks below 63 / 127 must not go to members of the special regions (their leader has to come first): ordinary members first
    in_special = {a for reg in (ra, rb) for m in members(*reg) for a in m}
    pool.sort(key=lambda ab: ab[0] in in_special)
    fill = pool[: len(free)]
    if len(fill) < len(free):  # pre_k == A: the remaining anchors (level 2 and beyond) as tiles, at the lowest free ranks
        rest = [a for a in range(geo.A) if a not in rank_of and a not in {p[0] for p in pool}]
        fill += [(a, geo.tile(a)) for a in rest[: len(free) - len(fill)]]
    assert len(fill) == len(free), (len(fill), len(free))
    for r, (a, bxm) in zip(free, fill):
        rank_of[a] = r
        box_of[a] = bxm
    assert sorted(rank_of.values()) == list(range(pre_k))
    lg = _descending(pre_k)
    for a, r in rank_of.items():
        _put(img, geo, a, box_of[a], lg[r])
    return img, dict(rank63=l63, rank64=m64, rank65=m65, rank127=l127, rank128=m128, rank_last=last, leaders=[a for a, r in rank_of.items() if r < len(normal)])


_BUILDERS = dict(empty=_case_empty, all_valid=_case_all_valid, exact_keep_k=_case_exact_keep_k, keep_k_plus_1=_case_keep_k_plus_1, ties=_case_ties,
                 iou_exact=_case_iou_exact, degenerate=_case_degenerate, conf_equal=_case_conf_equal, level_edges=_case_level_edges, ballot_words=_case_ballot_words)


def _case_random(geo, pre_k, keep_k, rng):
    """Any geometry (the many-image set): a random share of the anchors valid (none at all for every fifth image), as tiles; a third of them, where the anchor to the left is
    free, with a lower-scored exact duplicate."""
    img = _background(geo, rng)
    share = 0.0 if rng.integers(5) == 0 else rng.uniform(0.05, 0.9)
    valid = [int(a) for a in rng.permutation(geo.A)[: int(round(share * geo.A))]]
    if valid:
        img.logit[valid] = _descending(len(valid), 3.0, 1.0)
    taken = set(valid)
    n_dup = 0
    for a in valid[:: 3]:
        l, x, y = geo.locate(a)
        if x == 0:
            continue
        left = geo.anchor(l, x - 1, y)
        if left in taken:
            continue
        taken.add(left)
        _put(img, geo, left, geo.tile(a), 0.9 - 0.01 * n_dup)
        n_dup += 1
    return img, dict(valid=len(valid))


# ---- tensors ----------------------------------------------------------------------------------------------------------------------------------------------------------
def render(geo: Geometry, images: List[Image], seed: int) -> List[torch.Tensor]:
    """The prediction tensors of the images: per level f32 [B, h, w, pitch] = [17 DFL logits x 4 sides | class logit | 3 unused | raw FLAME channels | pad]."""
    g = torch.Generator().manual_seed(seed)
    B = len(images)
    bins = torch.from_numpy(np.stack([im.bins for im in images])).long()      # [B, A, 4]
    logit = torch.from_numpy(np.stack([im.logit for im in images])).float()   # [B, A]
    out = []
    for l, lv in enumerate(geo.levels):
        h, w, pitch = lv["h"], lv["w"], lv["pitch"]
        assert pitch >= PRED_FLAME_OFF + geo.shape_c + geo.expr_c + 13
        s0, s1 = geo.starts[l], geo.starts[l + 1]
        t = torch.randn(B, h * w, pitch, generator=g) * 1.5
        reg = torch.full((B, h * w, 4, po.REG_MAX + 1), DFL_LO)
        reg.scatter_(3, bins[:, s0:s1, :, None], DFL_HI)
        t[..., : 4 * (po.REG_MAX + 1)] = reg.reshape(B, h * w, -1)
        t[..., PRED_CLS_OFF] = logit[:, s0:s1]
        out.append(t.reshape(B, h, w, pitch).contiguous())
    return out


def build_case_set(geo: Geometry, pre_k: int, keep_k: int, names=CASE_NAMES, seed: int = 7) -> CaseSet:
    assert 1 <= keep_k <= pre_k <= min(1024, geo.A)
    images, cases = [], []
    for i, name in enumerate(names):
        rng = np.random.default_rng([seed, CASE_NAMES.index(name)])
        got = _BUILDERS[name](geo, pre_k, keep_k, rng)
        images.append(got[0])
        cases.append(Case(name, i, got[1], list(got[2]) if len(got) > 2 else []))
    return CaseSet(geo, pre_k, keep_k, render(geo, images, seed), cases)


def build_random_set(geo: Geometry, pre_k: int, keep_k: int, B: int, seed: int = 11) -> CaseSet:
    """B random images (``_case_random``) for any geometry: the many-image head-list test."""
    assert 1 <= keep_k <= pre_k <= min(1024, geo.A)
    rng = np.random.default_rng(seed)
    got = [_case_random(geo, pre_k, keep_k, rng) for _ in range(B)]
    return CaseSet(geo, pre_k, keep_k, render(geo, [g_[0] for g_ in got], seed), [Case("random", i, g_[1]) for i, g_ in enumerate(got)])


# ---- the oracle's view ----------------------------------------------------------------------------------------------------------------------------------------------------
def oracle_dense(geo: Geometry, preds: List[torch.Tensor]):
    """ndfl_decode of the planted tensors: boxes [B, A, 4], scores [B, A, 1], flame [B, A, 413]."""
    S_c, E_c, o = geo.shape_c, geo.expr_c, PRED_FLAME_OFF
    olevels = []
    for t in preds:
        nchw = t.permute(0, 3, 1, 2)
        fl = po.assemble_flame_channels(nchw[:, o : o + S_c], nchw[:, o + S_c : o + S_c + E_c], nchw[:, o + S_c + E_c : o + S_c + E_c + 6],
                                        nchw[:, o + S_c + E_c + 6 : o + S_c + E_c + 9], nchw[:, o + S_c + E_c + 9 : o + S_c + E_c + 12],
                                        nchw[:, o + S_c + E_c + 12 : o + S_c + E_c + 13])
        olevels.append((nchw[:, :68], nchw[:, 68:69], fl))
    return po.ndfl_decode(olevels, tuple(lv["stride"] for lv in geo.levels))


def oracle_view(cs: CaseSet):
    """(dense boxes, dense scores, dense flame), (candidate boxes [B, pre_k, 4] with the planted overrides, scores [B, pre_k, 1], flame [B, pre_k, 413], anchor idx [B, pre_k])."""
    rb, rs, rf = oracle_dense(cs.geo, cs.preds)
    bb, ss, ff, idx = po.decoding_topk(rb, rs, rf, cs.pre_k)
    bb = bb.clone()
    cs.patch_boxes(bb)
    return (rb, rs, rf), (bb, ss, ff, idx)


def oracle_select(cs: CaseSet, cand_boxes, cand_scores, cand_flame, conf: float = CONF, iou: float = IOU, keep_k: Optional[int] = None):
    """postprocess_batched on candidate tensors (the oracle's own or the engine's): per image (boxes [n, 4], scores [n], flame [n, 413])."""
    if cand_scores.dim() == 2:
        cand_scores = cand_scores.unsqueeze(-1)
    return po.postprocess_batched(cand_boxes, cand_scores, cand_flame, conf, iou, pre_nms_max=cs.pre_k, post_nms_max=keep_k or cs.keep_k)


def oracle_keep(cand_boxes_b: torch.Tensor, cand_scores_b: torch.Tensor, conf: float = CONF, iou: float = IOU) -> np.ndarray:
    """Candidate ranks one image's NMS keeps BEFORE the keep_k cut, in visit order (nms_torchvision on the >= conf prefix: the candidates are sorted)."""
    s = cand_scores_b.reshape(-1).numpy()
    n = int((s >= np.float32(conf)).sum())
    assert bool((s[:n] >= np.float32(conf)).all())
    return po.nms_torchvision(cand_boxes_b[:n].numpy(), s[:n], iou)


def iou_f32(a, b) -> np.float32:
    """IoU of two boxes in the oracle's float32 arithmetic (nms_torchvision, one pair)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    area = lambda q: np.float32(np.float32(q[2] - q[0]) * np.float32(q[3] - q[1]))  # noqa: E731
    w = max(np.float32(0), np.float32(min(a[2], b[2]) - max(a[0], b[0])))
    h = max(np.float32(0), np.float32(min(a[3], b[3]) - max(a[1], b[1])))
    inter = np.float32(w * h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(inter / np.float32(np.float32(area(a) + area(b)) - inter))
