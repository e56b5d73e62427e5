"""Exact-arithmetic inputs for the stem-in-pair launch, the "u" tile of csrc/ds_b2b.hip (no GPU, no library): u8 images, stem weights, and the weights of the two convs
behind the stem, chosen so that EVERY stored bf16 of the launch has exactly one right value.  The method of tests/conv_exact_cases.py, carried through three layers and
through the / 255 fold:

  * the tile computes the stem as  sum_k q_k * (hi_k + mid_k + lo_k) + b  with  hi + mid + lo = v = fl32(w / 255)  (three bf16 values), q a u8 pixel (an exact bf16).
    The stem weights here are DEFINED through v: v is drawn on a grid 2^-m, and w is the float32 near 255 v whose correctly rounded quotient w / 255 is that v (about one
    v in 255 has none: another is drawn).  Every product q * part is exact, every part is a multiple of the grid, and the operand ranges keep
    sum |q| (|hi| + |mid| + |lo|) + |b|  below 2^24 grid units: the fp32 accumulator then holds the mathematically exact stem value in ANY summation order, and what goes
    into the planes is ONE round-to-nearest-even of it (after which ReLU changes nothing but the negative values);
  * the stem's bf16 values are multiples of the same grid; with small-integer weights behind them the downsample's and the 1x1's sums stay exact in the same way.

    stem_pair_case(variant, S, B, family, seed)    the operands of one case (cached and shared: do not write to them)
    program_arrays(case)                           the same in the layouts arch.Program.weights / .biases hold for ops 0, 1, 2
    reference(case, fault, rounding, stem)         the chain in float64, explicit zero padding; planted faults; wrong roundings at the stem; or from a given stem tensor
    abs_sum_bounds(case)                           max sum |terms| + |bias| per layer, in grid units: no partial sum, in any order, exceeds it
    on_grid(case, stem) / exact_pixels(case, stem) for a stem tensor that another kernel computed: its values on the grid, the output pixels that read only such values

Families (which fault each one can show: tests/test_stem_pair_exact_cases_host.py):
    chain      dense pixels 0..255, v an integer in [-2, 2], integer biases; integer downsample weights in [-2, 2] and 1x1 weights in [-1, 1]: three real layers
    pass_int   the chain's kind of stem in front of a PASS-THROUGH pair: every downsample channel copies one stem channel of one tap (ky, kx) in {1, 2} x {1, 2}
               (weight 1, bias 0), the 1x1 is a one-hot selector: every compared output is one stem value untouched (an already rounded bf16 goes through ReLU and
               round-to-nearest-even unchanged).  Seeds 0 and 1 select complementary halves of the 4 x 48 (tap, channel) pairs: together every stem pixel of the map
    pass_mid   pass-through; dense pixels, v = k / 8 with |k| < 2^11: hi and mid both non-zero
    pass_lo    pass-through; pixels 0..3, v = k * 2^-14; two fifths of the weights of a main channel have 2^17 <= |k| < 2^18 and are drawn until lo != 0 (an 18-bit
               span: a 17-bit one never leaves a third part, |v - hi| <= 2^8 units always fits mid), the others |k| < 2^12
In pass_mid and pass_lo the stem values of the main channels are large on their grid (ties are one value in thousands there), so every sixth channel is a TIE channel:
tiny |k| and a bias that puts the sums where every other grid point is a tie.

Significand bits are counted as in conv_exact_cases (8 = bf16)."""
from __future__ import annotations

import functools
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_exact_cases as cx

FAMILIES = ("chain", "pass_int", "pass_mid", "pass_lo")
FAULTS = ("drop_lo", "drop_mid", "pixel_sign", "left_clamp", "top_clamp", "ninth_row", "ring_kept")
C2 = {"vgg_heads_m": 128, "vgg_heads_l": 192}  # couts of conv1|conv2 (2 x hidden of stage 1)
GRID_LOG2 = {"chain": 0, "pass_int": 0, "pass_mid": -3, "pass_lo": -14}
SIZES = ((96, 3), (64, 5))  # (S, B): 96 = a 3 x 3 grid of 8 x 8 output tiles per image (an interior tile, four edges, four corners); 64 = four corner tiles
FAMILY_SEEDS = (("chain", 0), ("pass_int", 0), ("pass_int", 1), ("pass_mid", 0), ("pass_mid", 1), ("pass_lo", 0), ("pass_lo", 1))
# what tests/test_gpu_stem_pair_exact.py runs and tests/test_stem_pair_exact_cases_host.py vouches for: (variant, S, B, family, seed)
GPU_CASES = [(v, S, B, f, s) for v in ("vgg_heads_m", "vgg_heads_l") for S, B in SIZES for f, s in FAMILY_SEEDS]
TIE_EVERY = 6  # pass_mid / pass_lo: channels c % 6 == 5 are tie channels
LO_WIDE_SHARE = 0.4
# integer stem biases (chain, pass_int), by c % 16: the sum itself has a standard deviation near 1 100, so these only make sure that no channel sits in one binade
STEM_BIAS_INT = (0, 257, -259, 514, -518, 771, 1030, -1285, 300, 3, 130, -385, 2056, 645, -66, 1542)


def split3(v32: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """float32 -> (hi, mid, lo) as float64 arrays that hold bf16 values: the tile's own split, each part the nearest-even bf16 of what the parts before it left"""
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32))
    h = t.bfloat16().float()
    r1 = t - h
    m = r1.bfloat16().float()
    l = (r1 - m).bfloat16().float()
    return h.double().numpy(), m.double().numpy(), l.double().numpy()


def _weights_for(v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """v (float32 targets) -> (w float32, found): w near 255 v with np.float32(w) / np.float32(255) == v (numpy divides float32 correctly rounded)"""
    v = v.astype(np.float32)
    w0 = (v.astype(np.float64) * 255.0).astype(np.float32)
    w, found = w0.copy(), np.zeros(v.shape, dtype=bool)
    for step in (0, 1, -1, 2, -2, 3, -3):
        c = w0.copy()
        for _ in range(abs(step)):
            c = np.nextafter(c, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
        ok = ~found & ((c / np.float32(255.0)).astype(np.float32) == v)
        w[ok], found = c[ok], found | ok
    return w, found


def _draw_until(rng, shape, draw: Callable, accept: Optional[Callable] = None) -> Tuple[np.ndarray, np.ndarray]:
    """v = draw(n) (float32, on the family's grid) for every slot, redrawn where no float32 w gives fl32(w / 255) == v or where `accept(v)` says no"""
    n = int(np.prod(shape))
    v = draw(n)
    for _ in range(200):
        w, ok = _weights_for(v)
        if accept is not None:
            ok &= accept(v)
        if ok.all():
            return v.reshape(shape), w.reshape(shape)
        v[~ok] = draw(int((~ok).sum()))
    raise AssertionError("no weights found")


def _stem_operands(family: str, rng) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """(v [27][48] float32, w [27][48] float32, bias [48] float32, largest pixel)"""
    g = 2.0 ** GRID_LOG2[family]
    if family in ("chain", "pass_int"):
        v, w = _draw_until(rng, (27, 48), lambda n: rng.integers(-2, 3, size=n).astype(np.float32))
        bias = np.array([STEM_BIAS_INT[c % 16] for c in range(48)], dtype=np.float32)
        return v, w, bias, 255
    tie = np.arange(48) % TIE_EVERY == TIE_EVERY - 1
    v, w = np.zeros((27, 48), np.float32), np.zeros((27, 48), np.float32)
    bias = np.zeros(48, np.float32)
    if family == "pass_mid":
        vm, wm = _draw_until(rng, (27, 48), lambda n: (rng.integers(-(2 ** 11) + 1, 2 ** 11, size=n) * g).astype(np.float32), lambda v: split3(v)[1] != 0)
        vt, wt = _draw_until(rng, (27, 48), lambda n: (rng.integers(-2, 3, size=n) * g).astype(np.float32))
        bias[~tie] = (rng.integers(-4000, 4001, size=int((~tie).sum())) * g).astype(np.float32)
        bias[tie] = (rng.integers(300, 700, size=int(tie.sum())) * g).astype(np.float32)  # sums of +-135: most values in [32, 128), where odd eighths / quarters tie
        pmax = 255
    else:
        sign = lambda n: rng.choice((-1, 1), size=n)  # noqa: E731
        vw, ww = _draw_until(rng, (27, 48), lambda n: (rng.integers(2 ** 17, 2 ** 18, size=n) * sign(n) * g).astype(np.float32), lambda v: split3(v)[2] != 0)
        vn, wn = _draw_until(rng, (27, 48), lambda n: (rng.integers(0, 2 ** 12, size=n) * sign(n) * g).astype(np.float32))
        wide = rng.random((27, 48)) < LO_WIDE_SHARE
        vm, wm = np.where(wide, vw, vn), np.where(wide, ww, wn)
        vt, wt = _draw_until(rng, (27, 48), lambda n: (rng.integers(-8, 9, size=n) * g).astype(np.float32))
        bias[~tie] = (rng.integers(-(2 ** 16), 2 ** 16 + 1, size=int((~tie).sum())) * g).astype(np.float32)
        bias[tie] = (rng.integers(330, 440, size=int(tie.sum())) * g).astype(np.float32)  # sums of +-50 units: values in [256, 512) units, where every odd unit ties
        pmax = 3
    v[:, ~tie], w[:, ~tie] = vm[:, ~tie], wm[:, ~tie]
    v[:, tie], w[:, tie] = vt[:, tie], wt[:, tie]
    return v, w, bias, pmax


def selector(seed: int, c: int) -> Tuple[int, int, int]:
    """pass-through downsample channel c of selector set `seed` -> (ky, kx, stem channel): the 192 (tap, channel) pairs in two halves, each with all four taps and
    all 48 channels (so each half alone sees row 0 and column 0 of the stem map)"""
    ch, ky = c % 48, 1 + c // 48
    return ky, 1 + (ch + seed) % 2, ch


def final_source(o: int) -> int:
    """pass-through: the downsample channel that output channel o of the 1x1 copies (every one of the 96 at least once, in another order the second time round)"""
    return o if o < 96 else (7 * o + 3) % 96


@functools.lru_cache(maxsize=None)
def stem_pair_case(variant: str, S: int, B: int, family: str, seed: int = 0) -> Dict[str, object]:
    """images u8 [B,S,S,3]; w [27][48] (k = (ky * 3 + kx) * 3 + ci) with v = fl32(w / 255) and its parts hi / mid / lo (float64), b_stem [48]; w_ds [96,3,3,64]
    (input channels 48..63 zero), b_ds [96]; w_11 [C2,1,1,96], b_11 [C2]: float32 arrays.  For the pass families `seed` also picks the selector set (seed % 2)."""
    assert family in FAMILIES and variant in C2 and S % 32 == 0
    rng = np.random.default_rng([20251021, FAMILIES.index(family), seed, S, B, C2[variant]])
    v, w, b_stem, pmax = _stem_operands(family, rng)
    assert np.array_equal((w / np.float32(255.0)).astype(np.float32), v) and w.dtype == np.float32  # the identity, for every weight
    hi, mid, lo = split3(v)
    assert np.array_equal(hi + mid + lo, v.astype(np.float64))
    images = rng.integers(0, pmax + 1, size=(B, S, S, 3)).astype(np.uint8)
    c2 = C2[variant]
    w_ds, b_ds = np.zeros((96, 3, 3, 64), np.float32), np.zeros(96, np.float32)
    w_11, b_11 = np.zeros((c2, 1, 1, 96), np.float32), np.zeros(c2, np.float32)
    if family == "chain":
        w_ds[..., :48] = rng.integers(-2, 3, size=(96, 3, 3, 48))
        b_ds[:] = rng.integers(-400, 401, size=96)
        w_11[:] = rng.integers(-1, 2, size=(c2, 1, 1, 96))
        b_11[:] = rng.integers(-400, 401, size=c2)
    else:
        for c in range(96):
            ky, kx, ch = selector(seed, c)
            w_ds[c, ky, kx, ch] = 1.0
        for o in range(c2):
            w_11[o, 0, 0, final_source(o)] = 1.0
    return {"variant": variant, "S": S, "B": B, "family": family, "seed": seed, "grid": 2.0 ** GRID_LOG2[family], "images": torch.from_numpy(images),
            "w": w, "v": v, "hi": hi, "mid": mid, "lo": lo, "b_stem": b_stem, "w_ds": w_ds, "b_ds": b_ds, "w_11": w_11, "b_11": b_11}


def program_arrays(case: Dict[str, object]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """(weights, biases) of ops 0, 1, 2 as arch.Program holds them: flat float32; the stem as [48][ky][kx][ci], the convs as [cout][ky][kx][cin]"""
    ws = [np.ascontiguousarray(case["w"].T).reshape(-1), case["w_ds"].reshape(-1).copy(), case["w_11"].reshape(-1).copy()]
    bs = [case["b_stem"].copy(), case["b_ds"].copy(), case["b_11"].copy()]
    return [a.astype(np.float32) for a in ws], [a.astype(np.float32) for a in bs]


# ----------------------------------------------------------------------------------------------------------------------
# the chain in float64
# ----------------------------------------------------------------------------------------------------------------------
def _taps_s2(x: torch.Tensor, left: Optional[torch.Tensor] = None, top: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3 / stride-2 / pad-1 im2col of x [B,H,W,C] (H, W even) through cx.taps, with the padding made HERE so that a fault can fill it: column -1 = `left` [B,H,C],
    row -1 = `top` [B,W,C] (the corner and everything else: zeros).  Two rows / columns are put in front (cx.taps adds a third, of zeros): its output row i + 1 reads
    rows 2 i - 1 .. 2 i + 1 of x."""
    xp = F.pad(x, (0, 0, 2, 0, 2, 0))
    if left is not None:
        xp[:, 2:, 1] = left
    if top is not None:
        xp[:, 1, 2:] = top
    return cx.taps(xp, 3, 2)[:, 1:, 1:]


def _round_store(y: torch.Tensor, fn: Callable = cx.rne) -> torch.Tensor:
    """float64 values that a correct layer holds exactly in its fp32 accumulator -> ReLU and the bf16 store (`fn` on the float32 value), as float32"""
    y32 = y.float()
    assert torch.equal(y32.double(), y), "not exact in fp32"
    return torch.relu(fn(y32, cx.BF16)) + 0.0  # (the tile rounds, then takes the maximum with +0 on the packed values: the same bits, and no -0)


def stem_exact(case: Dict[str, object], fault: Optional[str] = None) -> torch.Tensor:
    """[B,S/2,S/2,48] float64: sum q * v + b before ReLU and rounding"""
    q = case["images"].double()
    if fault == "pixel_sign":
        q = torch.where(q >= 128, q - 256, q)
    A = _taps_s2(q, left=q[:, :, 0] if fault == "left_clamp" else None, top=q[:, 0] if fault == "top_clamp" else None)
    if fault == "ninth_row":
        A = A.clone()
        src = A.clone()
        for ky in range(3):
            A[..., ky * 9 + 8] = src[..., ((ky + 1) % 3) * 9 + 8]
    v = case["hi"] + case["mid"] + case["lo"]
    if fault == "drop_lo":
        v = case["hi"] + case["mid"]
    if fault == "drop_mid":
        v = case["hi"] + case["lo"]
    return A @ torch.from_numpy(v) + torch.from_numpy(case["b_stem"]).double()


def reference(case: Dict[str, object], fault: Optional[str] = None, rounding: Optional[str] = None, stem: Optional[torch.Tensor] = None, stages: bool = False):
    """What a correct launch stores, as float32 that holds bf16 values: [B,S/4,S/4,C2] -- couts in the order of the weights' rows, which the program stores as two
    segments.  fault: one of FAULTS.  rounding: one of cx.WRONG_ROUNDINGS, applied at the stem instead of round-to-nearest-even.  stem: a given stem tensor
    [B,S/2,S/2,48] (bf16 values) instead of this file's own: the two convs behind it alone.  stages: (stem, downsample, output) instead of the output."""
    assert fault in (None,) + FAULTS and rounding in (None,) + tuple(cx.WRONG_ROUNDINGS)
    if stem is None:
        s = _round_store(stem_exact(case, fault), cx.WRONG_ROUNDINGS[rounding] if rounding else cx.rne)
    else:
        assert fault is None and rounding is None
        s = torch.where(on_grid(case, stem), stem.float(), torch.zeros(()))  # (outputs that read a value off the grid are not defined exactly: exact_pixels)
    B, H, W, _ = s.shape
    ring = None
    if fault == "ring_kept":  # a stem pixel at gy == -1 or gx == -1 sees only the zeros above / left of the image: ReLU(bias), stored
        ring = _round_store(torch.from_numpy(case["b_stem"]).double())
    A = _taps_s2(s.double(), left=ring.double().expand(B, H, 48) if ring is not None else None, top=ring.double().expand(B, W, 48) if ring is not None else None)
    if ring is not None:  # the corner (-1, -1): tap (0, 0) of output pixel (0, 0)
        A[:, 0, 0, :48] = ring.double()
    d = _round_store(A @ torch.from_numpy(case["w_ds"][..., :48].reshape(96, 432).T.copy()).double() + torch.from_numpy(case["b_ds"]).double())
    o = _round_store(d.double() @ torch.from_numpy(case["w_11"].reshape(-1, 96).T.copy()).double() + torch.from_numpy(case["b_11"]).double())
    return (s, d, o) if stages else o


def on_grid(case: Dict[str, object], stem: torch.Tensor) -> torch.Tensor:
    """which values of a stem tensor are multiples of the case's grid.  This file's own stem values all are.  The library's stem KERNEL sums fl(q / 255) * w in an fmaf
    chain: where the exact sum is 0 it may hold 1e-5 instead, which no bf16 rounding brings back to the grid, and a sum that reads it is no longer exact in fp32."""
    u = stem.double() / case["grid"]
    return u == u.round()


def exact_pixels(case: Dict[str, object], stem: torch.Tensor) -> torch.Tensor:
    """[B,S/4,S/4] bool: the output pixels whose 3 x 3 x 48 stem values are all on the grid -- where reference(case, stem=stem) is the one right value"""
    off = (~on_grid(case, stem)).any(-1, keepdim=True).double()
    return _taps_s2(off).sum(-1) == 0


def abs_sum_bounds(case: Dict[str, object]) -> Tuple[float, float, float]:
    """max over the outputs of sum |terms| + |bias| at the stem (the three parts of a weight counted apart), the downsample and the 1x1, in units of the grid"""
    g = case["grid"]
    parts = torch.from_numpy(np.abs(case["hi"]) + np.abs(case["mid"]) + np.abs(case["lo"]))
    b0 = float((_taps_s2(case["images"].double()) @ parts + torch.from_numpy(np.abs(case["b_stem"])).double()).max())
    s, d, _ = reference(case, stages=True)
    b1 = float((_taps_s2(s.double()) @ torch.from_numpy(np.abs(case["w_ds"][..., :48]).reshape(96, 432).T.copy()).double() + torch.from_numpy(np.abs(case["b_ds"])).double()).max())
    b2 = float((d.double() @ torch.from_numpy(np.abs(case["w_11"]).reshape(-1, 96).T.copy()).double() + torch.from_numpy(np.abs(case["b_11"])).double()).max())
    return b0 / g, b1 / g, b2 / g


def output_bits(y: torch.Tensor) -> torch.Tensor:
    """float32 that holds bf16 values -> int16 bit patterns"""
    return cx.storage_bits(y, cx.BF16)


def source_of_output(case: Dict[str, object], o: int) -> Tuple[int, int, int]:
    """pass families: output channel o at output pixel (y, x) is stem channel ch at stem pixel (2 y + ky - 1, 2 x + kx - 1): (ky, kx, ch)"""
    return selector(case["seed"], final_source(o))
