"""Exact-arithmetic inputs for the conv tiles (no GPU, no library): small INTEGER activations, weights, biases and residuals, so that every product and every
partial sum of a convolution is an integer far below 2^24 -- exact in fp32 in ANY summation order, grouping, ring depth, MFMA shape or K split.  Every correct
tile then holds the same fp32 value before its store, and the stored 16-bit value is one well-defined rounding of it: a comparison needs no tolerance, and a
store that truncates, rounds halves up, drops or repeats one product of a long K loop, or loses the sign of a zero shows as a difference of bits.

    exact_case(...)      seeded x, W, bias (and a residual with alpha = 0.5) for one shape and one storage width
    reference(...)       the convolution in float64 from those integers, explicit zero padding, activation and residual in float64; three planted faults
    rne / truncate / half_up / half_away     restatements of a float32 -> `bits`-significand store on the float32 bit pattern

tests/test_conv_exact_cases_host.py checks on the CPU what makes the cases mean something (exactness in several summation orders, the share of ties, that the wrong
roundings and the planted faults are visible); tests/test_gpu_conv_exact.py feeds the cases to every tile and compares bits.

Storage widths are counted in significand bits, the implicit one included: 8 = bf16, 11 = fp16."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

BF16, FP16 = 8, 11
ALPHA = 0.5  # a power of two: alpha * (integer residual) is a half-integer, still exact

# (B, H, W, Cin, Cout, k, stride): the smallest shapes at which tiles are known to break (CONV_CASES and the r / w tile tests of tests/test_gpu_parity.py)
SHAPES = [
    (1, 16, 16, 32, 32, 1, 1),  # smallest 1x1
    (1, 5, 5, 32, 13, 1, 1),  # fp32 output, ragged cout
    (2, 11, 13, 96, 96, 3, 1),  # 143 pixels per image: linear pixel tiles straddle images
    (1, 22, 44, 128, 128, 3, 1),  # ragged map under 128-wide tiles
    (3, 9, 19, 192, 192, 3, 1),  # K = 1728
    (1, 8, 12, 512, 128, 3, 1),  # K = 4608, the longest K of the network
    (2, 40, 40, 64, 128, 3, 1),  # 40-wide maps
    (2, 23, 45, 96, 192, 3, 2),  # odd input, stride 2
    (2, 32, 48, 96, 192, 3, 2),  # the r tile
    (5, 24, 32, 96, 96, 3, 1),  # the w tiles
    (2, 19, 19, 576, 192, 1, 1),  # 1x1 with K = 576
]

X_MAX, W_MAX, RES_MAX = 3, 4, 64
# The bias of output channel c is BIAS_TABLE[storage][c % 16].  The conv sum itself is small (its standard deviation is sqrt(K * 4 * 20/3): 29 at K = 32, 350 at
# K = 4608), so the bias decides the binade of an output and with it whether ties exist there: integers tie from 2^bits on (bf16: |y| >= 256, fp16: |y| >= 2048).
# Both tables keep a quarter of the channels below that (exactly representable outputs, and the only place where a ReLU yields zeros next to small values), spread the
# rest over four to five binades of both signs, and stay far from the storage's largest finite value (fp16: 65 504).
BIAS_TABLE = {
    BF16: (0, 257, -259, 514, -518, 771, 1030, -1285, 2060, 3, 130, -385, 4112, 645, -66, 1542),
    FP16: (0, 2056, -2072, 4112, -4144, 6168, 8240, -10280, 16480, 24, 1040, -3080, 32896, 5160, -528, 12336),
}
FAULTS = ("tap_shift", "drop_channel", "res_before_act")


def out_hw(H: int, W: int, k: int, stride: int) -> Tuple[int, int]:
    return (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1


@functools.lru_cache(maxsize=None)
def exact_case(B: int, H: int, W: int, Cin: int, Cout: int, k: int, stride: int, seed: int = 0, storage: int = BF16) -> Dict[str, object]:
    """x [B,H,W,Cin], W [Cout,k,k,Cin], bias [Cout], res [B,Ho,Wo,Cout]: float32 tensors that hold integers; alpha.  x, W and res do not depend on `storage`
    (the same operands under both bias tables).  The tensors are shared between callers: do not write to them."""
    rng = np.random.default_rng([20250917, seed, B, H, W, Cin, Cout, k, stride])
    x = rng.integers(-X_MAX, X_MAX + 1, size=(B, H, W, Cin))
    Wt = rng.integers(-W_MAX, W_MAX + 1, size=(Cout, k, k, Cin))
    Ho, Wo = out_hw(H, W, k, stride)
    res = rng.integers(-RES_MAX, RES_MAX + 1, size=(B, Ho, Wo, Cout))
    table = BIAS_TABLE[storage]
    bias = np.array([table[c % len(table)] for c in range(Cout)])
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    return {"x": f(x), "W": f(Wt), "bias": f(bias), "res": f(res), "alpha": ALPHA, "shape": (B, H, W, Cin, Cout, k, stride), "storage": storage}


def taps(x: torch.Tensor, k: int, stride: int, shift_tap: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """im2col with explicit zero padding: [B,H,W,Cin] -> [B,Ho,Wo,k*k*Cin], K ordered (ky, kx, cin).  shift_tap: that tap reads one column further right (a planted fault)."""
    B, H, W, Cin = x.shape
    p = k // 2
    Ho, Wo = out_hw(H, W, k, stride)
    xp = F.pad(x, (0, 0, p, p + 1, p, p))  # one spare zero column on the right for the shifted tap
    cols = []
    for ky in range(k):
        for kx in range(k):
            dx = kx + (1 if shift_tap == (ky, kx) else 0)
            cols.append(xp[:, ky : ky + stride * (Ho - 1) + 1 : stride, dx : dx + stride * (Wo - 1) + 1 : stride, :])
    return torch.cat(cols, dim=-1)


def reference(case: Dict[str, object], act: int = 0, with_res: bool = False, fault: Optional[str] = None) -> torch.Tensor:
    """[B,Ho,Wo,Cout] float64: act(conv(x, W) + bias) (+ alpha * res), act 0 = none, 1 = ReLU.  fault plants one structural error:
    tap_shift (tap (0, 0) reads one column to the right), drop_channel (input channel 1 is missing from K), res_before_act (the residual goes inside the activation)."""
    assert act in (0, 1) and fault in (None,) + FAULTS
    _, _, _, Cin, Cout, k, stride = case["shape"]
    A = taps(case["x"].double(), k, stride, shift_tap=(0, 0) if fault == "tap_shift" else None)
    Wm = case["W"].double().clone()
    if fault == "drop_channel":
        Wm[..., 1] = 0.0
    y = A @ Wm.reshape(Cout, k * k * Cin).T + case["bias"].double()
    r = case["alpha"] * case["res"].double() if with_res else None
    if fault == "res_before_act":
        assert with_res
        y, r = y + r, None
    if act == 1:
        y = torch.relu(y)
    return y if r is None else y + r


def abs_sum_bound(case: Dict[str, object], with_res: bool = False) -> float:
    """max over the outputs of sum |terms| + |bias| (+ |alpha * res|): no partial sum, in any order, exceeds it"""
    _, _, _, Cin, Cout, k, stride = case["shape"]
    s = taps(case["x"].double().abs(), k, stride) @ case["W"].double().abs().reshape(Cout, k * k * Cin).T + case["bias"].double().abs()
    if with_res:
        s = s + case["alpha"] * case["res"].double().abs()
    return float(s.max())


def pixel_shuffle(y: torch.Tensor) -> torch.Tensor:
    """[B,H,W,4*C] -> [B,2H,2W,C]: channel block d = 2*dy + dx goes to pixel (2y + dy, 2x + dx) (ConvTranspose2d(k=2, s=2) as four pointwise GEMMs)"""
    B, H, W, C4 = y.shape
    C = C4 // 4
    z = torch.zeros(B, 2 * H, 2 * W, C, dtype=y.dtype)
    for d in range(4):
        z[:, d // 2 :: 2, d % 2 :: 2] = y[..., d * C : (d + 1) * C]
    return z


# ----------------------------------------------------------------------------------------------------------------------
# float32 -> `bits`-significand storage, restated on the float32 bit pattern (sign | magnitude).  +-0, values below the storage's smallest normal and non-finite
# values are returned as they are; overflow to infinity is the caller's to exclude (the cases stay far below fp16's 65 504).
# ----------------------------------------------------------------------------------------------------------------------
def _parts(y: torch.Tensor, bits: int):
    assert y.dtype == torch.float32 and bits in (BF16, FP16)
    u = y.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    sign, mag = u & 0x80000000, u & 0x7FFFFFFF
    e = mag >> 23
    alone = (e < (1 if bits == BF16 else 127 - 14)) | (e == 255)
    return sign, mag, alone, 24 - bits


def _join(y: torch.Tensor, sign: torch.Tensor, mag: torch.Tensor, alone: torch.Tensor) -> torch.Tensor:
    v = sign | mag
    v = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32).reshape(y.shape)
    return torch.where(alone.reshape(y.shape), y, v)


def rne(y: torch.Tensor, bits: int) -> torch.Tensor:
    """round to nearest, ties to even: the correct store"""
    sign, mag, alone, drop = _parts(y, bits)
    mag = (mag + ((1 << (drop - 1)) - 1) + ((mag >> drop) & 1)) & ~((1 << drop) - 1)
    return _join(y, sign, mag, alone)


def truncate(y: torch.Tensor, bits: int) -> torch.Tensor:
    """the low bits dropped (towards zero)"""
    sign, mag, alone, drop = _parts(y, bits)
    return _join(y, sign, mag & ~((1 << drop) - 1), alone)


def half_away(y: torch.Tensor, bits: int) -> torch.Tensor:
    """half an ulp added to the magnitude, then truncated: ties away from zero.  On the sign-magnitude pattern this is what `(u + 0x8000) >> 16` does."""
    sign, mag, alone, drop = _parts(y, bits)
    return _join(y, sign, (mag + (1 << (drop - 1))) & ~((1 << drop) - 1), alone)


def half_up(y: torch.Tensor, bits: int) -> torch.Tensor:
    """half an ulp added to the VALUE, then rounded down: ties towards +infinity.  Positive values as half_away; a negative tie goes towards zero."""
    sign, mag, alone, drop = _parts(y, bits)
    half = 1 << (drop - 1)
    mag = torch.where(sign == 0, mag + half, mag + half - 1) & ~((1 << drop) - 1)
    return _join(y, sign, mag, alone)


WRONG_ROUNDINGS = {"truncate": truncate, "half_up": half_up, "half_away": half_away}


def classify(y: torch.Tensor, bits: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(exactly representable, exact tie between two neighbours, inexact non-tie): boolean masks over a float32 tensor"""
    _, mag, alone, drop = _parts(y, bits)
    rem = (mag & ((1 << drop) - 1)).reshape(y.shape)
    alone = alone.reshape(y.shape)
    exact = alone | (rem == 0)
    tie = ~alone & (rem == (1 << (drop - 1)))
    return exact, tie, ~exact & ~tie


def storage_bits(y: torch.Tensor, bits: int) -> torch.Tensor:
    """a float32 tensor that is representable in the storage -> its 16-bit patterns (int16), -0 and +0 apart"""
    s = y.to(torch.bfloat16 if bits == BF16 else torch.float16)
    assert torch.equal(s.float().view(torch.int32), y.contiguous().view(torch.int32)), "not representable in the storage"
    return s.view(torch.int16)


def expected(case: Dict[str, object], bits: int, act: int = 0, with_res: bool = False) -> torch.Tensor:
    """what a correct tile stores, as float32: rne(float64 reference, bits)"""
    y = reference(case, act, with_res)
    y32 = y.float()
    assert torch.equal(y32.double(), y), "the reference is not exact in fp32"
    return rne(y32, bits)
