"""Exact-arithmetic inputs for the 8-bit conv tiles (no GPU, no library): the cases of tests/conv_exact_cases.py carried over to the e4m3 and int8 variants of
csrc/conv_pp.hip.  Operands are small integers that are their own codes in every format on the path, every per-cout factor g[c] is a power of two, and the bias is
an integer in the units the accumulator counts in -- so a correct tile holds ONE fp32 value v = (sum + bias) * g[c] before its store, whatever the K order, and the
stored byte (or bf16 pattern) is one well-defined rounding of it.

    q8_link(shape, link, seed)   operands, bias, exponents e[c] (g = 2^-e) and the diagonal of one link: "i8_bf16", "i8_i8", "f8_bf16", "f8_f8", "bf16_i8", "bf16_f8"
    value(case, ...)             v in float64, before the store's clamp and rounding: act((conv + bias) * g (+ diag * x)) (+ alpha * res); seven planted faults
    store_i8 / store_f8          clamp, then round: the correct store ("rne") and the wrong ones, restated on float64
    classify_i8 / classify_f8    what the rounding step sees: (exactly representable, exact tie, inexact non-tie, clamped at the top, clamped at the bottom)
    kernel_bias / kernel_gscale / kernel_diag   the vectors vgh_conv2d takes for a link (include/vgh.h), given the packer's weight scale

tests/test_conv_q8_exact_cases_host.py checks on the CPU what makes the cases mean something; tests/test_gpu_conv_q8_exact.py feeds them to every g tile.

Weight scales the cases rely on (asserted against the packers by the host test): every int8 row carries one planted +-127, so vgh_pack_conv_weights_i8 gives
wscale = 1 and every weight is its own code; every e4m3 row's largest weight is 4, so vgh_pack_conv_weights_fp8 gives wscale = 2^-6 and the codes hold 64 * w."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch

import conv_exact_cases as cx

E4M3 = torch.float8_e4m3fn
F8_WSCALE = 2.0 ** -6  # the e4m3 packer's row scale when the row's largest weight is 4: the smallest power of two s with 4 / s <= 448
I8_MAX, F8_MAX = 127.0, 448.0
X_SPIKE = 127  # int8 inputs: about 1 code in 512 is +-127 (never -128: the format is symmetric)
SPIKE_ONE_IN = 512

# (B, H, W, Cin, Cout), all 3x3 / stride 1: the smallest shapes at which the 8-bit g tiles can go wrong
SHAPES = [
    (2, 11, 13, 64, 64),  # ragged 8x8 sub-patches, one 64-channel block
    (1, 20, 20, 192, 96),  # three 64-channel blocks, the 96-cout tile
    (2, 9, 19, 128, 256),  # two cout tiles per pixel group, the 128-cout tile
    (1, 8, 12, 512, 128),  # K = 4608, the longest K of the network
    (3, 16, 16, 256, 192),  # several images, full sub-patches
]
LINKS = ("i8_bf16", "i8_i8", "f8_bf16", "f8_f8", "bf16_i8", "bf16_f8")
BF16_IN_SHAPE = SHAPES[0]  # the bf16 -> 8-bit links run on one shape: their K loop is the bf16 tile's, held to the bit by tests/test_gpu_conv_exact.py

# ---- the tables.  v = (sum + bias[c]) * 2^-e[c]; the conv sum has standard deviation sigma(link, K) (below).
# An int8 store ties where (sum + bias) = 2^(e-1) mod 2^e and |v| < 127: a share 2^-e of the values the clamp leaves alone, so e >= 1 and 127 * 2^e around sigma;
# an e4m3 store ties by the binade of |sum + bias| alone (integers in [16, 32): every second one, [32, 64): every fourth ...), whatever e is, so the bias stays small
# against sigma and e only places the +-448 clamp at about two sigma.  Both 8-bit bias tables are fractions of sigma: a few channels pushed towards either clamp.
# bf16 stores tie from |v| = 256 * 2^-e on: cx's own bf16 bias table.
E_OFFSETS = (0, -1, 1, -2, 0, 1, -1, 0, -2, 1, 0, -1, 1, 0, -1, -2)  # e[c] = e0(link, K) + E_OFFSETS[c % 16]
BIAS_SIGMAS = (0.0, 0.5, -0.5, 1.0, -1.0, 0.25, -0.25, 1.5, -1.5, 0.125, -0.75, 0.75, 2.0, -2.0, 0.0625, -0.375)  # bias[c] = round(sigma * (BIAS_SHARE * BIAS_SIGMAS[c % 16] + BIAS_SHIFT))
# e4m3: within half a sigma, or the ties of the small binades are lost.  int8: spread over about half the clamp range 127 * 2^e0 (sigma is ~1000 behind an int8
# input and 124 behind the bf16 one).  All of them moved up by a quarter sigma, so that a ReLU leaves enough values to round.
BIAS_SHARE = {"i8_i8": 0.25, "bf16_i8": 1.5, "f8_f8": 0.25, "bf16_f8": 0.25}
BIAS_SHIFT = {"i8_i8": 0.25, "bf16_i8": 0.25, "f8_f8": 0.25, "bf16_f8": 0.25}
DIAG_TABLE = (3, -5, 1, 7, -2, 9, -1, 4, -8, 2, 6, -3, 5, -7, 8, -4)  # the bypass: dvec[c] = DIAG_TABLE[c % 16] * 2^-e[c], an integer times a power of two
FAULTS = cx.FAULTS + ("x_unsigned", "bias_real_units", "diag_next_channel", "swap_runs")


def sigma(link: str, K: int) -> float:
    """standard deviation of the conv sum: x uniform in [-3, 3] (variance 4), w uniform in [-4, 4] (20 / 3); int8 inputs add the +-127 spikes to x (127^2 / 512)
    and one +-127 weight per row"""
    if link.startswith("i8"):
        ex2 = 4.0 + X_SPIKE ** 2 / SPIKE_ONE_IN
        return float(np.sqrt(ex2 * (20.0 / 3.0 * K + 127.0 ** 2)))
    return float(np.sqrt(4.0 * 20.0 / 3.0 * K))


def e0(link: str, K: int) -> int:
    s = sigma(link, K)
    if link.endswith("_i8"):
        return max(3, int(round(np.log2(s / I8_MAX))))  # e = 1 .. 4: an int8 store of integers (e <= 0) has no ties
    if link.endswith("_f8"):
        return int(round(np.log2(2.0 * s / F8_MAX)))
    return 2  # bf16 output: the ties do not depend on e; 0 .. 3 puts four different factors into every 16-byte store


@functools.lru_cache(maxsize=None)
def _i8_operands(B: int, H: int, W: int, Cin: int, Cout: int, seed: int):
    rng = np.random.default_rng([20251020, seed, B, H, W, Cin, Cout])
    x = rng.integers(-cx.X_MAX, cx.X_MAX + 1, size=(B, H, W, Cin))
    spike = rng.integers(0, SPIKE_ONE_IN, size=x.shape) == 0
    x = np.where(spike, np.where(rng.integers(0, 2, size=x.shape) == 0, -X_SPIKE, X_SPIKE), x)
    Wt = rng.integers(-cx.W_MAX, cx.W_MAX + 1, size=(Cout, 3, 3, Cin))
    at = rng.integers(0, 9 * Cin, size=Cout)  # one planted +-127 per row, the sign alternating by row
    Wt.reshape(Cout, -1)[np.arange(Cout), at] = np.where(np.arange(Cout) % 2 == 0, 127, -127)
    res = rng.integers(-cx.RES_MAX, cx.RES_MAX + 1, size=(B, H, W, Cout))
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    return f(x), f(Wt), f(res)


@functools.lru_cache(maxsize=None)
def q8_link(shape: Tuple[int, int, int, int, int], link: str, seed: int = 0) -> Dict[str, object]:
    """x [B,H,W,Cin], W [Cout,3,3,Cin], res [B,H,W,Cout], bias [Cout]: float32 tensors that hold integers; e [Cout] int64 and g = 2^-e float32; diag [Cout] float32
    (used by the bypass runs of "i8_bf16" only).  x, W and res depend on the input format alone: the e4m3 and bf16 inputs are cx's own operands, the int8 inputs add
    the +-127 codes.  The tensors are shared between callers: do not write to them."""
    assert link in LINKS and len(shape) == 5
    B, H, W, Cin, Cout = shape
    if link.startswith("i8"):
        x, Wt, res = _i8_operands(B, H, W, Cin, Cout, seed)
    else:
        c = cx.exact_case(B, H, W, Cin, Cout, 3, 1, seed, cx.BF16)
        x, Wt, res = c["x"], c["W"], c["res"]
    K = 9 * Cin
    ch = torch.arange(Cout)
    e = e0(link, K) + torch.tensor(E_OFFSETS)[ch % 16]
    if link.endswith("bf16"):
        bias = torch.tensor(cx.BIAS_TABLE[cx.BF16], dtype=torch.float32)[ch % 16]
    else:
        bias = torch.round(sigma(link, K) * (BIAS_SHARE[link] * torch.tensor(BIAS_SIGMAS, dtype=torch.float64) + BIAS_SHIFT[link])).float()[ch % 16]
    g = torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double()).float()
    diag = torch.tensor(DIAG_TABLE, dtype=torch.float32)[ch % 16] * g
    return {"x": x, "W": Wt, "res": res, "alpha": cx.ALPHA, "bias": bias, "e": e, "g": g, "diag": diag, "shape": (B, H, W, Cin, Cout, 3, 1), "link": link}


def _codes(case: Dict[str, object], fault: Optional[str], x: Optional[torch.Tensor]) -> torch.Tensor:
    x = (case["x"] if x is None else x).double()
    if fault == "x_unsigned":  # the code -127 read as a byte without its sign: 129
        x = torch.where(x == -127.0, torch.full_like(x, 129.0), x)
    return x


def conv_sum(case: Dict[str, object], fault: Optional[str] = None, x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,H,W,Cout] float64: the convolution alone (cx.taps: explicit zero padding) of the case's input, or of `x` in its place; the faults that live in the K loop"""
    _, _, _, Cin, Cout, k, stride = case["shape"]
    A = cx.taps(_codes(case, fault, x), k, stride, shift_tap=(0, 0) if fault == "tap_shift" else None)
    Wm = case["W"].double().clone()
    if fault == "drop_channel":
        Wm[..., 1] = 0.0
    return A @ Wm.reshape(Cout, k * k * Cin).T


def value(case: Dict[str, object], act: int = 0, with_res: bool = False, diag: bool = False, fault: Optional[str] = None, x: Optional[torch.Tensor] = None,
          res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,H,W,Cout] float64, before the store: act((conv(x, W) + bias) * g (+ diag[c] * x[pixel][c])) (+ alpha * res).  fault plants one error: cx's three
    (tap_shift, drop_channel, res_before_act); x_unsigned (int8 inputs: -127 read as 129); bias_real_units (the bias added after the factor instead of before it);
    diag_next_channel (the bypass reads channel c + 1); swap_runs (the two 4-cout runs of every 8 couts trade places in the output).  x / res: other inputs in place of the case's own."""
    assert act in (0, 1) and fault in (None,) + FAULTS
    assert not diag or case["link"] == "i8_bf16"
    Cout = case["shape"][4]
    s, g = conv_sum(case, fault, x), case["g"].double()
    y = s * g + case["bias"].double() if fault == "bias_real_units" else (s + case["bias"].double()) * g
    if diag:
        assert case["shape"][3] >= Cout
        xc = _codes(case, fault, x)
        xc = xc[..., 1 : Cout + 1] if fault == "diag_next_channel" else xc[..., :Cout]
        if fault == "diag_next_channel" and xc.shape[-1] < Cout:  # (cin == cout: the last cout reads past the pixel, the next pixel's first code or zero -- taken as zero)
            xc = torch.cat([xc, torch.zeros_like(xc[..., :1])], dim=-1)
        y = y + case["diag"].double() * xc
    r = case["alpha"] * (case["res"] if res is None else res).double() if with_res else None
    if fault == "res_before_act":
        assert with_res
        y, r = y + r, None
    if act == 1:
        y = torch.relu(y)
    if r is not None:
        y = y + r
    if fault == "swap_runs":
        y = y.reshape(*y.shape[:-1], Cout // 8, 2, 4).flip(-2).reshape(y.shape)
    return y


def abs_sum_bound(case: Dict[str, object]) -> float:
    """max over the outputs of sum |terms| + |bias|, in the case's own integers: no partial sum of the accumulator, in any order, exceeds it"""
    _, _, _, Cin, Cout, k, stride = case["shape"]
    s = cx.taps(case["x"].double().abs(), k, stride) @ case["W"].double().abs().reshape(Cout, k * k * Cin).T + case["bias"].double().abs()
    return float(s.max())


def exact_f32(v: torch.Tensor) -> torch.Tensor:
    """float64 -> float32, asserting that nothing is lost: what the tile holds in a register before its store"""
    v32 = v.float()
    assert torch.equal(v32.double(), v), "the value is not exact in fp32"
    return v32


# ----------------------------------------------------------------------------------------------------------------------
# the stores, on float64 values (exact: every v here is a small multiple of a power of two).  lo: 0 under ReLU, else the format's most negative code.
# ----------------------------------------------------------------------------------------------------------------------
def _lo(act: int, hi: float) -> float:
    return 0.0 if act == 1 else -hi


def _round_half_even(q: torch.Tensor) -> torch.Tensor:
    return torch.round(q)  # torch.round: halves to the even neighbour


def _half_away(q: torch.Tensor) -> torch.Tensor:
    return torch.sign(q) * torch.floor(q.abs() + 0.5)


def store_i8(v: torch.Tensor, act: int, how: str = "rne") -> torch.Tensor:
    """int8 codes (int16 tensor) of a float64 tensor.  rne: clamp to [lo, 127], round halves to even -- the correct store.  Wrong ones: truncate, half_away
    (roundf), half_up (floor(v + 0.5)), clamp_128 (the bottom clamp at -128: visible without ReLU only)."""
    assert v.dtype == torch.float64
    lo = _lo(act, I8_MAX)
    if how == "clamp_128":
        return _round_half_even(v.clamp(0.0 if act == 1 else -128.0, I8_MAX)).to(torch.int16)
    c = v.clamp(lo, I8_MAX)
    q = {"rne": _round_half_even, "truncate": torch.trunc, "half_away": _half_away, "half_up": lambda t: torch.floor(t + 0.5)}[how](c)
    return q.to(torch.int16)


def _f8_step(c: torch.Tensor) -> torch.Tensor:
    """the spacing of e4m3 around c: 2^(floor(log2 |c|) - 3), 2^-9 below the smallest normal 2^-6"""
    ex = torch.frexp(c.abs().clamp(min=2.0 ** -6))[1] - 1  # |c| = m * 2^(ex + 1), m in [0.5, 1)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex - 3).double())


def store_f8(v: torch.Tensor, act: int, how: str = "rne") -> torch.Tensor:
    """e4m3 bytes (uint8 tensor) of a float64 tensor.  rne: clamp to [lo, 448], round to the nearest e4m3 value, halves to even -- the correct store, and torch's own
    conversion (asserted).  Wrong ones: truncate, half_away, nan_overflow (what lies beyond +-448 becomes the NaN code 0x7F / 0xFF instead of saturating)."""
    assert v.dtype == torch.float64
    lo = _lo(act, F8_MAX)
    c = v.clamp(lo, F8_MAX)
    rne = c.float().to(E4M3)
    if how == "rne":
        return rne.view(torch.uint8)
    if how == "nan_overflow":
        b = rne.view(torch.uint8).clone()
        b[v > F8_MAX] = 0x7F
        b[v < min(lo, -F8_MAX)] = 0xFF
        return b
    step = _f8_step(c)
    q = {"truncate": torch.trunc, "half_away": _half_away}[how](c / step) * step
    b = q.float().to(E4M3)
    assert torch.equal(b.float().double(), q), "a rounded value must be an e4m3 value"
    # (a value that rounds to zero keeps its sign, as the hardware convert and torch's do)
    return torch.where((q == 0) & (c < 0), torch.full_like(b.view(torch.uint8), 0x80), b.view(torch.uint8))


WRONG_STORES = {"i8": ("truncate", "half_away", "half_up", "clamp_128"), "f8": ("truncate", "half_away", "nan_overflow")}
STORE = {"i8": store_i8, "f8": store_f8}


def classify_i8(v: torch.Tensor, act: int):
    """(exact, tie, inexact, top, bottom) boolean masks: the first three partition the values by what the rounding step sees AFTER the clamp (a clamped value is
    exact); top / bottom: the clamp changed the value (v > 127, v < -127 without ReLU)"""
    c = v.clamp(_lo(act, I8_MAX), I8_MAX)
    frac = c - torch.floor(c)
    exact, tie = frac == 0.0, frac == 0.5
    return exact, tie, ~exact & ~tie, v > I8_MAX, (v < -I8_MAX) & (act == 0)


def classify_f8(v: torch.Tensor, act: int):
    c = v.clamp(_lo(act, F8_MAX), F8_MAX)
    q = c / _f8_step(c)
    frac = q - torch.floor(q)
    exact, tie = frac == 0.0, frac == 0.5
    return exact, tie, ~exact & ~tie, v > F8_MAX, (v < -F8_MAX) & (act == 0)


CLASSIFY = {"i8": classify_i8, "f8": classify_f8}


def expected(case: Dict[str, object], act: int = 0, with_res: bool = False, diag: bool = False) -> torch.Tensor:
    """what a correct tile stores: int16 codes (int8 output), uint8 bytes (e4m3 output) or float32 values that are bf16 values (bf16 output)"""
    v = value(case, act, with_res, diag)
    out = case["link"].split("_")[1]
    exact_f32(v)
    if out == "bf16":
        return cx.rne(v.float(), cx.BF16)
    assert not with_res and not diag
    return STORE[out](v, act)


# ----------------------------------------------------------------------------------------------------------------------
# what vgh_conv2d takes (include/vgh.h): the bias in accumulator units, the factor from accumulator units to output units
# ----------------------------------------------------------------------------------------------------------------------
def kernel_bias(case: Dict[str, object]) -> torch.Tensor:
    """float32 [Cout] as the library reads it.  int8 input: int32 BIT PATTERNS (the accumulator is an int32 that starts at the bias); e4m3 input: bias / unit with
    unit = wscale * s_in = 2^-6 (the accumulator counts in 64ths: codes hold 64 * w); bf16 input: the bias itself."""
    src = case["link"].split("_")[0]
    if src == "i8":
        return case["bias"].to(torch.int32).view(torch.float32)
    if src == "f8":
        return case["bias"] / F8_WSCALE
    return case["bias"].clone()


def kernel_gscale(case: Dict[str, object]) -> torch.Tensor:
    """float32 [Cout]: unit / s_out[c] with s_out[c] = 2^e[c]; unit = 1 for int8 (wscale 1, s_in 1) and bf16 inputs, 2^-6 for e4m3 inputs"""
    return case["g"] * (F8_WSCALE if case["link"].startswith("f8") else 1.0)


def kernel_diag(case: Dict[str, object]) -> torch.Tensor:
    """float32 [Cout]: the bypass vector, w[c][centre][c] * s_in in output units"""
    return case["diag"].clone()
