"""CPU restatement (NumPy, integers after the tables) of OpenCV's 8-bit ``cv2.warpAffine(src, M, (w, h), flags=INTER_LINEAR)`` with the default
constant-0 border, and of ``cv2.getRotationMatrix2D``: what csrc/aligned.hip is checked against, bit for bit.

The arithmetic, as imgproc/src/imgwarp.cpp does it for CV_8U (restated from memory: cv2 is not installed where this was written, so this
leaf is UNPINNED against cv2 itself -- ``tests/test_aligned_heads_host.py::test_restatement_against_cv2`` and ``tools/first_contact.py --cv2``
pin it where cv2 exists):

  * M is inverted in double:  D = M00*M11 - M01*M10;  D = D ? 1/D : 0;  A = [[M11*D, -M01*D], [-M10*D, M00*D]];  b = -A @ M[:, 2]
  * per destination column x:  adelta[x] = rint(A00 * x * 1024),  bdelta[x] = rint(A10 * x * 1024)
  * per destination row y:     X0[y] = rint((A01 * y + b0) * 1024) + 16,  Y0[y] = rint((A11 * y + b1) * 1024) + 16
    (rint = round half to even; every product and sum is a separate double operation, nothing fused)
  * X = (X0[y] + adelta[x]) >> 5,  Y likewise (arithmetic shifts of int32);  source pixel (sx, sy) = (X >> 5, Y >> 5) saturated to int16,
    fractions fx = X & 31, fy = Y & 31
  * weights 32*(32-fx)*(32-fy), 32*fx*(32-fy), 32*(32-fx)*fy, 32*fx*fy of the taps (sx, sy), (sx+1, sy), (sx, sy+1), (sx+1, sy+1): they are
    OpenCV's float table times 2^15 without any rounding and sum to 2^15, so its table fix-up never acts (the weight 2^15 of fx = fy = 0 is taken
    as such: an integer shift returns the source bytes)
  * a tap outside the source reads 0;  result = (sum + 2^14) >> 15.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

INTER_LINEAR = 1
AB_BITS, INTER_BITS = 10, 5
AB_SCALE = 1 << AB_BITS
ROUND_DELTA = AB_SCALE // (1 << INTER_BITS) // 2  # 16
HALF = 1 << 14


def getRotationMatrix2D(center, angle, scale) -> np.ndarray:
    """cv2.getRotationMatrix2D: the centre is a Point2f (float32), the angle in degrees, counter-clockwise for the image's y-down axes."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    a = float(angle) * (math.pi / 180.0)
    alpha = math.cos(a) * scale
    beta = math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(M: np.ndarray) -> Tuple[float, float, float, float, float, float]:
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0] = a11
    m[1] *= -D
    m[3] *= -D
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    return m[0], m[1], b1, m[3], m[4], b2


def _rint_i32(v: np.ndarray, stats: Optional[dict]) -> np.ndarray:
    if stats is not None and v.size:  # distance of the values that get rounded from the nearest half: the fixture generator's robustness margin
        stats["half_margin"] = min(stats.get("half_margin", np.inf), float(np.abs(np.abs(v - np.floor(v)) - 0.5).min()))
    return np.clip(np.rint(v), -2147483648, 2147483647).astype(np.int64)  # saturate_cast<int>


def warp_affine(src: np.ndarray, M: np.ndarray, dsize: Tuple[int, int], flags: int = INTER_LINEAR, region: Optional[Tuple[int, int, int, int]] = None,
                stats: Optional[dict] = None) -> np.ndarray:
    """``src`` uint8 [H, W, C]; ``dsize`` = (width, height) of the warped canvas like cv2.  ``region`` = (x0, y0, x1, y1): only that part of
    the canvas is computed and returned (the same bytes as ``warp_affine(...)[y0:y1, x0:x1]``)."""
    assert flags == INTER_LINEAR and src.dtype == np.uint8 and src.ndim == 3
    H, W = src.shape[:2]
    x0, y0, x1, y1 = (0, 0, int(dsize[0]), int(dsize[1])) if region is None else region
    assert 0 <= x0 <= x1 <= dsize[0] and 0 <= y0 <= y1 <= dsize[1]
    a00, a01, b0, a10, a11, b1 = invert_affine(M)
    xs = np.arange(x0, x1, dtype=np.float64)
    ys = np.arange(y0, y1, dtype=np.float64)
    adelta = _rint_i32(a00 * xs * AB_SCALE, stats)
    bdelta = _rint_i32(a10 * xs * AB_SCALE, stats)
    X0 = _rint_i32((a01 * ys + b0) * AB_SCALE, stats) + ROUND_DELTA
    Y0 = _rint_i32((a11 * ys + b1) * AB_SCALE, stats) + ROUND_DELTA
    X = (X0[:, None] + adelta[None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (AB_BITS - INTER_BITS)
    sx = np.clip(X >> INTER_BITS, -32768, 32767)
    sy = np.clip(Y >> INTER_BITS, -32768, 32767)
    fx = X & 31
    fy = Y & 31
    acc = np.zeros((y1 - y0, x1 - x0, src.shape[2]), dtype=np.int64)
    for dy, dx, wgt in ((0, 0, 32 * (32 - fx) * (32 - fy)), (0, 1, 32 * fx * (32 - fy)), (1, 0, 32 * (32 - fx) * fy), (1, 1, 32 * fx * fy)):
        px, py = sx + dx, sy + dy
        inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        tap = src[np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)].astype(np.int64)
        acc += tap * (wgt * inside)[:, :, None]
    return ((acc + HALF) >> 15).astype(np.uint8)


STATS: Optional[dict] = None  # set to a dict by tests/golden/make_golden_aligned.py to collect the rounding margins of warpAffine calls


# the name cv2 gives it, for the module that stands in for cv2 in tests/golden/make_golden_aligned.py
def warpAffine(src, M, dsize, flags=INTER_LINEAR):
    return warp_affine(np.ascontiguousarray(src), M, dsize, flags, stats=STATS)
