"""The rule of include/vgh_crop.h restated in NumPy: int64 positions, int32 sums, ``np.float32`` multiply then add, torch's round-to-nearest-even conversions for
the 16-bit dtypes.  A source is a uint8 array [h, w, 3]; a YUV frame is converted by tests/yuv_ref.py first (the header defines a frame's result that way).

  sums(sources, coefficients, supersample, source_index, size, fill, order)   int32 [n, S, S, 3] in the OUTPUT's channel order
  finish(sums, supersample, dtype, layout, scale, mean, std)                   the tensor as a NumPy array (16-bit dtypes: their raw uint16 patterns)
"""
import numpy as np
import torch

MAX_SUM = 255 * 1024 * 64


def sums(sources, coefficients, supersample, source_index, size, fill=(0, 0, 0), order="rgb"):
    """``fill`` is in the output's channel order, like the call's.  Every sub-sample of a head at once: positions [S K, S K] int64."""
    S, n = int(size), len(supersample)
    out = np.zeros((n, S, S, 3), np.int32)
    fill = np.array([int(v) for v in fill], np.int32)
    for k in range(n):
        K = int(supersample[k])
        img = sources[int(source_index[k])]
        if order == "bgr":
            img = img[:, :, ::-1]  # output channel c reads source channel 2 - c: the fill then lines up with it
        h, w = img.shape[:2]
        X0, XP, XQ, Y0, YP, YQ = (int(v) for v in coefficients[k])
        p = np.arange(S * K, dtype=np.int64)[None, :]
        q = np.arange(S * K, dtype=np.int64)[:, None]
        PX, PY = X0 + p * XP + q * XQ, Y0 + p * YP + q * YQ
        assert abs(X0) + S * K * (abs(XP) + abs(XQ)) < 2 ** 62 and abs(Y0) + S * K * (abs(YP) + abs(YQ)) < 2 ** 62
        sx, sy = PX >> 32, PY >> 32  # NumPy's >> on int64 floors
        fx, fy = ((PX >> 27) & 31).astype(np.int32)[..., None], ((PY >> 27) & 31).astype(np.int32)[..., None]

        def tap(x, y):
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            t = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int32)
            return np.where(inside[..., None], t, fill[None, None, :])

        value = (32 - fx) * (32 - fy) * tap(sx, sy) + fx * (32 - fy) * tap(sx + 1, sy) + (32 - fx) * fy * tap(sx, sy + 1) + fx * fy * tap(sx + 1, sy + 1)
        assert value.dtype == np.int32
        out[k] = value.reshape(S, K, S, K, 3).sum(axis=(1, 3), dtype=np.int32)  # q = i K + b, p = j K + a
    assert n == 0 or (out.min() >= 0 and out.max() <= MAX_SUM)
    return out


def coefficients_a_b(supersample, scale, mean, std):
    """a [n, 3] and b [3] float32: formed in float64, rounded once."""
    d = 1024.0 * np.asarray(supersample, np.float64) ** 2
    a = (float(scale) / (d[:, None] * np.asarray(std, np.float64)[None, :])).astype(np.float32)
    b = (-np.asarray(mean, np.float64) / np.asarray(std, np.float64)).astype(np.float32)
    return a, b


def finish(s, supersample, dtype, layout, scale=1 / 255, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """``dtype``: "uint8", "float32", "float16" or "bfloat16" -> [n, 3, S, S] ("nchw") or [n, S, S, 3] ("nhwc"); uint16 bit patterns for the 16-bit dtypes."""
    K = np.asarray(supersample, np.int64)
    if dtype == "uint8":
        d = (1024 * K * K)[:, None, None, None]
        y = ((2 * s.astype(np.int64) + d) // (2 * d)).astype(np.uint8)
    else:
        a, b = coefficients_a_b(supersample, scale, mean, std)
        y = s.astype(np.float32)  # exact: every sum is below 2^24
        assert np.array_equal(y.astype(np.int32), s)
        y = y * a[:, None, None, :]  # one float32 operation ...
        y = y + b[None, None, None, :]  # ... and another
        assert y.dtype == np.float32
        if dtype == "float16":
            y = torch.from_numpy(y).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
        elif dtype == "bfloat16":
            y = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return np.ascontiguousarray(y.transpose(0, 3, 1, 2)) if layout == "nchw" else y


def raw(t: torch.Tensor) -> np.ndarray:
    """A result tensor as the array ``finish`` returns: the 16-bit dtypes as their bit patterns."""
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()
