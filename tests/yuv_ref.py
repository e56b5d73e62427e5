"""The conversion rule of include/vgh.h (vgh_yuv420_image) restated in NumPy, twice: a per-pixel loop that follows the header line by line, and a vectorised
form for whole frames.  Planes are uint8 arrays y [h, w], u and v [(h+1)//2, (w+1)//2] (any strides: pitched or interleaved views are fine);
coef = (y_offset, cy, crv, cgu, cgv, cbu).  Also: seeded frames in the memory layouts decoders produce, for the tests that need them."""
import numpy as np


def yuv_to_rgb_loop(y, u, v, coef):
    y_offset, cy, crv, cgu, cgv, cbu = (int(c) for c in coef)
    h, w = y.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    clamp8 = lambda t: min(max(t, 0), 255)  # noqa: E731
    for yy in range(h):
        for xx in range(w):
            c = int(y[yy, xx]) - y_offset
            d = int(u[yy >> 1, xx >> 1]) - 128
            e = int(v[yy >> 1, xx >> 1]) - 128
            terms = (cy * c + crv * e + 32768, cy * c + cgu * d + cgv * e + 32768, cy * c + cbu * d + 32768)
            assert all(abs(t) < 2 ** 31 for t in terms)  # the header's overflow bound
            out[yy, xx] = [clamp8(t >> 16) for t in terms]  # Python's >> floors, like the arithmetic shift
    return out


def yuv_to_rgb(y, u, v, coef):
    y_offset, cy, crv, cgu, cgv, cbu = (np.int32(c) for c in coef)
    h, w = y.shape
    c = y.astype(np.int32) - y_offset
    yi, xi = np.arange(h) >> 1, np.arange(w) >> 1
    d = u.astype(np.int32)[yi][:, xi] - 128
    e = v.astype(np.int32)[yi][:, xi] - 128
    luma = cy * c + 32768
    rgb = np.stack([luma + crv * e, luma + cgu * d + cgv * e, luma + cbu * d], axis=-1)
    assert rgb.dtype == np.int32
    return np.ascontiguousarray(np.clip(rgb >> 16, 0, 255).astype(np.uint8))


def picture(h, w, seed, saturating=False):
    """Dense planes (y, u, v) of one picture: random bytes, or only the extreme values 0 and 255."""
    g = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    draw = (lambda s: g.integers(0, 2, s, dtype=np.uint8) * np.uint8(255)) if saturating else (lambda s: g.integers(0, 256, s, dtype=np.uint8))
    return draw((h, w)), draw((ch, cw)), draw((ch, cw))


def surface(layout, y, u, v, pitch=None, extra_rows=0, seed=99):
    """One contiguous decoder surface holding the picture -> (buffer uint8 [n], pitch, uv_offset).  ``layout``: "nv12" | "nv21" (interleaved chroma rows ``pitch``
    apart) | "i420" (chroma rows ``pitch // 2`` apart, V plane behind the U plane).  The luma plane is ``h + extra_rows`` rows tall (an aligned surface height),
    so the chroma starts at uv_offset = pitch * (h + extra_rows); every byte that belongs to no sample is random."""
    h, w = y.shape
    ch, cw = u.shape
    pitch = 2 * cw if pitch is None else pitch
    assert pitch >= w and pitch >= 2 * cw
    uv_offset = pitch * (h + extra_rows)
    buf = np.random.default_rng(seed).integers(0, 256, uv_offset + pitch * ch + 8, dtype=np.uint8)
    buf[:pitch * h].reshape(h, pitch)[:, :w] = y
    if layout == "i420":
        cp = pitch // 2
        buf[uv_offset:uv_offset + cp * ch].reshape(ch, cp)[:, :cw] = u
        buf[uv_offset + cp * ch:uv_offset + 2 * cp * ch].reshape(ch, cp)[:, :cw] = v
    else:
        first, second = (u, v) if layout == "nv12" else (v, u)
        rows = buf[uv_offset:uv_offset + pitch * ch].reshape(ch, pitch)
        rows[:, 0:2 * cw:2] = first
        rows[:, 1:2 * cw:2] = second
    return buf, pitch, uv_offset
