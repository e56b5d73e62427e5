"""The conversion rule of include/vgh.h for deep frames (vgh_yuv420p16_image) restated in NumPy, twice: a per-pixel loop that follows the header line by line,
and a vectorised form for whole frames.  Planes are uint16 arrays of WORDS, y [h, w], u and v [(h+1)//2, (w+1)//2] (any strides); ``bit_depth`` D is 10 or 12,
``shift`` says where the D significant bits lie in the word; coef = (y_offset, cy, crv, cgu, cgv, cbu), scaled by 2^(D+8).  ``coefficients`` restates the
coefficient formulas from the (Kr, Kb) table.  Also: seeded frames in the memory layouts decoders produce.  Shares no code with head_detector_amd/video.py."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def coefficients(matrix, full_range, bit_depth):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        y_offset, sy, sc = 0, 255.0 / (2 ** bit_depth - 1), 255.0 / (2 ** bit_depth - 1)
    else:
        y_offset, sy, sc = 16 * 2 ** (bit_depth - 8), 255.0 / (219.0 * 2 ** (bit_depth - 8)), 255.0 / (224.0 * 2 ** (bit_depth - 8))
    one = float(2 ** (bit_depth + 8))
    return (y_offset, int(round(one * sy)), int(round(one * sc * 2.0 * (1.0 - kr))), int(round(one * sc * -2.0 * kb * (1.0 - kb) / kg)),
            int(round(one * sc * -2.0 * kr * (1.0 - kr) / kg)), int(round(one * sc * 2.0 * (1.0 - kb))))


def yuv16_to_rgb_loop(y, u, v, coef, bit_depth, shift):
    y_offset, cy, crv, cgu, cgv, cbu = (int(c) for c in coef)
    D = int(bit_depth)
    mask, half, rnd = 2 ** D - 1, 2 ** (D - 1), 2 ** (D + 7)
    h, w = y.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    clamp8 = lambda t: min(max(t, 0), 255)  # noqa: E731
    for yy in range(h):
        for xx in range(w):
            c = ((int(y[yy, xx]) >> shift) & mask) - y_offset
            d = ((int(u[yy >> 1, xx >> 1]) >> shift) & mask) - half
            e = ((int(v[yy >> 1, xx >> 1]) >> shift) & mask) - half
            terms = (cy * c + crv * e + rnd, cy * c + cgu * d + cgv * e + rnd, cy * c + cbu * d + rnd)
            assert all(abs(t) < 2 ** 31 for t in terms)  # the header's overflow bound
            out[yy, xx] = [clamp8(t >> (D + 8)) for t in terms]  # Python's >> floors, like the arithmetic shift
    return out


def yuv16_to_rgb(y, u, v, coef, bit_depth, shift):
    assert y.dtype == u.dtype == v.dtype == np.uint16
    y_offset, cy, crv, cgu, cgv, cbu = (np.int32(c) for c in coef)
    D = int(bit_depth)
    mask, half, rnd = np.int32(2 ** D - 1), np.int32(2 ** (D - 1)), np.int32(2 ** (D + 7))
    sample = lambda p: (p.astype(np.int32) >> shift) & mask  # noqa: E731
    h, w = y.shape
    c = sample(y) - y_offset
    yi, xi = np.arange(h) >> 1, np.arange(w) >> 1
    d = sample(u)[yi][:, xi] - half
    e = sample(v)[yi][:, xi] - half
    luma = cy * c + rnd
    rgb = np.stack([luma + crv * e, luma + cgu * d + cgv * e, luma + cbu * d], axis=-1)
    assert rgb.dtype == np.int32
    return np.ascontiguousarray(np.clip(rgb >> (D + 8), 0, 255).astype(np.uint8))


def picture16(h, w, seed, bit_depth=10, saturating=False, shift=0):
    """Dense word planes (y, u, v) of one picture: random D-bit samples, or only the extreme values 0 and 2^D - 1, placed at ``shift`` -- and random garbage in
    every bit of the word that is not a sample bit (a decoder promises nothing about them)."""
    g = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    top = 2 ** bit_depth - 1
    keep = np.uint16(top << shift)

    def draw(s):
        sample = g.integers(0, 2, s, dtype=np.uint16) * np.uint16(top) if saturating else g.integers(0, top + 1, s, dtype=np.uint16)
        garbage = g.integers(0, 65536, s, dtype=np.uint16) & ~keep
        return (sample << np.uint16(shift)) | garbage

    return draw((h, w)), draw((ch, cw)), draw((ch, cw))


def surface16(layout, y, u, v, pitch=None, extra_rows=0, seed=99):
    """One contiguous decoder surface holding the word planes -> (buffer uint8 [n], pitch, uv_offset), both in BYTES.  ``layout``: "p010" (interleaved (U, V) word
    pairs, chroma rows ``pitch`` apart) | "i010" (chroma rows ``pitch // 2`` apart, V plane behind the U plane).  The luma plane is ``h + extra_rows`` rows tall,
    so the chroma starts at uv_offset = pitch * (h + extra_rows); every byte that belongs to no sample is a random sentinel.  Little-endian words."""
    h, w = y.shape
    ch, cw = u.shape
    pitch = 4 * cw if pitch is None else pitch
    assert pitch % 4 == 0 and pitch >= 2 * w and pitch >= 4 * cw
    uv_offset = pitch * (h + extra_rows)
    buf = np.random.default_rng(seed).integers(0, 256, uv_offset + pitch * ch + 8, dtype=np.uint8)
    words = buf.view("<u2")
    pw = pitch // 2
    words[:pw * h].reshape(h, pw)[:, :w] = y
    at = uv_offset // 2
    if layout == "i010":
        cp = pitch // 4
        words[at:at + cp * ch].reshape(ch, cp)[:, :cw] = u
        words[at + cp * ch:at + 2 * cp * ch].reshape(ch, cp)[:, :cw] = v
    else:
        assert layout == "p010"
        rows = words[at:at + pw * ch].reshape(ch, pw)
        rows[:, 0:2 * cw:2] = u
        rows[:, 1:2 * cw:2] = v
    return buf, pitch, uv_offset
