"""The rules of include/vgh_video.h restated on the CPU.  The anonymisation rests on the restatement that is already pinned (tests/anonymize_ref.py): a plane's
expected bytes are ``anonymize_ref.render`` of the plane stacked three times, with the boxes, the owner map, the cell sides and the tap tables OF THAT PLANE;
what is new -- the chroma owner, the chroma box, the chroma cell side and radius -- is worked out here again in plain loops and Python integers, sharing no
code with head_detector_amd/video.py or csrc/yuv_anonymize.hip.  The packer is restated twice, a per-pixel loop that follows the header line by line and a
vectorised form for whole images; tests/test_yuv_anonymize_host.py holds the two equal."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_ref as ref  # noqa: E402

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}  # (Kr, Kb)


# ---- the host half ------------------------------------------------------------------------------------------------------------------------------
def chroma_box(box):
    """(x0 >> 1, y0 >> 1, (x1 + 1) >> 1, (y1 + 1) >> 1) as floor divisions of Python integers; a luma box with a zero side gets an empty chroma box."""
    x0, y0, x1, y1 = (int(v) for v in box)
    if x1 - x0 == 0 or y1 - y0 == 0:
        return (x0 // 2, y0 // 2, x0 // 2, y0 // 2)
    return (x0 // 2, y0 // 2, (x1 + 1) // 2, (y1 + 1) // 2)


def chroma_owner(owner, n):
    """int32 [(H + 1) // 2, (W + 1) // 2]: per chroma sample the maximum of the luma owners of the in-image pixels {2 cy, 2 cy + 1} x {2 cx, 2 cx + 1}, every value
    outside [0, n) counting as -1."""
    H, W = owner.shape
    out = np.full(((H + 1) // 2, (W + 1) // 2), -1, dtype=np.int32)
    for cy in range(out.shape[0]):
        for cx in range(out.shape[1]):
            best = -1
            for y in (2 * cy, 2 * cy + 1):
                for x in (2 * cx, 2 * cx + 1):
                    if y < H and x < W:
                        o = int(owner[y, x])
                        if 0 <= o < n and o > best:
                            best = o
            out[cy, cx] = best
    return out


def coefficients(matrix, full_range):
    """(y_offset, kyr, kyg, kyb, kur, kug, kub, kvr, kvg, kvb) of the issue's definition."""
    kr, kb = MATRICES[matrix]
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    kyr, kyb = int(round(65536.0 * sy * kr)), int(round(65536.0 * sy * kb))
    kyg = int(round(65536.0 * sy)) - kyr - kyb
    kub = kvr = int(round(65536.0 * sc / 2.0))
    kur = int(round(65536.0 * sc * -kr / (2.0 * (1.0 - kb))))
    kvb = int(round(65536.0 * sc * -kb / (2.0 * (1.0 - kr))))
    return (0 if full_range else 16, kyr, kyg, kyb, kur, -(kur + kub), kub, kvr, -(kvr + kvb), kvb)


def clamp8(v):
    return min(max(v, 0), 255)


def pixel_yuv(color, coef):
    """(Y, U, V) of one RGB pixel: the packer's rule with m = 1."""
    r, g, b = (int(c) for c in color)
    o, k = int(coef[0]), [int(c) for c in coef[1:]]
    return (clamp8(o + ((k[0] * r + k[1] * g + k[2] * b + 32768) >> 16)), clamp8(128 + ((k[3] * r + k[4] * g + k[5] * b + 32768) >> 16)),
            clamp8(128 + ((k[6] * r + k[7] * g + k[8] * b + 32768) >> 16)))


# ---- the anonymised frame -----------------------------------------------------------------------------------------------------------------------
def plane(P, boxes, owner, method, cell, tap_tables, c):
    """One plane as a one-channel image under the pinned restatement."""
    P = np.ascontiguousarray(P)
    return np.ascontiguousarray(ref.render(np.stack([P, P, P], -1), boxes, owner, method, cell=cell, tap_tables=tap_tables, color=(c, c, c))[..., 0])


def render_frame(y, u, v, luma_boxes, owner, method, *, luma_cell=None, chroma_cell=None, luma_taps=None, chroma_taps=None, chroma_boxes=None, color_yuv=(0, 0, 0)):
    """(Y, U, V) of the anonymised frame.  ``owner``: the LUMA owner map int32 [H, W].  ``chroma_boxes`` default to ``chroma_box`` of the luma boxes."""
    n = len(luma_boxes)
    if chroma_boxes is None:
        chroma_boxes = [chroma_box(b) for b in luma_boxes]
    oc = chroma_owner(owner, n)
    return (plane(y, luma_boxes, owner, method, luma_cell, luma_taps, color_yuv[0]), plane(u, chroma_boxes, oc, method, chroma_cell, chroma_taps, color_yuv[1]),
            plane(v, chroma_boxes, oc, method, chroma_cell, chroma_taps, color_yuv[2]))


# ---- the packer ---------------------------------------------------------------------------------------------------------------------------------
def pack_loop(image, coef):
    """(Y [H, W], U, V [(H + 1) // 2, (W + 1) // 2]) of a uint8 [H, W, 3] image: the header's rule pixel by pixel and block by block, Python integers."""
    H, W = image.shape[:2]
    o, k = int(coef[0]), [int(c) for c in coef[1:]]
    y = np.zeros((H, W), np.uint8)
    u = np.zeros(((H + 1) // 2, (W + 1) // 2), np.uint8)
    v = np.zeros_like(u)
    for yy in range(H):
        for xx in range(W):
            r, g, b = (int(c) for c in image[yy, xx])
            y[yy, xx] = clamp8(o + ((k[0] * r + k[1] * g + k[2] * b + 32768) >> 16))
    for cy in range(u.shape[0]):
        for cx in range(u.shape[1]):
            S, m = [0, 0, 0], 0
            for yy in (2 * cy, 2 * cy + 1):
                for xx in (2 * cx, 2 * cx + 1):
                    if yy < H and xx < W:
                        m += 1
                        for c in range(3):
                            S[c] += int(image[yy, xx, c])
            rm, gm, bm = ((2 * s + m) // (2 * m) for s in S)
            terms = (k[3] * rm + k[4] * gm + k[5] * bm + 32768, k[6] * rm + k[7] * gm + k[8] * bm + 32768)
            assert all(abs(t) < 2 ** 31 for t in terms)
            u[cy, cx], v[cy, cx] = clamp8(128 + (terms[0] >> 16)), clamp8(128 + (terms[1] >> 16))
    return y, u, v


def pack(image, coef):
    """``pack_loop`` vectorised (int64 arrays)."""
    H, W = image.shape[:2]
    o, k = int(coef[0]), [int(c) for c in coef[1:]]
    rgb = image.astype(np.int64)
    y = np.clip(o + ((k[0] * rgb[..., 0] + k[1] * rgb[..., 1] + k[2] * rgb[..., 2] + 32768) >> 16), 0, 255).astype(np.uint8)
    CH, CW = (H + 1) // 2, (W + 1) // 2
    padded = np.zeros((2 * CH, 2 * CW, 3), np.int64)
    padded[:H, :W] = rgb
    count = np.zeros((2 * CH, 2 * CW), np.int64)
    count[:H, :W] = 1
    S = padded.reshape(CH, 2, CW, 2, 3).sum(axis=(1, 3))
    m = count.reshape(CH, 2, CW, 2).sum(axis=(1, 3))[..., None]
    mean = (2 * S + m) // (2 * m)
    u = np.clip(128 + ((k[3] * mean[..., 0] + k[4] * mean[..., 1] + k[5] * mean[..., 2] + 32768) >> 16), 0, 255).astype(np.uint8)
    v = np.clip(128 + ((k[6] * mean[..., 0] + k[7] * mean[..., 1] + k[8] * mean[..., 2] + 32768) >> 16), 0, 255).astype(np.uint8)
    return y, u, v
