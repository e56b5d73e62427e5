"""TEST INFRASTRUCTURE: the NumPy restatement of the rule of include/vgh_osd.h (libvghosd.so, head_detector_amd/overlay.py): the key plane, the owner of a
plane sample, the blend.  Items are plain dicts -- ``kind`` ("bar", "rect", "text"), ``box`` (x0, y0, x1, y1), ``color`` (one byte per plane), ``alpha`` (0 .. 256)
and ``thickness`` (rect) or ``scale`` and ``codes`` (text) -- walked in order, vectorised over each item's clipped box.  Nothing of the package's ``overlay`` module
is used: the font is parsed out of csrc/osd_rules.h."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = os.path.join(ROOT, "head_detector_amd", "csrc", "osd_rules.h")
CHARS = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#%.:-+/"  # glyph code = index


def parse_font(path=RULES) -> np.ndarray:
    """uint8 [44, 7]: kFont of csrc/osd_rules.h, read from the header's text."""
    text = open(path).read()
    body = re.search(r"kFont\[VGHO_GLYPHS\]\[VGHO_GLYPH_ROWS\] = \{(.*?)\n\};", text, flags=re.S).group(1)
    rows = [[int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]{2})", line)] for line in body.splitlines() if "{" in line]
    font = np.array(rows, dtype=np.uint8)
    assert font.shape == (len(CHARS), 7), font.shape
    return font


FONT = parse_font()


def encode(string):
    """The glyph codes of a string: lower case becomes upper case, anything outside the font a space."""
    return [CHARS.index(ch) if ch in CHARS else 0 for ch in str(string).upper()]


def text_size(length, scale):
    return 6 * scale * length - scale, 7 * scale


def bar(box, color, alpha=256):
    return dict(kind="bar", box=tuple(int(v) for v in box), color=tuple(color), alpha=int(alpha))


def rect(box, color, thickness, alpha=256):
    return dict(kind="rect", box=tuple(int(v) for v in box), color=tuple(color), alpha=int(alpha), thickness=int(thickness))


def text(x, y, codes, color, scale, alpha=256):
    codes = encode(codes) if isinstance(codes, str) else [int(c) for c in codes]
    w, h = text_size(len(codes), scale)
    return dict(kind="text", box=(int(x), int(y), int(x) + w, int(y) + h), color=tuple(color), alpha=int(alpha), scale=int(scale), codes=codes)


def coverage(item, H, W, font=FONT):
    """(ys, xs, covered): the rows and columns of the item's box clipped to the target and a bool array [len(ys), len(xs)] of the positions it covers."""
    x0, y0, x1, y1 = item["box"]
    xs, ys = np.arange(max(x0, 0), min(x1, W), dtype=np.int64), np.arange(max(y0, 0), min(y1, H), dtype=np.int64)
    X, Y = xs[None, :], ys[:, None]
    if item["kind"] == "bar":
        covered = np.ones((len(ys), len(xs)), dtype=bool)
    elif item["kind"] == "rect":
        covered = np.minimum(np.minimum(X - x0, x1 - 1 - X), np.minimum(Y - y0, y1 - 1 - Y)) < item["thickness"]
    else:
        s, codes = item["scale"], np.asarray(item["codes"], dtype=np.int64)
        assert (x1 - x0, y1 - y0) == text_size(len(codes), s)
        u, v = (X - x0) // s, (Y - y0) // s
        covered = (u % 6 < 5) & (((font[codes[u // 6], v] >> np.minimum(u % 6, 7)) & 1) == 1)
    return ys, xs, np.broadcast_to(covered, (len(ys), len(xs)))


def key_plane(H, W, items, font=FONT) -> np.ndarray:
    """int64 [H, W]: 1 + the largest index of an item that covers the position, 0 where none does."""
    K = np.zeros((H, W), dtype=np.int64)
    for i, item in enumerate(items):
        ys, xs, covered = coverage(item, H, W, font)
        if covered.size:
            sub = K[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            sub[covered] = i + 1  # the items come in ascending order: the latest wins
    return K


def owner(K, shift) -> np.ndarray:
    """The owner of every sample of a plane of ``shift``: the maximum key of its (up to) 2^shift x 2^shift in-target positions, minus 1 (-1 = nobody)."""
    if shift == 0:
        return K - 1
    H, W = K.shape
    n = 1 << shift
    ph, pw = (H + n - 1) >> shift, (W + n - 1) >> shift
    padded = np.zeros((ph * n, pw * n), dtype=K.dtype)
    padded[:H, :W] = K
    return padded.reshape(ph, n, pw, n).max(axis=(1, 3)) - 1


def blend(src, c, a):
    return (np.asarray(src, dtype=np.int64) * (256 - a) + np.asarray(c, dtype=np.int64) * a + 128) >> 8


def render(planes, shifts, H, W, items, font=FONT):
    """New planes: every owned sample becomes the blend of its owner's colour (of that plane) over the SOURCE sample; every other sample stays."""
    K = key_plane(H, W, items, font)
    colors = np.array([it["color"] for it in items], dtype=np.int64).reshape(len(items), len(planes))
    alphas = np.array([it["alpha"] for it in items], dtype=np.int64)
    out = []
    for p, (plane, shift) in enumerate(zip(planes, shifts)):
        o = owner(K, shift)
        assert plane.shape == o.shape and plane.dtype == np.uint8, (plane.shape, o.shape)
        new = plane.copy()
        owned = o >= 0
        if owned.any():
            new[owned] = blend(plane[owned], colors[o[owned], p], alphas[o[owned]]).astype(np.uint8)
        out.append(new)
    return out
