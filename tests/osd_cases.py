"""TEST INFRASTRUCTURE: the planted cases of the on-screen display (include/vgh_osd.h, libvghosd.so) and the surfaces they are drawn on.  A case is a target
size and a list of items in the form of tests/osd_ref.py (colours are PLANE bytes here, one per plane: the same three bytes serve a YUV frame and an RGB image);
a surface is one buffer of random bytes in which the planes of a layout ("nv12", "nv21", "i420", "rgb"; pitched or dense) lie, so that every byte between a row's
last sample and the pitch, every spare row and the tail are sentinels that must survive.  Nothing here uses the package's ``overlay`` module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import osd_ref as ref  # noqa: E402

LAYOUTS = ("nv12", "nv21", "i420", "rgb")
ALPHAS = (0, 1, 128, 255, 256)


# ---- surfaces -------------------------------------------------------------------------------------------------------------------------------------------
def geometry(shape, layout, pitched):
    """dict(size, planes): the byte size of the surface and, per plane, dict(offset, pitch, step, shift, h, w)."""
    h, w = shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if layout == "rgb":
        pitch, lead = (3 * w + 11, 5) if pitched else (3 * w, 0)  # a pitched image starts off a dword
        planes = [dict(offset=lead + c, pitch=pitch, step=3, shift=0, h=h, w=w) for c in range(3)]
        return dict(size=lead + pitch * h + 8, planes=planes)
    pitch, extra = (2 * cw + 10, 3) if pitched else (2 * cw, 0)
    uv = pitch * (h + extra)
    luma = dict(offset=0, pitch=pitch, step=1, shift=0, h=h, w=w)
    if layout == "i420":
        cp = pitch // 2
        chroma = [dict(offset=uv + k * cp * ch, pitch=cp, step=1, shift=1, h=ch, w=cw) for k in range(2)]
    else:
        first = [dict(offset=uv + k, pitch=pitch, step=2, shift=1, h=ch, w=cw) for k in range(2)]
        chroma = first if layout == "nv12" else first[::-1]  # planes are (Y, U, V) by meaning: NV21 stores V first
    return dict(size=uv + pitch * ch + 8, planes=[luma] + chroma)


def views(buffer, geom):
    """The planes of a surface as strided views of its NumPy buffer."""
    return [np.lib.stride_tricks.as_strided(buffer[p["offset"]:], (p["h"], p["w"]), (p["pitch"], p["step"])) for p in geom["planes"]]


def shifts(layout):
    return (0, 0, 0) if layout == "rgb" else (0, 1, 1)


def content(shape, layout, seed):
    """The dense planes of a case's picture: they depend on the KIND of target (three full planes, or one full and two half planes), not on the layout."""
    g = np.random.default_rng(seed)
    h, w = shape
    return [g.integers(0, 256, ((h + (1 << s) - 1) >> s, (w + (1 << s) - 1) >> s), dtype=np.uint8) for s in shifts(layout)]


def surface(shape, layout, pitched, planes, seed):
    """(buffer, geom): a surface of random bytes that holds ``planes``."""
    geom = geometry(shape, layout, pitched)
    buffer = np.random.default_rng(seed + 1000).integers(0, 256, geom["size"], dtype=np.uint8)
    for view, plane in zip(views(buffer, geom), planes):
        view[...] = plane
    return buffer, geom


# ---- item sets ------------------------------------------------------------------------------------------------------------------------------------------
def _colour(k):
    return ((37 * k + 11) % 256, (91 * k + 200) % 256, (53 * k + 77) % 256)


def _edges(h, w):
    boxes = [(-9, -7, 6, 5), (w - 6, -7, w + 9, 5), (-9, h - 5, 6, h + 7), (w - 6, h - 5, w + 9, h + 7),  # the four corners
             (w // 2 - 5, -11, w // 2 + 6, 4), (w // 2 - 5, h - 4, w // 2 + 6, h + 11), (-11, h // 2 - 3, 4, h // 2 + 4), (w - 4, h // 2 - 3, w + 11, h // 2 + 4),  # the edges
             (-40, -40, -3, -3), (w, 0, w + 20, h), (0, h, w, h + 1), (-(1 << 23), 3, -(1 << 23) + 9, 9), (3, 1 << 23, 9, (1 << 23) + 9),  # wholly outside
             (20, 20, 20, 40), (20, 20, 40, 20), (7, 7, 7, 7),  # a zero side
             (-5, -5, w + 5, h + 5)]  # all of it, under ...
    items = [ref.bar(boxes[-1], _colour(0), 77)]
    items += [ref.bar(b, _colour(k + 1), ALPHAS[k % 5]) if k % 2 else ref.rect(b, _colour(k + 1), 2, ALPHAS[(k + 3) % 5]) for k, b in enumerate(boxes[:-1])]
    return items


def _odd(h, w):
    """x0, y0, x1, y1 odd or even in all sixteen combinations, apart from each other: the keys a chroma sample reads beyond an odd edge belong to nobody."""
    items = []
    for k in range(16):
        bx, by = 4 + (k % 4) * (w // 4), 4 + (k // 4) * (h // 4)
        sx, sy = max(2, w // 4 - 12), max(2, h // 4 - 10)
        box = (bx + (k & 1), by + (k >> 1 & 1), bx + sx + (k >> 2 & 1), by + sy + (k >> 3 & 1))
        items.append(ref.bar(box, _colour(k), 256) if k % 3 else ref.rect(box, _colour(k), 1 + k % 2, 200))
    return items


def _rects(h, w):
    return [ref.rect((3, 3, 43, 33), _colour(1), 1), ref.rect((50, 5, 90, 35), _colour(2), 15), ref.rect((50, 40, 91, 71), _colour(3), 15, 128),  # 1; half the shorter side
            ref.rect((5, 40, 45, 60), _colour(4), 10), ref.rect((95, 10, 125, 22), _colour(5), 40, 255), ref.rect((100, 50, 101, 51), _colour(6), 1),  # half; larger; a pixel
            ref.rect((3, 70, 8, 74), _colour(7), 1), ref.rect((-6, 80, 60, 120), _colour(8), 3, 128), ref.rect((11, 77, 40, 78), _colour(9), 5)]


def _stack(h, w):
    """Overlapping items of every alpha: the topmost is blended against the source only; the transparent one on top still owns its pixels."""
    items = [ref.bar((5 + 6 * k, 5 + 4 * k, 65 + 6 * k, 45 + 4 * k), _colour(k), a) for k, a in enumerate(ALPHAS)]
    items += [ref.rect((1 + 7 * k, 30 + 3 * k, 80 + 2 * k, 90 - 2 * k), _colour(9 + k), 3, a) for k, a in enumerate(ALPHAS[::-1])]
    items.append(ref.bar((20, 20, 61, 51), _colour(20), 0))  # fully transparent, on top: the source shows through, not the items below
    items.append(ref.text(23, 23, "A0", _colour(21), 2, 128))
    return items


def _text(h, w):
    items = [ref.text(0, 1, list(range(0, 22)), _colour(1), 1), ref.text(0, 9, list(range(22, 44)), _colour(2), 1, 128),  # every glyph of the font once
             ref.text(2, 18, "#7 93%", _colour(3), 2), ref.text(1, 34, "ID:4+/-.", _colour(4), 3, 255), ref.text(37, 0, "K", _colour(5), 16, 200),  # scales 2, 3 and 16
             ref.text(-50, 60, [(3 * k + 1) % 44 for k in range(64)], _colour(6), 1), ref.text(3, 70, [(5 * k + 2) % 44 for k in range(64)], _colour(7), 2, 77)]  # 64 codes
    # runs clipped by each edge (and a corner), and one wholly outside
    items += [ref.text(-7, 50, "LEFT", _colour(8), 2), ref.text(w - 20, 45, "RIGHT", _colour(9), 2), ref.text(60, -5, "TOP", _colour(10), 2),
              ref.text(70, h - 9, "BOTTOM", _colour(11), 2), ref.text(w - 11, h - 10, "XY", _colour(12), 3), ref.text(w + 1, 5, "OUT", _colour(13), 1)]
    return items


def labelled_heads(h, w, n, seed):
    """n heads as a tracker's picture has them: a box, a label bar and its text each (3 n items)."""
    g = np.random.default_rng(seed)
    items = []
    for k in range(n):
        x, y, bw, bh = int(g.integers(-8, w)), int(g.integers(-8, h)), int(g.integers(1, 30)), int(g.integers(1, 30))
        label = f"#{k} {int(g.integers(0, 101))}%"
        tw, th = ref.text_size(len(label), 1)
        by = y - (th + 2) if y - (th + 2) >= 0 else y
        items += [ref.rect((x, y, x + bw, y + bh), _colour(k), 1 + k % 2, ALPHAS[1 + k % 4]), ref.bar((x, by, x + tw + 2, by + th + 2), _colour(k), 256),
                  ref.text(x + 1, by + 1, label, _colour(k + 100), 1, ALPHAS[2 + k % 3])]
    return items


def _tiny(h, w):
    return [ref.bar((0, 0, 1, 1), _colour(1), 128), ref.rect((-1, -1, 3, 3), _colour(2), 1, 256), ref.bar((1, 1, 2, 2), _colour(3), 255), ref.text(-2, -3, "8", _colour(4), 1)]


def cases():
    """name -> dict(shape, items, seed)."""
    out = {}
    big = (97, 131)  # odd: the last chroma row and column serve one luma row and column
    for k, (name, make) in enumerate((("edges", _edges), ("odd", _odd), ("rects", _rects), ("stack", _stack), ("text", _text))):
        out[name] = dict(shape=big, items=make(*big), seed=10 + k)
    out["edges_64"] = dict(shape=(64, 64), items=_edges(64, 64), seed=20)
    out["odd_64"] = dict(shape=(64, 64), items=_odd(64, 64), seed=21)
    out["many_heads"] = dict(shape=(64, 64), items=labelled_heads(64, 64, 300, 5), seed=22)
    out["no_items"] = dict(shape=big, items=[], seed=23)
    out["no_items_64"] = dict(shape=(64, 64), items=[], seed=24)
    out["tiny_2x2"] = dict(shape=(2, 2), items=_tiny(2, 2), seed=25)
    out["tiny_1x1"] = dict(shape=(1, 1), items=_tiny(1, 1), seed=26)
    out["outside_only"] = dict(shape=(64, 64), items=[ref.bar((-30, -30, -1, -1), _colour(1)), ref.text(70, 70, "NO", _colour(2), 2)], seed=27)
    return out


_EXPECTED = {}


def expected(name, case, layout):
    """(source planes, expected planes) of a case on a target of ``layout``'s kind; computed once and shared: treat them as read-only."""
    kind = "rgb" if layout == "rgb" else "yuv"
    if (name, kind) not in _EXPECTED:
        h, w = case["shape"]
        src = content(case["shape"], layout, case["seed"])
        _EXPECTED[(name, kind)] = (src, ref.render(src, shifts(layout), h, w, case["items"]))
    return _EXPECTED[(name, kind)]


# ---- the C arrays of a case, made here and not by the package -----------------------------------------------------------------------------------------
KINDS = {"bar": 0, "rect": 1, "text": 2}


def c_arrays(items, item_dtype):
    """(rows, codes): the ``vgho_item`` rows (``item_dtype`` = the binding's) and the uint8 glyph codes of ref items."""
    rows = np.zeros(len(items), item_dtype)
    codes = []
    for k, it in enumerate(items):
        r = rows[k]
        r["kind"] = KINDS[it["kind"]]
        r["x0"], r["y0"], r["x1"], r["y1"] = it["box"]
        r["alpha"], r["color"] = it["alpha"], it["color"]
        if it["kind"] == "rect":
            r["thickness"] = it["thickness"]
        if it["kind"] == "text":
            r["scale"], r["code_offset"], r["length"] = it["scale"], len(codes), len(it["codes"])
            codes += it["codes"]
    return rows, np.array(codes, dtype=np.uint8)
