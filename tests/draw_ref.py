"""CPU restatement of the three OpenCV drawing primitives behind ``PredictionResult.draw`` (head_detector/draw_utils.py of the reference):
``circle`` (filled), ``polylines`` (closed, thickness 1, 8-connected) and ``rectangle`` (thickness 2), with cv2's signatures so that this module
can stand in for cv2, plus ``render``: the painter's-order evaluation of a whole draw plan that the GPU tests compare csrc/draw.hip with.

PARITY UNPINNED against cv2 itself: the rules below are OpenCV 4.x's drawing.cpp (clipLine, the Line walk for thickness 1, FillCircle, the
thickness-2 edges of rectangle) restated in this project's words where neither cv2 nor its source was at hand.  They are the contract until
``test_draw_host.py::test_restatement_against_cv2`` (skipped without cv2) or ``tools/first_contact.py --cv2`` says otherwise.

Every primitive exists twice: a literal loop form (``*_loop``: one pixel at a time, the rule as written) and a NumPy form (closed form over
many segments at once); tests/test_draw_host.py compares the two.

The rules
  points      int32 pixel coordinates (the callers truncate toward zero)
  rectangle   thickness 2: every edge is the quad ``p +- 1 px normal`` filled inclusively (three pixels wide) plus a radius-1 filled circle (a
              five-pixel plus) at both ends.  For the four axis-aligned edges of (x, y) .. (x2, y2) the union is
              [x..x2] x [y-1..y+1]  U  [x..x2] x [y2-1..y2+1]  U  [x-1..x+1] x [y..y2]  U  [x2-1..x2+1] x [y..y2], clipped: the outer corner pixels stay unpainted.
  line        (1) clipLine to [0, W-1] x [0, H-1]: the ENDPOINTS move (a clipped line is not the visible part of the unclipped one);
              (2) a Bresenham walk from the left end: D + 1 pixels along the major axis, ``err = D - 2d``; paint; ``err < 0``: step the minor
              axis, ``err += 2D - 2d``; else ``err -= 2d``; step the major axis.  Closed form: after k major steps the minor offset is
              ``(2 k d + D - 1) // (2 D)``.
  circle      filled: rows cy + j, |j| <= R, columns cx - hw[|j|] .. cx + hw[|j|], clipped; ``half_widths(R)`` is OpenCV's midpoint loop.
"""
import numpy as np

BOX_COLOUR, WIRE_COLOUR, DOT_COLOUR = (255, 0, 0), (0, 0, 255), (255, 255, 255)
CLASS_COLOURS = (BOX_COLOUR, WIRE_COLOUR, DOT_COLOUR)  # class 0 box, 1 wire, 2 dots: the order in which one head's classes are painted


# ---- circle ------------------------------------------------------------------------------------------------------------------------------
def half_widths(radius: int) -> list:
    """hw[j], j = 0 .. R: half the width of the filled circle's row at distance j from the centre row."""
    hw = [0] * (radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def circle_loop(img, center, radius, color, thickness=-1):
    assert thickness == -1, "only the filled circle is restated"
    H, W = img.shape[:2]
    hw = half_widths(radius)
    cx, cy = int(center[0]), int(center[1])
    for j in range(-radius, radius + 1):
        for i in range(-hw[abs(j)], hw[abs(j)] + 1):
            if 0 <= cy + j < H and 0 <= cx + i < W:
                img[cy + j, cx + i] = color
    return img


def circle(img, center, radius, color, thickness=-1):
    assert thickness == -1, "only the filled circle is restated"
    H, W = img.shape[:2]
    hw = half_widths(radius)
    cx, cy = int(center[0]), int(center[1])
    for j in range(max(-radius, -cy), min(radius, H - 1 - cy) + 1):
        a, b = max(cx - hw[abs(j)], 0), min(cx + hw[abs(j)], W - 1)
        if a <= b:
            img[cy + j, a : b + 1] = color
    return img


def circles(img, centres, radius, color):
    """All filled circles of one class at once: ``centres`` int [K, 2]."""
    H, W = img.shape[:2]
    hw = half_widths(radius)
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 2)
    for j in range(-radius, radius + 1):
        for i in range(-hw[abs(j)], hw[abs(j)] + 1):
            x, y = c[:, 0] + i, c[:, 1] + j
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            img[y[ok], x[ok]] = color
    return img


# ---- line --------------------------------------------------------------------------------------------------------------------------------
def _trunc_div(num_a, num_b, den):
    """trunc(float(num_a) * num_b / den): one double product, one double division, truncation toward zero."""
    q = float(num_a) * num_b / den
    return int(q)


def clip_line_loop(W, H, p1, p2):
    """-> (drawn, (x1, y1), (x2, y2)) by the rule as written."""
    right, bottom = W - 1, H - 1
    x1, y1, x2, y2 = int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])

    def code(x, y):
        return (x < 0) + 2 * (x > right) + 4 * (y < 0) + 8 * (y > bottom)

    c1, c2 = code(x1, y1), code(x2, y2)
    if c1 & c2:
        return False, (x1, y1), (x2, y2)
    if c1 | c2:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _trunc_div(a - y1, x2 - x1, y2 - y1)
            y1 = a
            c1 = (x1 < 0) + 2 * (x1 > right)
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _trunc_div(a - y2, x1 - x2, y1 - y2)
            y2 = a
            c2 = (x2 < 0) + 2 * (x2 > right)
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _trunc_div(a - x1, y2 - y1, x2 - x1)
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _trunc_div(a - x2, y1 - y2, x1 - x2)
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def walk_loop(p1, p2):
    """The pixels of an (already clipped) segment in drawing order."""
    x1, y1, x2, y2 = int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])
    dx, dy = x2 - x1, y2 - y1
    x, y = x1, y1
    if dx < 0:
        dx, dy, x, y = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    y_major = dy > dx
    D, d = (dy, dx) if y_major else (dx, dy)
    err = D - 2 * d
    out = []
    for _ in range(D + 1):
        out.append((x, y))
        if err < 0:
            if y_major:
                x += 1
            else:
                y += sy
            err += 2 * D - 2 * d
        else:
            err -= 2 * d
        if y_major:
            y += sy
        else:
            x += 1
    return out


def line_loop(img, p1, p2, color):
    H, W = img.shape[:2]
    drawn, a, b = clip_line_loop(W, H, p1, p2)
    if drawn:
        for x, y in walk_loop(a, b):
            img[y, x] = color
    return img


def clip_lines(W, H, x1, y1, x2, y2):
    """``clip_line_loop`` on int arrays -> (drawn, x1, y1, x2, y2, moved): ``moved`` marks drawn segments with an end that was moved."""
    right, bottom = W - 1, H - 1
    x1, y1, x2, y2 = (np.array(v, dtype=np.int64) for v in (x1, y1, x2, y2))
    ox1, oy1, ox2, oy2 = x1.copy(), y1.copy(), x2.copy(), y2.copy()

    def code(x, y):
        return (x < 0) * 1 + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8

    def xcode(x):
        return (x < 0) * 1 + (x > right) * 2

    def moved_by(m, num_a, num_b, den):
        q = num_a.astype(np.float64) * num_b / np.where(m, den, 1)
        return np.where(m, np.trunc(q).astype(np.int64), 0)

    c1, c2 = code(x1, y1), code(x2, y2)
    alive = (c1 & c2) == 0
    work = alive & ((c1 | c2) != 0)
    m = work & ((c1 & 12) != 0)
    a = np.where(c1 < 8, 0, bottom)
    x1 = x1 + moved_by(m, a - y1, x2 - x1, y2 - y1)
    y1 = np.where(m, a, y1)
    c1 = np.where(m, xcode(x1), c1)
    m = work & ((c2 & 12) != 0)
    a = np.where(c2 < 8, 0, bottom)
    x2 = x2 + moved_by(m, a - y2, x1 - x2, y1 - y2)
    y2 = np.where(m, a, y2)
    c2 = np.where(m, xcode(x2), c2)
    work = work & ((c1 & c2) == 0) & ((c1 | c2) != 0)
    m = work & (c1 != 0)
    a = np.where(c1 == 1, 0, right)
    y1 = y1 + moved_by(m, a - x1, y2 - y1, x2 - x1)
    x1 = np.where(m, a, x1)
    c1 = np.where(m, 0, c1)
    m = work & (c2 != 0)
    a = np.where(c2 == 1, 0, right)
    y2 = y2 + moved_by(m, a - x2, y1 - y2, x1 - x2)
    x2 = np.where(m, a, x2)
    c2 = np.where(m, 0, c2)
    drawn = alive & ((c1 | c2) == 0)
    moved = drawn & ((x1 != ox1) | (y1 != oy1) | (x2 != ox2) | (y2 != oy2))
    return drawn, x1, y1, x2, y2, moved


def line_pixels(x1, y1, x2, y2):
    """All pixels of the (already clipped) segments, by the closed form -> (xs, ys, segment index of every pixel)."""
    x1, y1, x2, y2 = (np.asarray(v, dtype=np.int64) for v in (x1, y1, x2, y2))
    dx, dy = x2 - x1, y2 - y1
    swap = dx < 0
    sx0, sy0 = np.where(swap, x2, x1), np.where(swap, y2, y1)
    dx, dy = np.where(swap, -dx, dx), np.where(swap, -dy, dy)
    step = np.where(dy < 0, -1, 1)
    dy = np.abs(dy)
    y_major = dy > dx
    D, d = np.where(y_major, dy, dx), np.where(y_major, dx, dy)
    n = D + 1
    # per pixel: int32 while 2 k d + D - 1 fits (every segment clipped to an image of up to 32767 pixels a side does), else int64
    t = np.int32 if len(D) and int(D.max()) < 32767 else np.int64
    seg = np.repeat(np.arange(len(n), dtype=np.int32), n)
    k = np.arange(int(n.sum()), dtype=t) - np.repeat((np.cumsum(n) - n).astype(t), n)
    minor = (2 * k * d.astype(t)[seg] + np.maximum(D - 1, 0).astype(t)[seg]) // np.maximum(2 * D, 1).astype(t)[seg]  # D == 0: k == 0 -> 0
    along_x, along_y = np.where(y_major[seg], minor, k), np.where(y_major[seg], k, minor)
    return sx0.astype(t)[seg] + along_x, sy0.astype(t)[seg] + step.astype(t)[seg] * along_y, seg


def segments(img, x1, y1, x2, y2, color, max_pixels=1 << 17):
    """Many thickness-1 segments of one colour (the order among them cannot matter)."""
    H, W = img.shape[:2]
    drawn, x1, y1, x2, y2, _ = clip_lines(W, H, x1, y1, x2, y2)
    x1, y1, x2, y2 = x1[drawn], y1[drawn], x2[drawn], y2[drawn]
    if not len(x1):
        return img
    n = np.maximum(np.abs(x2 - x1), np.abs(y2 - y1)) + 1
    bins = np.cumsum(n) // max_pixels  # bounded memory: pieces of about max_pixels pixels
    for b in np.unique(bins):
        s = bins == b
        xs, ys, _ = line_pixels(x1[s], y1[s], x2[s], y2[s])
        img[ys, xs] = color
    return img


def polylines(img, pts, isClosed, color, thickness=1):
    """cv2.polylines for closed polygons of thickness 1: with p[-1] as the start, p[-1]->p[0], p[0]->p[1], ..."""
    assert isClosed and thickness == 1, "only closed polylines of thickness 1 are restated"
    for poly in pts:
        p = np.asarray(poly).reshape(-1, 2).astype(np.int64)
        q = np.roll(p, 1, axis=0)
        segments(img, q[:, 0], q[:, 1], p[:, 0], p[:, 1], color)
    return img


def polylines_loop(img, pts, isClosed, color, thickness=1):
    assert isClosed and thickness == 1
    for poly in pts:
        p = [tuple(int(v) for v in q) for q in np.asarray(poly).reshape(-1, 2)]
        p0 = p[-1]
        for q in p:
            line_loop(img, p0, q, color)
            p0 = q
    return img


# ---- rectangle ---------------------------------------------------------------------------------------------------------------------------
def _band(img, xa, xb, ya, yb, color):
    H, W = img.shape[:2]
    xa, xb, ya, yb = max(xa, 0), min(xb, W - 1), max(ya, 0), min(yb, H - 1)
    if xa <= xb and ya <= yb:
        img[ya : yb + 1, xa : xb + 1] = color


def rectangle(img, pt1, pt2, color, thickness=2):
    assert thickness == 2, "only thickness 2 is restated"
    x, y, x2, y2 = int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1])
    assert x2 >= x and y2 >= y, "pt2 is pt1 + (w, h) with w, h >= 0"
    _band(img, x, x2, y - 1, y + 1, color)
    _band(img, x, x2, y2 - 1, y2 + 1, color)
    _band(img, x - 1, x + 1, y, y2, color)
    _band(img, x2 - 1, x2 + 1, y, y2, color)
    return img


def rectangle_loop(img, pt1, pt2, color, thickness=2):
    """Where the band formula comes from: per edge the three-pixel-wide quad and a five-pixel plus at both ends, pixel by pixel."""
    assert thickness == 2
    H, W = img.shape[:2]
    x, y, x2, y2 = int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1])

    def put(px, py):
        if 0 <= px < W and 0 <= py < H:
            img[py, px] = color

    def plus(px, py):
        for ox, oy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            put(px + ox, py + oy)

    corners = [(x, y), (x2, y), (x2, y2), (x, y2)]
    for (ax, ay), (bx, by) in zip(corners, corners[1:] + corners[:1]):
        for px in range(min(ax, bx), max(ax, bx) + 1):
            for py in range(min(ay, by), max(ay, by) + 1):
                for o in (-1, 0, 1):
                    if ay == by and ax != bx:  # horizontal edge: the normal is vertical
                        put(px, py + o)
                    elif ax == bx and ay != by:
                        put(px + o, py)  # (an edge of length 0 has no quad, only its two pluses)
        plus(ax, ay)
        plus(bx, by)
    return img


# ---- a whole plan in painter's order -------------------------------------------------------------------------------------------------------
def render(image, points, boxes, triangles, indices, radius, colour_of=None, reverse=False):
    """A copy of ``image`` with every head's classes painted in order: ``points`` int [n, V, 2]; ``boxes`` int [n, 4] (x, y, w, h) or None;
    ``triangles`` int [T, 3] or None; ``indices`` int [K] or None (dots of ``radius``).  ``colour_of(head, cls)`` replaces the class colours and
    ``reverse`` paints last-to-first (then a pixel ends with its FIRST primitive's colour): what the GPU tests use to show that order matters."""
    img = np.array(image, copy=True)
    colour_of = colour_of or (lambda head, cls: CLASS_COLOURS[cls])
    jobs = []
    for h in range(len(points)):
        P = np.asarray(points[h], dtype=np.int64)
        if boxes is not None:
            jobs.append((h, 0, P))
        if triangles is not None:
            jobs.append((h, 1, P))
        if indices is not None:
            jobs.append((h, 2, P))
    for h, cls, P in (reversed(jobs) if reverse else jobs):
        colour = colour_of(h, cls)
        if cls == 0:
            x, y, w, hh = (int(v) for v in boxes[h])
            rectangle(img, (x, y), (x + w, y + hh), colour, 2)
        elif cls == 1:
            t = np.asarray(triangles, dtype=np.int64)
            a, b, c = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
            s, e = np.concatenate([c, a, b]), np.concatenate([a, b, c])
            segments(img, s[:, 0], s[:, 1], e[:, 0], e[:, 1], colour)
        else:
            circles(img, P[np.asarray(indices, dtype=np.int64)], radius, colour)
    return img
