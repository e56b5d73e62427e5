"""The rules of include/vgh_anon.h restated on the CPU: plain loops over heads, cells and taps, Python integers and int64 arrays, no float but where the header
itself names one (the margin, sigma and the Gaussian's exp).  The yardstick of csrc/anonymize.hip and of head_detector_amd/anonymize.py: it shares no code with
either -- the box, the ellipse, the cell side, the radius, the taps and the mesh bounds are all worked out here again."""
import math

import numpy as np

TAP_SUM = 65536
MAX_RADIUS = 1024


# ---- the host half ------------------------------------------------------------------------------------------------------------------------------
def geometry_box(bbox, margin):
    """(x0, y0, x1, y1), half-open and unclipped: the bbox grown by int(w * margin) and int(h * margin) on either side."""
    x, y, w, h = int(bbox[0]), int(bbox[1]), int(bbox[2]), int(bbox[3])
    mx, my = int(w * float(margin)), int(h * float(margin))
    return (x - mx, y - my, x + w + mx, y + h + my)


def mesh_box(vertices, triangles, H, W):
    """The inclusive, clipped pixel bounds of a mesh (the union of its triangles' integer boxes), made half-open; a mesh that touches no pixel gets a box with
    zero sides."""
    used = sorted({int(v) for v in np.asarray(triangles).reshape(-1)})
    if not used:
        return (0, 0, 0, 0)
    xs = [float(np.float32(vertices[v][0])) for v in used]
    ys = [float(np.float32(vertices[v][1])) for v in used]
    if not all(math.isfinite(q) for q in xs + ys):
        return (0, 0, W, H)
    x0, y0 = max(math.ceil(max(min(xs), -1.0)), 0), max(math.ceil(max(min(ys), -1.0)), 0)
    x1, y1 = min(math.floor(min(max(xs), float(W))), W - 1) + 1, min(math.floor(min(max(ys), float(H))), H - 1) + 1
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else (x0, y0, x0, y0)


def cell_side(box, cells):
    longest = max(box[2] - box[0], box[3] - box[1])
    side = longest // cells + (1 if longest % cells else 0)
    return side if side > 1 else 1


def blur_radius(box, strength):
    """(sigma, r): sigma = strength * max(Wb, Hb) in float64, r = ceil(3 sigma)."""
    sigma = float(strength) * max(box[2] - box[0], box[3] - box[1])
    return sigma, int(math.ceil(3.0 * sigma))


def taps(sigma, radius):
    """List of radius + 1 integers, the centre first: q_k = floor(65536 g_k / G + 0.5) for k >= 1, the centre takes what is left of 65536."""
    if radius == 0:
        return [TAP_SUM]
    g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(radius + 1)]
    total = g[0]
    for k in range(1, radius + 1):
        total += 2.0 * g[k]
    q = [0] + [int(math.floor(TAP_SUM * g[k] / total + 0.5)) for k in range(1, radius + 1)]
    q[0] = TAP_SUM - 2 * sum(q[1:])
    return q


# ---- the owner map ------------------------------------------------------------------------------------------------------------------------------
def in_ellipse(box, px, py):
    x0, y0, x1, y1 = (int(v) for v in box)
    wb, hb = x1 - x0, y1 - y0
    ex, ey = 2 * (int(px) - x0) + 1 - wb, 2 * (int(py) - y0) + 1 - hb
    return ex * ex * hb * hb + ey * ey * wb * wb <= wb * wb * hb * hb  # Python integers: exact


def owner_map(H, W, boxes, region):
    """int32 [H, W]: the largest i whose box ("box") or inscribed ellipse ("ellipse") contains the pixel, -1 where there is none."""
    owner = np.full((H, W), -1, dtype=np.int32)
    for i, (x0, y0, x1, y1) in enumerate(boxes):  # ascending: a later head overwrites
        for py in range(max(y0, 0), min(y1, H)):
            for px in range(max(x0, 0), min(x1, W)):
                if region == "box" or in_ellipse((x0, y0, x1, y1), px, py):
                    owner[py, px] = i
    return owner


def owned_mask(owner, i, box):
    """bool [H, W]: the pixels head i owns AND its geometry box contains (the one rule of every region)."""
    H, W = owner.shape
    x0, y0, x1, y1 = box
    inside = np.zeros((H, W), dtype=bool)
    inside[max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = True
    return (owner == i) & inside


# ---- the effects --------------------------------------------------------------------------------------------------------------------------------
def blur_image(image, t):
    """The two passes of the header over the WHOLE image for one tap table (list, centre first): uint8 [H, W, 3] in, uint8 out."""
    H, W = image.shape[:2]
    r = len(t) - 1
    src = image.astype(np.int64)
    acc = np.zeros((H, W, 3), dtype=np.int64)
    for k in range(-r, r + 1):
        cols = np.clip(np.arange(W) + k, 0, W - 1)
        acc += t[abs(k)] * src[:, cols]
    h = (acc + 128) >> 8
    assert int(h.max()) <= 65280
    acc = np.zeros((H, W, 3), dtype=np.int64)
    for k in range(-r, r + 1):
        rows = np.clip(np.arange(H) + k, 0, H - 1)
        acc += t[abs(k)] * h[rows]
    assert int(acc.max()) + (1 << 23) < (1 << 32)
    return ((acc + (1 << 23)) >> 24).astype(np.uint8)


def pixelate_into(out, image, mask, box, side):
    """Every cell of the grid anchored at the box's unclipped corner: the rounded mean of ALL its in-image pixels, written where ``mask`` holds."""
    H, W = image.shape[:2]
    x0, y0, x1, y1 = box
    for gy in range(y0, y1, side):
        for gx in range(x0, x1, side):
            ax, ay, bx, by = max(gx, 0), max(gy, 0), min(gx + side, x1, W), min(gy + side, y1, H)
            if bx <= ax or by <= ay:
                continue
            m = (bx - ax) * (by - ay)
            where = mask[ay:by, ax:bx]
            if not where.any():
                continue
            for c in range(3):
                S = int(image[ay:by, ax:bx, c].astype(np.int64).sum())
                out[ay:by, ax:bx, c][where] = (2 * S + m) // (2 * m)


def render(image, boxes, owner, method, *, cell=None, tap_tables=None, color=(0, 0, 0)):
    """uint8 [H, W, 3]: ``image`` with every head's effect on the pixels it owns inside its box.  ``owner`` int32 [H, W] (values outside [0, n) own nothing);
    ``cell`` the cell side per head (pixelate), ``tap_tables`` a list of taps per head (blur).  Every effect reads ``image`` alone."""
    image = np.asarray(image)
    out = image.copy()
    blurred = {}
    for i, box in enumerate(boxes):
        mask = owned_mask(owner, i, box)
        if not mask.any():
            continue
        if method == "fill":
            out[mask] = np.array(color, dtype=np.uint8)
        elif method == "pixelate":
            pixelate_into(out, image, mask, box, int(cell[i]))
        elif method == "blur":
            key = tuple(int(v) for v in tap_tables[i])
            if key not in blurred:
                blurred[key] = blur_image(image, list(key))
            out[mask] = blurred[key][mask]
        else:
            raise ValueError(method)
    return out
