"""NumPy restatement of the cross-tile merge rule of sliced detection (include/vgh_merge.h), in two forms -- ``merge_loop``, literal, one scalar
float32 operation at a time, and ``merge_vec``, one vector operation per kept candidate -- and a generator of planted families for the tests.  Not a test module.

The rule in short: candidate (t, r) exists iff r < counts[t]; clip to [0, S] with fmin(fmax(.)); drop it (status 2) if it comes within border * scale of an
interior edge of its tile's content rectangle (strict comparisons); image coordinates ((c - pad) / scale) + off; order by descending score bits (total order),
ties by ascending index; greedy walk in which only an earlier KEPT candidate of ANOTHER tile suppresses (status 3); the first max_heads kept are emitted
(status 1), later kept ones get status 4.  Every operation is float32, rounded on its own."""
import numpy as np

from head_detector_amd.sliced import SlicePlan, plan_slices

F = np.float32
ABSENT, KEPT, TRUNCATED, SUPPRESSED, OVER_CAP = range(5)


def order_key(score_bits: np.ndarray) -> np.ndarray:
    """uint32 score bits -> uint32 u, larger u = earlier: the total order of the bit patterns."""
    b = score_bits.astype(np.uint32)
    return b ^ np.where(b & np.uint32(0x80000000), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def _empty(max_heads, n_status):
    return dict(head_row=np.full(max_heads, -1, np.int32), head_tile=np.full(max_heads, -1, np.int32), boxes_full=np.zeros((max_heads, 4), F),
                scores=np.zeros(max_heads, F), n_heads=np.zeros(1, np.int32), n_kept_uncapped=np.zeros(1, np.int32), status=np.zeros(n_status, np.uint8))


def _match_scalar(a, b, thr, metric):
    area_a, area_b = F(F(a[2] - a[0]) * F(a[3] - a[1])), F(F(b[2] - b[0]) * F(b[3] - b[1]))
    xx1, yy1 = np.fmax(a[0], b[0]), np.fmax(a[1], b[1])
    xx2, yy2 = np.fmin(a[2], b[2]), np.fmin(a[3], b[3])
    w, h = np.fmax(F(0), F(xx2 - xx1)), np.fmax(F(0), F(yy2 - yy1))
    inter = F(w * h)
    den = F(F(area_a + area_b) - inter) if metric == "iou" else np.fmin(area_a, area_b)
    return bool(F(inter / den) > thr)  # False for NaN


def merge_loop(boxes, scores, counts, plan: SlicePlan, border=2.0, match_thr=0.5, metric="iou", max_heads=1000):
    """The rule, literally.  boxes [T, K, 4], scores [T, K] float32, counts [T] -> dict of the outputs of vghm_merge_tiles."""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    T, K = scores.shape
    S, border, thr = F(plan.image_size), F(border), F(match_thr)
    out = _empty(max_heads, T * K)
    live = []  # (-(u), index, tile, box in image coordinates)
    with np.errstate(all="ignore"):
        for t in range(T):
            off_x, off_y, _, _, pad_x, pad_y, new_w, new_h = (int(v) for v in plan.tiles[t])
            scale, interior = F(plan.scale[t]), int(plan.interior[t])
            bs = F(border * scale)
            for r in range(K):
                if r >= counts[t]:
                    continue
                i = t * K + r
                c = [np.fmin(np.fmax(v, F(0)), S) for v in boxes[t, r]]
                cut = (interior & 1 and c[0] < F(F(pad_x) + bs)) or (interior & 2 and c[1] < F(F(pad_y) + bs)) or \
                      (interior & 4 and c[2] > F(F(pad_x + new_w) - bs)) or (interior & 8 and c[3] > F(F(pad_y + new_h) - bs))
                if cut:
                    out["status"][i] = TRUNCATED
                    continue
                f = np.array([F(F(F(c[0] - F(pad_x)) / scale) + F(off_x)), F(F(F(c[1] - F(pad_y)) / scale) + F(off_y)),
                              F(F(F(c[2] - F(pad_x)) / scale) + F(off_x)), F(F(F(c[3] - F(pad_y)) / scale) + F(off_y))], F)
                u = int(order_key(scores[t, r:r + 1].view(np.uint32))[0])
                live.append((-u, i, t, f))
        live.sort(key=lambda e: (e[0], e[1]))
        kept = []
        for _, i, t, f in live:
            if any(kt != t and _match_scalar(kf, f, thr, metric) for _, kt, kf in kept):
                out["status"][i] = SUPPRESSED
                continue
            if len(kept) < max_heads:
                p = len(kept)
                out["head_row"][p], out["head_tile"][p], out["boxes_full"][p], out["scores"][p] = i, t, f, scores[t, i - t * K]
                out["status"][i] = KEPT
            else:
                out["status"][i] = OVER_CAP
            kept.append((i, t, f))
    out["n_kept_uncapped"][0] = len(kept)
    out["n_heads"][0] = min(len(kept), max_heads)
    return out


def merge_vec(boxes, scores, counts, plan: SlicePlan, border=2.0, match_thr=0.5, metric="iou", max_heads=1000):
    """The same rule with array operations (what the GPU tests compare against at thousands of candidates)."""
    boxes, scores, counts = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(counts)
    T, K = scores.shape
    S, border, thr = F(plan.image_size), F(border), F(match_thr)
    out = _empty(max_heads, T * K)
    tiles = plan.tiles.astype(np.int64)
    tile_of = np.repeat(np.arange(T), K)
    exists = (np.tile(np.arange(K), T) < np.repeat(counts, K))
    g = tiles[tile_of]
    scale, interior = plan.scale.astype(F)[tile_of], plan.interior.astype(np.int64)[tile_of]
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(boxes.reshape(-1, 4), F(0)), S)
        bs = (border * scale).astype(F)
        px, py = g[:, 4].astype(F), g[:, 5].astype(F)
        cut = ((interior & 1) != 0) & (c[:, 0] < px + bs) | ((interior & 2) != 0) & (c[:, 1] < py + bs) | \
              ((interior & 4) != 0) & (c[:, 2] > (g[:, 4] + g[:, 6]).astype(F) - bs) | ((interior & 8) != 0) & (c[:, 3] > (g[:, 5] + g[:, 7]).astype(F) - bs)
        pad = np.stack([px, py, px, py], 1)
        off = np.stack([g[:, 0], g[:, 1], g[:, 0], g[:, 1]], 1).astype(F)
        f = (((c - pad) / scale[:, None]).astype(F) + off).astype(F)
        out["status"][exists & cut] = TRUNCATED
        idx = np.flatnonzero(exists & ~cut)
        u = order_key(scores.reshape(-1).view(np.uint32)[idx]).astype(np.int64)
        idx = idx[np.lexsort((idx, -u))]
        b, tl = f[idx], tile_of[idx]
        area = ((b[:, 2] - b[:, 0]).astype(F) * (b[:, 3] - b[:, 1]).astype(F)).astype(F)
        removed = np.zeros(len(idx), bool)
        n_kept = 0
        for p in range(len(idx)):
            i = idx[p]
            if removed[p]:
                out["status"][i] = SUPPRESSED
                continue
            if n_kept < max_heads:
                out["head_row"][n_kept], out["head_tile"][n_kept], out["boxes_full"][n_kept], out["scores"][n_kept] = i, tl[p], b[p], scores.reshape(-1)[i]
                out["status"][i] = KEPT
            else:
                out["status"][i] = OVER_CAP
            n_kept += 1
            rest = b[p + 1:]
            w = np.fmax(F(0), (np.fmin(b[p, 2], rest[:, 2]) - np.fmax(b[p, 0], rest[:, 0])).astype(F))
            h = np.fmax(F(0), (np.fmin(b[p, 3], rest[:, 3]) - np.fmax(b[p, 1], rest[:, 1])).astype(F))
            inter = (w * h).astype(F)
            den = ((area[p] + area[p + 1:]).astype(F) - inter).astype(F) if metric == "iou" else np.fmin(area[p], area[p + 1:])
            removed[p + 1:] |= ((inter / den).astype(F) > thr) & (tl[p + 1:] != tl[p])
    out["n_kept_uncapped"][0] = n_kept
    out["n_heads"][0] = min(n_kept, max_heads)
    return out


OUTPUTS = ("head_row", "head_tile", "boxes_full", "scores", "n_heads", "n_kept_uncapped", "status")


def same_bytes(a: dict, b: dict):
    """None if every output of the two results is bytewise equal, else the name of the first that differs."""
    for k in OUTPUTS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


# ---- planted families -----------------------------------------------------------------------------------------------------------------------------------
def small_plan() -> SlicePlan:
    """100 x 100 image, S = 64, 25 % overlap: tile 0 the whole image (scale 0.64), tiles 1 .. 4 of 64 x 64 at scale 1 at offsets (0, 0), (36, 0), (0, 36),
    (36, 36).  At scale 1 with pad 0 a tile's padded coordinates are image coordinates minus the offset, exactly."""
    plan = plan_slices(100, 100, 64)
    assert plan.tiles[:, :2].tolist() == [[0, 0], [0, 0], [36, 0], [0, 36], [36, 36]] and plan.interior.tolist() == [0, 4 | 8, 1 | 8, 4 | 2, 1 | 2]
    return plan


def from_entries(plan: SlicePlan, keep_k: int, entries, padded=False):
    """entries: (tile, box, score), the box in image coordinates (``padded``: in the tile's padded space) -> (boxes, scores, counts), filled in the order given."""
    T = plan.n_tiles
    boxes, scores, counts = np.zeros((T, keep_k, 4), F), np.zeros((T, keep_k), F), np.zeros(T, np.int32)
    for t, box, score in entries:
        box = np.asarray(box, np.float64)
        if not padded:
            x, y, _, _, px, py, _, _ = plan.tiles[t]
            s = float(plan.scale[t])
            box = (box - [x, y, x, y]) * s + [px, py, px, py]
        boxes[t, counts[t]], scores[t, counts[t]] = box, score
        counts[t] += 1
    return boxes, scores, counts


def planted_cases():
    """name -> dict(boxes, scores, counts, plan, kwargs, expect): ``expect`` = the statuses of the existing candidates in entry order (None where the case only
    needs the comparison), ``must_have`` = statuses the case is there to produce."""
    plan, cases = small_plan(), {}

    def add(name, entries, expect=None, must_have=(), padded=False, keep_k=4, **kwargs):
        boxes, scores, counts = from_entries(plan, keep_k, entries, padded)
        at, rows = np.zeros(plan.n_tiles, int), []
        for t, _, _ in entries:
            rows.append(t * keep_k + at[t])
            at[t] += 1
        cases[name] = dict(boxes=boxes, scores=scores, counts=counts, plan=plan, kwargs=kwargs, rows=rows, expect=expect, must_have=set(must_have))

    A, B, C = (40, 38, 56, 54), (44, 38, 60, 54), (48, 38, 64, 54)  # IoU(A, B) = IoU(B, C) = 0.6, IoU(A, C) = 1 / 3
    # A kills B; B would have killed C, but B is not kept: C stays.  A mask-only shortcut (any earlier match removes) gets this wrong
    add("chain", [(1, A, 0.9), (2, B, 0.8), (4, C, 0.7)], [1, 3, 1], (1, 3))
    add("chain_longer", [(1, A, 0.9), (2, B, 0.8), (4, C, 0.7), (2, (52, 38, 68, 54), 0.6)], [1, 3, 1, 3], (1, 3))
    add("same_tile_pair", [(1, A, 0.9), (1, B, 0.8)], [1, 1], (1,))
    add("equal_scores_identical_boxes", [(2, A, 0.5), (1, A, 0.5), (4, C, 0.5), (2, C, 0.5)], [3, 1, 3, 1], (1, 3))  # ties: the lower tile goes first
    nested = (40, 38, 56, 46)  # half of A: IoU exactly 0.5, IoS exactly 1
    add("exact_threshold", [(1, A, 0.9), (2, nested, 0.8)], [1, 1], (1,))
    add("ios_nested", [(1, A, 0.9), (2, nested, 0.8)], [1, 3], (1, 3), metric="ios")
    add("ios_threshold_one", [(1, A, 0.9), (2, nested, 0.8)], [1, 1], (1,), metric="ios", match_thr=1.0)
    add("zero_area", [(1, (40, 40, 40, 50), 0.9), (2, (40, 40, 40, 50), 0.8), (2, (44, 44, 44, 44), 0.7), (4, (44, 44, 44, 44), 0.6)], [1, 1, 1, 1], (1,))
    # border = 2 source pixels at scale 1: on the threshold stays (strict comparisons), just inside it goes; edges on the image boundary never drop
    inside, lo, hi = float(np.nextafter(F(2), F(0))), 2.0, 62.0
    above = float(np.nextafter(F(62), F(64)))
    add("border", [(4, (lo, 10, 30, 30), 0.9), (4, (inside, 10, 30, 30), 0.8), (4, (10, lo, 30, 30), 0.7), (4, (10, inside, 30, 30), 0.6),  # left, top of tile 4
                   (1, (10, 10, hi, 30), 0.5), (1, (10, 10, above, 30), 0.4), (1, (10, 10, 30, hi), 0.3), (1, (10, 10, 30, above), 0.2),  # right, bottom of tile 1
                   (1, (0, 0, 30, 30), 0.95), (4, (34, 34, 64, 64), 0.96), (0, (0, 0, 64, 64), 0.1)],  # the image boundary: tile 1 left / top, tile 4 right / bottom, tile 0
        None, (1, 2), padded=True, keep_k=8)
    add("border_zero", [(4, (0, 10, 30, 30), 0.9), (1, (10, 10, 64, 30), 0.5)], [1, 1], (1,), padded=True, border=0.0)
    add("border_wide", [(4, (5, 10, 30, 30), 0.9), (1, (10, 10, 58.5, 30), 0.5), (0, (0, 0, 3, 3), 0.4)], [2, 2, 1], (1, 2), padded=True, border=6.0)
    add("everything_dropped", [(t, (0, 0, 64, 64), 0.5 + 0.1 * t) for t in (1, 2, 3, 4)], [2, 2, 2, 2], (2,), padded=True)
    add("cap", [(1, (2 + 8 * k, 2, 8 + 8 * k, 8), 0.9 - 0.1 * k) for k in range(4)] + [(2, A, 0.95), (1, B, 0.2)], [1, 1, 4, 4, 1, 3], (1, 3, 4), keep_k=8, max_heads=3)
    add("non_finite", [(1, (float("nan"), 10, 30, 30), 0.9), (2, (4, 10, float("inf"), 30), float("nan")), (4, (-float("inf"), 10, 30, 30), -float("nan")),
                       (0, (5, 5, 20, 20), float("inf")), (0, (6, 6, 20, 20), -0.0), (1, (6, 6, 20, 20), 0.0)], None, (1, 2), padded=True)
    return cases


def border_expectation():
    """statuses of the "border" case that concern the truncation rule: entry -> truncated?"""
    return [False, True, False, True, False, True, False, True, False, False, False]


def random_family(plan: SlicePlan, keep_k: int, n_live: int, seed: int, head_px=(12.0, 60.0)):
    """A seeded crowd: heads in image coordinates, each reported by every tile that sees it (jittered, clipped to the tile, so heads cut by a tile edge come out
    truncated), topped up with random boxes; scores from 101 values, so equal scores across tiles occur.  sum(counts) == n_live exactly, spread over the tiles."""
    rng = np.random.default_rng(seed)
    T = plan.n_tiles
    assert 0 <= n_live <= T * keep_k
    counts = np.full(T, n_live // T, np.int64)
    counts[:n_live - counts.sum()] += 1
    rng.shuffle(counts)
    n_pool = max(4, n_live // 3)
    size = rng.uniform(head_px[0], head_px[1], (n_pool, 2))
    xy = rng.uniform(0, 1, (n_pool, 2)) * [plan.width, plan.height]
    pool = np.concatenate([xy - size / 2, xy + size / 2], 1)
    boxes, scores = np.zeros((T, keep_k, 4), F), np.zeros((T, keep_k), F)
    for t in range(T):
        x, y, w, h, px, py, nw, nh = (int(v) for v in plan.tiles[t])
        s = float(plan.scale[t])
        seen = np.flatnonzero((pool[:, 2] > x + 1) & (pool[:, 0] < x + w - 1) & (pool[:, 3] > y + 1) & (pool[:, 1] < y + h - 1))
        rng.shuffle(seen)
        rows = []
        for k in seen[:counts[t]]:
            b = pool[k] + rng.normal(0, 0.04, 4) * np.tile(size[k], 2)
            rows.append(np.clip((b - [x, y, x, y]) * s + [px, py, px, py], [px, py, px, py], [px + nw, py + nh, px + nw, py + nh]))
        while len(rows) < counts[t]:
            c, d = rng.uniform([px, py], [px + nw, py + nh]), rng.uniform(3, 40, 2) * s
            rows.append(np.clip(np.concatenate([c - d / 2, c + d / 2]), -5, plan.image_size + 5))  # a few stick out of [0, S]: the clip of step 1
        if rows:
            boxes[t, :counts[t]] = np.array(rows)
            scores[t, :counts[t]] = np.sort(rng.integers(0, 101, counts[t]) / 100.0)[::-1]
    return boxes, scores, counts.astype(np.int32)
