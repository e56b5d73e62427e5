"""NumPy float64 restatement of the COCO-style box evaluation of include/vgh_eval.h (csrc/detection_ap.hip, head_detector_amd.detection_metrics): what
pycocotools' COCOeval(..., 'bbox') computes for one category, by its published definition, in plain loops.  Test infrastructure like mesh_metrics_ref.py:
the device is held to these values BITWISE (tests/test_gpu_detection_ap.py), and tools/detection_ap_bench.py times it as the CPU side.

Every float is one IEEE float64 operation in the order the header states (Python floats and NumPy float64 scalars round each operation on its own), every
count an integer; orders come from ``np.argsort(kind="mergesort")``, the curves from ``np.cumsum`` and ``np.searchsorted``."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RANGES = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
MAX_DETS = (1, 10, 100)


def iou_one(d, g, crowd):
    """bbIou for one pair of xywh boxes."""
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    da = dw * dh
    ga = gw * gh
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if not w > 0.0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if not h > 0.0:
        return 0.0
    i = w * h
    u = da if crowd else (da + ga) - i
    return i / u


def box_iou(dt, gt, crowd=None):
    """[nd, ng] float64, vectorised: the same operations as ``iou_one``, element by element."""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    crowd = np.zeros(len(gt), dtype=bool) if crowd is None else np.asarray(crowd).astype(bool)
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    if out.size == 0:
        return out
    da = (dt[:, 2] * dt[:, 3])[:, None]
    ga = (gt[:, 2] * gt[:, 3])[None, :]
    w = np.minimum((dt[:, 0] + dt[:, 2])[:, None], (gt[:, 0] + gt[:, 2])[None, :]) - np.maximum(dt[:, 0][:, None], gt[:, 0][None, :])
    h = np.minimum((dt[:, 1] + dt[:, 3])[:, None], (gt[:, 1] + gt[:, 3])[None, :]) - np.maximum(dt[:, 1][:, None], gt[:, 1][None, :])
    hit = (w > 0.0) & (h > 0.0)
    i = w * h
    u = np.where(crowd[None, :], np.broadcast_to(da, i.shape), (da + ga) - i)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[hit] = (i / u)[hit]
    return out


def _walk(row, g_order, g_ign, crowd, taken, best):
    """The walk over the ground truths as the header words it -> the matched ground truth or -1."""
    m = -1
    for g in g_order:
        if taken[g] and not crowd[g]:
            continue
        if m > -1 and not g_ign[m] and g_ign[g]:
            break
        if row[g] < best:
            continue
        best = row[g]
        m = g
    return m


def _walk_fast(row, g_order, n_valid, crowd, taken, best):
    """The same result without the Python loop, for the sizes of the GPU tests: the walk ends on the highest IoU >= best among the ground truths it may
    take, of equal ones on the last; it enters the ignored ones only when no non-ignored one matched.  tests/test_detection_ap_host.py holds it to
    ``_walk``."""
    for part in (g_order[:n_valid], g_order[n_valid:]):
        if len(part) == 0:
            continue
        c = row[part]
        ok = (~taken[part] | crowd[part]) & (c >= best)
        if ok.any():
            return int(part[np.flatnonzero(ok & (c == c[ok].max()))[-1]])
    return -1


def match_image(dt, gt, gt_area, gt_crowd, iou_thrs, area_ranges, max_det, fast=True):
    """One image.  ``dt`` [nd, 5] xywh + score, ``gt`` [ng, 4] -> (order [kept]: the input position of the detection at each rank,
    match int32 [A, T, kept]: the matched ground truth's input index or -1, ignore bool [A, T, kept], n_pos int [A])."""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 5)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    ng = len(gt)
    area = gt[:, 2] * gt[:, 3] if gt_area is None else np.asarray(gt_area, dtype=np.float64)
    crowd = np.zeros(ng, dtype=bool) if gt_crowd is None else np.asarray(gt_crowd).astype(bool)
    order = np.argsort(-dt[:, 4], kind="mergesort")[:max_det]
    d = dt[order]
    kept = len(d)
    ious = box_iou(d[:, :4], gt, crowd)
    d_area = d[:, 2] * d[:, 3]
    T, A = len(iou_thrs), len(area_ranges)
    match = np.full((A, T, kept), -1, dtype=np.int32)
    ignore = np.zeros((A, T, kept), dtype=bool)
    n_pos = np.zeros(A, dtype=np.int64)
    for a, (lo, hi) in enumerate(area_ranges):
        g_ign = crowd | (area < lo) | (area > hi)
        g_order = np.argsort(g_ign.astype(np.uint8), kind="mergesort")  # non-ignored first, each group in input order
        n_pos[a] = int((~g_ign).sum())
        for t, thr in enumerate(iou_thrs):
            taken = np.zeros(ng, dtype=bool)
            best = min(float(thr), 1 - 1e-10)
            for p in range(kept):
                m = _walk_fast(ious[p], g_order, int(n_pos[a]), crowd, taken, best) if fast else _walk(ious[p], g_order, g_ign, crowd, taken, best)
                if m > -1:
                    match[a, t, p] = m
                    ignore[a, t, p] = g_ign[m]
                    taken[m] = True
                else:
                    ignore[a, t, p] = bool(d_area[p] < lo or d_area[p] > hi)
    return order, match, ignore, n_pos


def match_all(detections, ground_truth, iou_thrs, area_ranges, max_det, gt_area=None, gt_crowd=None, fast=True):
    """Every image -> dict of the kept arrays, image after image in rank order: image, rank, index, score [K]; match, ignore [A, T, K]; n_pos [A]."""
    T, A = len(iou_thrs), len(area_ranges)
    image, rank, index, score, match, ignore = [], [], [], [], [], []
    n_pos = np.zeros(A, dtype=np.int64)
    for i, (dt, gt) in enumerate(zip(detections, ground_truth)):
        dt = np.asarray(dt, dtype=np.float64).reshape(-1, 5)
        order, m, ig, npos = match_image(dt, gt, None if gt_area is None else gt_area[i], None if gt_crowd is None else gt_crowd[i], iou_thrs, area_ranges, max_det, fast)
        image.append(np.full(len(order), i, dtype=np.int32))
        rank.append(np.arange(len(order), dtype=np.int32))
        index.append(order.astype(np.int32))
        score.append(dt[order, 4])
        match.append(m)
        ignore.append(ig)
        n_pos += npos
    cat = lambda parts, empty, axis=0: np.concatenate(parts, axis=axis) if parts else empty  # noqa: E731
    return {"image": cat(image, np.zeros(0, np.int32)), "rank": cat(rank, np.zeros(0, np.int32)), "index": cat(index, np.zeros(0, np.int32)),
            "score": cat(score, np.zeros(0, np.float64)), "match": cat(match, np.zeros((A, T, 0), np.int32), 2),
            "ignore": cat(ignore, np.zeros((A, T, 0), bool), 2), "n_pos": n_pos.astype(np.int32)}


def accumulate(m, n_iou_thr, rec_thrs, n_area, max_dets):
    """The curves from ``match_all``'s arrays -> (precision [T, R, A, M], recall [T, A, M], scores [T, R, A, M])."""
    rec_thrs = np.asarray(rec_thrs, dtype=np.float64)
    T, R, A, M = n_iou_thr, len(rec_thrs), n_area, len(max_dets)
    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    scores = -np.ones((T, R, A, M))
    for a in range(A):
        npig = int(m["n_pos"][a])
        if npig == 0:
            continue
        for k, max_det in enumerate(max_dets):
            keep = m["rank"] < max_det  # the kept arrays are in (image, rank) order, so the stable sort below orders by (-score, image, rank)
            sc = m["score"][keep]
            inds = np.argsort(-sc, kind="mergesort")
            sc_sorted = sc[inds]
            hit = (m["match"][a][:, keep] >= 0)[:, inds]
            ign = m["ignore"][a][:, keep][:, inds]
            tps = np.logical_and(hit, np.logical_not(ign))
            fps = np.logical_and(np.logical_not(hit), np.logical_not(ign))
            tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
            fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
            for t in range(T):
                tp, fp = tp_sum[t], fp_sum[t]
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                q = np.zeros((R,))
                ss = np.zeros((R,))
                recall[t, a, k] = rc[-1] if nd else 0
                pr = pr.tolist()
                q = q.tolist()
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                inds_r = np.searchsorted(rc, rec_thrs, side="left")
                for ri, pi in enumerate(inds_r):
                    if pi < nd:
                        q[ri] = pr[pi]
                        ss[ri] = sc_sorted[pi]
                precision[t, :, a, k] = np.array(q)
                scores[t, :, a, k] = np.array(ss)
    return precision, recall, scores


def summarize(precision, recall, iou_thrs, max_dets):
    """COCOeval.summarize's twelve numbers, entry by entry: (curve, IoU threshold or all, area range position, max_dets position), each the mean of the
    selected values above -1, or -1 when nothing is selected or left.  Written apart from ``detection_metrics.summarize_stats``, which the tests hold
    to this table and to the planted cases' hand-worked numbers."""
    last = len(max_dets) - 1
    table = [("precision", None, 0, last), ("precision", 0.5, 0, last), ("precision", 0.75, 0, last), ("precision", None, 1, last),
             ("precision", None, 2, last), ("precision", None, 3, last), ("recall", None, 0, 0), ("recall", None, 0, 1), ("recall", None, 0, last),
             ("recall", None, 1, last), ("recall", None, 2, last), ("recall", None, 3, last)]
    stats = []
    for curve, iou, a, k in table:
        values = []
        if a < precision.shape[2] and k < len(max_dets):
            for t, thr in enumerate(np.asarray(iou_thrs, dtype=np.float64)):
                if iou is None or thr == iou:
                    values.append(precision[t, :, a, k] if curve == "precision" else recall[t, a:a + 1, k])
        values = np.concatenate(values) if values else np.zeros(0)
        values = values[values > -1]
        stats.append(float(np.mean(values)) if len(values) else -1.0)
    return np.array(stats)


def evaluate(detections, ground_truth, iou_thrs=None, rec_thrs=None, area_ranges=None, max_dets=MAX_DETS, gt_area=None, gt_crowd=None, fast=True):
    """-> dict(precision, recall, scores, n_pos, stats, match=the arrays of ``match_all``)."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    rec_thrs = REC_THRS if rec_thrs is None else np.asarray(rec_thrs, dtype=np.float64)
    area_ranges = AREA_RANGES if area_ranges is None else np.asarray(area_ranges, dtype=np.float64).reshape(-1, 2)
    max_dets = tuple(int(k) for k in max_dets)
    m = match_all(detections, ground_truth, iou_thrs, area_ranges, max_dets[-1], gt_area, gt_crowd, fast)
    precision, recall, scores = accumulate(m, len(iou_thrs), rec_thrs, len(area_ranges), max_dets)
    return {"precision": precision, "recall": recall, "scores": scores, "n_pos": m["n_pos"], "stats": summarize(precision, recall, iou_thrs, max_dets),
            "match": m}


# ---- inputs shared by tests/test_detection_ap_host.py and tests/test_gpu_detection_ap.py -----------------------------------------------------------------
GT_COUNTS = (0, 1, 64, 65, 300)  # none, one, a wave, one past a wave, several waves; all inside the kernel's 512-entry LDS variant
LARGE_GT_COUNTS = (513, 1100)  # one past that variant, and well inside the 4 096-entry one: matched bits 8 .. 17 of a lane, positions above 512
DT_COUNTS = (0, 1, 99, 100, 101, 1024)  # either side of the default cut, and the ceiling
SIDES = (0, 4, 8, 16, 32, 64, 96, 128)  # 32 x 32 = 1024 and 96 x 96 = 9216 lie on the borders of small / medium / large and belong to both neighbours


def seeded_image(rng, ng, nd):
    """Integer boxes on a grid of 8 with few sizes and few scores: equal IoUs, equal scores, touching, nested and zero-area boxes are all frequent.
    -> (dt [nd, 5], gt [ng, 4], crowd uint8 [ng])."""
    def boxes(n):
        return np.stack([rng.integers(0, 16, n) * 8, rng.integers(0, 16, n) * 8, rng.choice(SIDES, n), rng.choice(SIDES, n)], axis=1).astype(np.float64).reshape(n, 4)

    gt = boxes(ng)
    dt = boxes(nd)
    if ng and nd:  # most detections sit on or next to a ground truth
        src = rng.integers(0, ng, nd)
        near = rng.random(nd) < 0.7
        dt[near] = gt[src[near]]
        shift = rng.random(nd) < 0.4
        dt[near & shift, :2] += rng.integers(-1, 2, (int((near & shift).sum()), 2)) * 8
    score = rng.integers(1, 20, nd) / 20.0
    crowd = (rng.random(ng) < 0.08).astype(np.uint8)
    return np.concatenate([dt, score[:, None]], axis=1), gt, crowd


def seeded_set(name):
    """"one": I = 1; "three": I = 3 with the 1 024-detection image; "many": I = 257, every pair of GT_COUNTS x DT_COUNTS among small images;
    "large": the two LARGE_GT_COUNTS images and a small one;
    "mixed": small images around one with 513 ground truths, which takes the whole set to the 4 096-entry variant.
    While ranking, the kernel holds 4 x its ground-truth capacity of scores at a time: 2 048 in the 512-entry variant, 16 384 in the other.  "many"
    holds an image of 2 500 detections and "mixed" one of 17 000, so both variants go through more than one tile of scores (both are cut to 100).
    -> (detections, ground_truth, gt_crowd, max_dets)."""
    rng = np.random.default_rng({"one": 11, "three": 12, "many": 13, "large": 14, "mixed": 15}[name])
    if name == "one":
        sizes, max_dets = [(65, 101)], (1, 10, 100)
    elif name == "three":
        sizes, max_dets = [(300, 1024), (0, 99), (64, 0)], (1, 100, 1024)
    elif name == "large":
        sizes, max_dets = [(LARGE_GT_COUNTS[0], 200), (LARGE_GT_COUNTS[1], 300), (3, 40)], (1, 100, 1024)
    elif name == "mixed":
        sizes, max_dets = [(2, 5), (65, 40), (0, 3), (LARGE_GT_COUNTS[0], 150), (7, 0), (300, 101), (1, 1), (5, 17000)], (1, 10, 100)
    else:
        sizes = [(GT_COUNTS[(i // 8) % 5], DT_COUNTS[(i // 8) % 6]) if i % 8 == 0 else (i % 4, i % 7) for i in range(257)]
        sizes[5] = (3, 2500)
        max_dets = (1, 10, 100)
    images = [seeded_image(rng, ng, nd) for ng, nd in sizes]
    for dt, _, _ in images:
        if len(dt) > 2048:  # scores in tied pairs all over the image: the best 100 come from every tile of scores, and ties reach across tiles
            dt[:, 4] = np.floor(rng.permutation(len(dt)) / 2) / len(dt)
    return [im[0] for im in images], [im[1] for im in images], [im[2] for im in images], max_dets


def planted(name):
    """The hand-worked cases of tests/test_detection_ap_host.py -> (detections, ground_truth, options)."""
    if name == "tp_fp_tp":  # two ground truths; detections TP (0.9), FP (0.8), TP (0.7)
        return [[[0, 0, 10, 10, 0.9], [50, 50, 10, 10, 0.8], [20, 0, 10, 10, 0.7]]], [[[0, 0, 10, 10], [20, 0, 10, 10]]], {}
    if name == "perfect":  # six images, one ground truth each, two per size class, found exactly
        gts = [[[5, 5, s, s]] for s in (10, 12, 50, 60, 200, 300)]
        return [[g[0] + [0.9 - 0.1 * i]] for i, g in enumerate(gts)], gts, {}
    if name == "no_detections":
        return [[], []], [[[0, 0, 10, 10]], [[0, 0, 50, 50], [0, 0, 200, 200]]], {}
    if name == "small_only":  # no medium and no large ground truth
        return [[[0, 0, 10, 10, 0.9]]], [[[0, 0, 10, 10], [40, 40, 20, 20]]], {}
    if name == "ignored_match":  # in "small" the first detection matches the large (ignored) ground truth: neither TP nor FP
        return [[[0, 0, 100, 100, 0.9], [200, 200, 10, 10, 0.8]]], [[[200, 200, 10, 10], [0, 0, 100, 100]]], {}
    if name == "equal_iou":  # both ground truths overlap the detection with IoU exactly 0.5: the later one is taken
        return [[[0, 0, 10, 10, 0.9]]], [[[0, 0, 10, 20], [0, 0, 20, 10]]], {}
    if name in ("rank_100", "rank_100_counted"):  # the only true positive has the lowest of 101 scores
        dt = [[1000 + 20 * i, 0, 10, 10, 0.99 - 0.001 * i] for i in range(100)] + [[0, 0, 10, 10, 0.5]]
        return [dt], [[[0, 0, 10, 10]]], ({} if name == "rank_100" else {"max_dets": (1, 10, 1000)})
    raise KeyError(name)


PLANTED = ("tp_fp_tp", "perfect", "no_detections", "small_only", "ignored_match", "equal_iou", "rank_100", "rank_100_counted")
