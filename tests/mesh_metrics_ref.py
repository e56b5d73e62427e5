"""A float64 NumPy restatement of what csrc/mesh_metrics.hip computes (include/vgh_eval.h): both neighbour rules of Z_n and the one-sided nearest search,
in the kernels' operation order and with a stable (distance, index) order.  NumPy never fuses a multiply into an add, so every figure here is what the
device must give bit for bit."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_metrics.npz")
MEAN_LANES = 256  # the fixed summation order of include/vgh_eval.h


def sqdist(a, b):
    """float64 [A, B]: (dx * dx + dy * dy) + dz * dz between the points a [A, 3] and b [B, 3] (any float type; float32 widens exactly)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def column_order(gt, columns):
    """int64 [N, len(columns)]: entry [r, c] is the point of rank r among the distances to vertex columns[c], ordered by (distance, index)."""
    gt = np.asarray(gt, dtype=np.float32)
    return np.argsort(sqdist(gt, gt[np.asarray(columns)]), axis=0, kind="stable")


def partners(gt, top_k, neighbours):
    """int64 [N, top_k]: the partner of (i, j)."""
    N = len(gt)
    assert N >= top_k + 1
    if neighbours == "reference":  # the column slice of the source: the point of rank i in column j + 1
        return column_order(gt, np.arange(1, top_k + 1))
    assert neighbours == "nearest"  # the point of rank j + 1 in column i
    out = np.empty((N, top_k), dtype=np.int64)
    for lo in range(0, N, 512):
        cols = np.arange(lo, min(lo + 512, N))
        out[cols] = column_order(gt, cols)[1:top_k + 1].T
    return out


def agree(pred, gt, top_k=5, neighbours="reference"):
    """The agreement count of one head: pred, gt [N, 3], compared as float32."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    p = partners(gt, top_k, neighbours)
    gz, pz = gt[:, 2], pred[:, 2]
    return int(((gz[:, None] >= gz[p]) == (pz[:, None] >= pz[p])).sum())


def z_order(pred, gt, top_k=5, neighbours="reference"):
    """(ratio float64 [n], count int32 [n]) for [n, N, 3]."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    count = np.array([agree(p, g, top_k, neighbours) for p, g in zip(pred, gt)], dtype=np.int32).reshape(len(gt))
    return count.astype(np.float64) / float(gt.shape[1] * top_k), count


def transformed(points, T=None, s=1.0):
    """float64 [P, 3]: p_k = ((v0 * T[k][0] + v1 * T[k][1]) + v2 * T[k][2]) * s + T[k][3], or the points widened when T is None."""
    v = np.asarray(points, dtype=np.float32).astype(np.float64)
    if T is None:
        return v
    T = np.asarray(T, dtype=np.float64)
    return np.stack([((v[:, 0] * T[k, 0] + v[:, 1] * T[k, 1]) + v[:, 2] * T[k, 2]) * np.float64(s) + T[k, 3] for k in range(3)], axis=1)


def fixed_order_mean(x):
    """Lane l adds elements l, l + 256, ... in turn, the 256 partial sums fold as a tree, the total is divided by the count."""
    x = np.asarray(x, dtype=np.float64)
    part = np.zeros((MEAN_LANES,), dtype=np.float64)
    for lo in range(0, len(x), MEAN_LANES):
        chunk = x[lo:lo + MEAN_LANES]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    h = MEAN_LANES // 2
    while h:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0] / np.float64(len(x))


def nearest_one(query, points, T=None, query_scale=None, point_scale=1.0):
    """(sqdist float64 [M], index int32 [M], mean float64) of one head."""
    q = np.asarray(query, dtype=np.float32).astype(np.float64)
    if query_scale is not None:
        q = q * np.float64(query_scale)
    p = transformed(points, T, point_scale)
    sq = np.empty((len(q),), dtype=np.float64)
    idx = np.empty((len(q),), dtype=np.int32)
    for lo in range(0, len(q), 256):
        d = sqdist(q[lo:lo + 256], p)
        at = d.argmin(axis=1)  # the first minimum: the lowest index on a tie
        idx[lo:lo + 256] = at
        sq[lo:lo + 256] = d[np.arange(len(at)), at]
    return sq, idx, fixed_order_mean(sq)


def nearest(query, points, transform=None, query_scale=None, point_scale=None):
    """(sqdist [n, M], index [n, M], mean [n]) for [n, M, 3] and [n, P, 3]; transform [n, 3, 4], the scales [n], or None."""
    n = len(query)
    res = [nearest_one(query[h], points[h], None if transform is None else transform[h], None if query_scale is None else query_scale[h],
                       1.0 if point_scale is None else point_scale[h]) for h in range(n)]
    M = np.shape(query)[1]
    return (np.array([r[0] for r in res], dtype=np.float64).reshape(n, M), np.array([r[1] for r in res], dtype=np.int32).reshape(n, M),
            np.array([r[2] for r in res], dtype=np.float64).reshape(n))


def jittered(template_mm, seed, jitter=0.5):
    """(gt, pred) float32 [V, 3]: the template in millimetres plus seeded jitter (breaks the template's mirror-symmetry ties), and a prediction whose depth
    order disagrees with it here and there."""
    rng = np.random.default_rng(seed)
    gt = (np.asarray(template_mm, dtype=np.float64) + rng.uniform(-jitter, jitter, size=np.shape(template_mm))).astype(np.float32)
    pred = (gt.astype(np.float64) + rng.normal(0.0, 4.0, size=gt.shape)).astype(np.float32)
    return gt, pred


# ---- seeded inputs shared by tests/golden/make_golden_metrics.py and the tests: the fixture stores seeds and outputs only ---------------------------
ZN_CASES = ("first24", "first40", "spread300", "all2470", "two_heads")  # the subsets of head_indices the fixture records calc_zn for
PROCRUSTES_CASES = tuple((seed, scaling, reflection) for seed in (11, 12) for scaling in (True, False) for reflection in ("best", True, False))


def zn_subset(name, head_indices):
    head_indices = np.asarray(head_indices, dtype=np.int64)
    if name == "first24":
        return head_indices[:24]
    if name == "first40":
        return head_indices[:40]
    if name in ("spread300", "two_heads"):
        return head_indices[np.linspace(0, len(head_indices) - 1, 300).astype(np.int64)]
    assert name == "all2470"
    return head_indices


def zn_inputs(name, seeds, v_template, head_indices):
    """(pred, gt) float32 [n, N, 3] of a recorded case: one head per seed."""
    mm = np.asarray(v_template, dtype=np.float64)[zn_subset(name, head_indices)] * 1000.0
    pairs = [jittered(mm, int(s)) for s in np.atleast_1d(seeds)]
    return np.stack([p for _, p in pairs]), np.stack([g for g, _ in pairs])


def procrustes_inputs(seed):
    """(X, Y) float64 [7, 3]: seven landmarks in millimetres and a rotated, scaled, shifted, noisy copy."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 30.0, size=(7, 3))
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Y = 0.37 * X @ Q + rng.normal(0.0, 2.0, size=(7, 3)) + np.array([120.0, -40.0, 15.0])
    return X, Y


def align_inputs():
    """(pred_vertices float32 [60, 3], pred_lmks [7, 3], gt_lmks [7, 3])."""
    gt_lmks, pred_lmks = procrustes_inputs(21)
    pred_vertices = np.random.default_rng(22).normal(100.0, 25.0, size=(60, 3)).astype(np.float32)
    return pred_vertices, pred_lmks, gt_lmks


def embedding_inputs():
    """(vertices float64 [2, 90, 3], faces int64 [150, 3], lmk_face_idx int64 [68], lmk_b_coords float64 [68, 3])."""
    rng = np.random.default_rng(31)
    vertices = rng.normal(0.0, 50.0, size=(2, 90, 3))
    faces = np.stack([rng.permutation(90)[:3] for _ in range(150)]).astype(np.int64)
    idx = rng.integers(0, 150, size=68).astype(np.int64)
    b = rng.dirichlet(np.ones(3), size=68)
    return vertices, faces, idx, b


def rotation_inputs():
    """(R_pred, R_gt) float64 [12, 3, 3]: random pairs, then relative angles of 0.01, 0.5, 89, 91, 179.5 and 179.99 degrees about random axes."""
    rng = np.random.default_rng(41)

    def rot(axis, deg):
        a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        t = np.radians(deg)
        return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)

    gt = [rot(rng.normal(size=3), rng.uniform(0.0, 180.0)) for _ in range(12)]
    pred = [rot(rng.normal(size=3), rng.uniform(0.0, 180.0)) for _ in range(6)]
    pred += [rot(rng.normal(size=3), deg) @ gt[6 + k] for k, deg in enumerate((0.01, 0.5, 89.0, 91.0, 179.5, 179.99))]
    return np.stack(pred), np.stack(gt)
