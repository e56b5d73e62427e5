"""Mesh benchmark metrics: how good a set of predicted heads is against ground-truth meshes, with the DAD-3DHeads numbers the reference reports
(yolo_head_training/evaluation/evaluate_dad.py:111,256-306 and evaluation/dad_utils.py): ``nme_2d``, ``z_n``, ``rot_error``, ``angle_error``, ``chamfer``.

  z_order_accuracy(pred, gt, top_k=5, neighbours="reference")     -> (ratio [n], count [n])        calc_zn, every head in one launch      (device)
  nearest_points(query, points, transform=None, query_scale=None) -> (sqdist, index, mean)         one-sided nearest neighbour            (device)
  chamfer_to_gt(gt_vertices, pred_vertices, gt_landmarks7, pred_landmarks7, ...) -> chamfer [n]    calc_ch_dist without its file reads    (host + device)
  procrustes(X, Y, scaling=True, reflection="best")               -> (d, Z, tform)                 MATLAB's procrustes                    (host, float64)
  landmarks_from_embedding(vertices, faces, lmk_face_idx, lmk_b_coords) -> [n, L, 3]               mesh_points_by_barycentric_coordinates (host)
  rotation_errors(R_pred, R_gt)                                   -> (rot_error [n], angle_error [n])                                     (host, float64)
  nme_2d(pred_landmarks, gt_landmarks, normaliser)                -> [n]                                                                  (host, float64)

The two searches are the hot path (6.1 M pairs a head for Z_n at the 2 470 head vertices, 10.5 M for chamfer) and run in csrc/mesh_metrics.hip
(libvgheval.so, include/vgh_eval.h); there is no CPU path for them.  Distances are squared distances in float64 from the float32 coordinates, ordered by
(distance, index): counts, indices and distances are bitwise reproducible and equal to the float64 restatement tests/mesh_metrics_ref.py.

THE QUIRK OF calc_zn, kept.  The source sorts with ``argsort(distances, dim=0)`` and then takes ``[:, 1 : top_k + 1]``: columns, not rows.  As written,
vertex i is compared with the i-th nearest point of vertex j + 1 (j = 0 .. top_k - 1), not with its own nearest neighbours.  ``neighbours="reference"``
computes exactly that (and reproduces the source's values); ``neighbours="nearest"`` is the intended reading: every vertex against its own ``top_k`` nearest.

Every function takes NumPy arrays or GPU tensors; the device functions return NumPy (``to_host=True``) or GPU tensors, the host functions NumPy.
Arguments are validated before a GPU is looked for."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib_eval

SEVEN_OF_68 = (36, 39, 42, 45, 33, 48, 54)  # get_7_landmarks_from_68: eye corners (outer, inner, inner, outer), nose tip, mouth corners
METRIC_KEYS = ("nme_2d", "z_n", "rot_error", "angle_error", "chamfer")  # the keys of evaluate_dad.py:111, in its order


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------------------
def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _device_of(*candidates):
    """The device of the first GPU tensor among the arguments; host data alone needs a GPU to be present."""
    for c in candidates:
        if isinstance(c, torch.Tensor):
            if not c.is_cuda:
                raise ValueError("a torch tensor must live on the GPU (pass NumPy for host data)")
            return c.device
    if not torch.cuda.is_available():
        raise _lib_eval.VghError("mesh metrics need a GPU: the HIP kernels of libvgheval.so are the only implementation of the neighbour searches")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(a, dev, dtype):
    """A contiguous tensor of ``dtype`` on ``dev``; the caller's array or tensor is never written."""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError("a torch tensor must live on the GPU (pass NumPy for host data)")
        return a.detach().to(device=dev, dtype=dtype).contiguous()
    np_dtype = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(dev)


def _host(a, dtype=np.float64) -> np.ndarray:
    """A NumPy copy-or-view of ``a`` as ``dtype`` (``None``: as it is); GPU tensors are brought to the host."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)


def _points_shape(shape, what):
    """[N, 3] or [n, N, 3] -> (n, N)."""
    shape = tuple(shape)
    if len(shape) not in (2, 3) or shape[-1] != 3:
        raise ValueError(f"{what} must be [N, 3] or [n, N, 3], got {shape}")
    return (shape[0] if len(shape) == 3 else 1), shape[-2]


def _per_head(a, n, tail, what):
    """``a`` as float64 [n, *tail] on the host: one entry per head, or one entry shared by all heads."""
    a = _host(a)
    if a.shape == tuple(tail):
        a = np.broadcast_to(a, (n,) + tuple(tail))
    if a.shape != (n,) + tuple(tail):
        raise ValueError(f"{what} must be {list(tail)} or {[n] + list(tail)}, got {a.shape}")
    return np.ascontiguousarray(a)


# ---- Z_n -----------------------------------------------------------------------------------------------------------------------------------------------
def z_order_accuracy(pred, gt, top_k: int = 5, neighbours: str = "reference", to_host: bool = True):
    """``calc_zn`` (dad_utils.py:8-35) for one head ([N, 3]) or many ([n, N, 3]) -> (ratio float64 [n], count int32 [n]).

    ``count`` is the number of pairs (i, j), i < N, j < top_k, with ``(gt_z[i] >= gt_z[p]) == (pred_z[i] >= pred_z[p])`` for the partner p (the module
    docstring states both ``neighbours``); ``ratio = count / (N * top_k)``, and ``ratio.mean()`` is what ``calc_zn`` returns.  Partners are found among
    the GROUND-TRUTH points by squared float64 distance, ties by index.  Inputs are converted to float32 (what the kernel reads) and never modified.
    ``N < top_k + 1`` raises ValueError (the source would index out of range)."""
    if neighbours not in _lib_eval.NEIGHBOURS:
        raise ValueError(f"neighbours must be 'reference' or 'nearest', got {neighbours!r}")
    top_k = int(top_k)
    if not 1 <= top_k <= _lib_eval.MAX_TOP_K:
        raise ValueError(f"top_k must lie in 1 .. {_lib_eval.MAX_TOP_K}, got {top_k}")
    n, N = _points_shape(_shape(gt), "gt")
    if _points_shape(_shape(pred), "pred") != (n, N) or len(_shape(pred)) != len(_shape(gt)):
        raise ValueError(f"pred {_shape(pred)} and gt {_shape(gt)} must have the same shape")
    if N < top_k + 1:
        raise ValueError(f"{N} points are too few for top_k = {top_k}: at least top_k + 1 are needed")
    if N > _lib_eval.MAX_POINTS or n > _lib_eval.MAX_HEADS:
        raise ValueError(f"{n} heads of {N} points exceed {_lib_eval.MAX_HEADS} heads of {_lib_eval.MAX_POINTS} points")
    dev = _device_of(pred, gt)
    p = _to_device(pred, dev, torch.float32).reshape(n, N, 3)
    g = _to_device(gt, dev, torch.float32).reshape(n, N, 3)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    job = _lib_eval.ZOrderJob()
    job.n_heads, job.n_points, job.top_k, job.mode = n, N, top_k, _lib_eval.NEIGHBOURS[neighbours]
    if n:
        job.pred_dev, job.gt_dev, job.agree_dev = p.data_ptr(), g.data_ptr(), count.data_ptr()
    with torch.cuda.device(dev):
        _lib_eval.check(_lib_eval.load().vghev_z_order(job, torch.cuda.current_stream().cuda_stream))
    if to_host:
        count = count.cpu().numpy()
        return count.astype(np.float64) / float(N * top_k), count
    # a tensor divisor: dividing by a Python number multiplies by its rounded reciprocal on the device, which is not count / (N * top_k) to the last bit
    return count.to(torch.float64) / torch.full((n,), float(N * top_k), dtype=torch.float64, device=dev), count


# ---- nearest neighbour ------------------------------------------------------------------------------------------------------------------------------
def check_nearest_arguments(q_shape, p_shape, transform=None, query_scale=None, point_scale=None):
    """Validates what needs no GPU -> (n, M, P, transform float64 [n, 3, 4] or None, query_scale float64 [n] or None, point_scale float64 [n] or None)."""
    n, M = _points_shape(q_shape, "query")
    n_p, P = _points_shape(p_shape, "points")
    if n_p != n or len(tuple(q_shape)) != len(tuple(p_shape)):
        raise ValueError(f"query {tuple(q_shape)} and points {tuple(p_shape)} must hold the same number of heads")
    if M < 1 or P < 1:
        raise ValueError(f"query and points must not be empty, got {M} queries and {P} points")
    if max(M, P) > _lib_eval.MAX_POINTS or n > _lib_eval.MAX_HEADS:
        raise ValueError(f"{n} heads of {M} x {P} points exceed {_lib_eval.MAX_HEADS} heads of {_lib_eval.MAX_POINTS} points")
    if point_scale is not None and transform is None:
        raise ValueError("point_scale needs a transform")
    t = None if transform is None else _per_head(transform, n, (3, 4), "transform")
    qs = None if query_scale is None else _per_head(query_scale, n, (), "query_scale")
    ps = None if point_scale is None else _per_head(point_scale, n, (), "point_scale")
    return n, M, P, t, qs, ps


def nearest_points(query, points, transform=None, query_scale=None, point_scale=None, to_host: bool = True):
    """For every query the nearest point of the same head -> (sqdist float64 [n, M], index int32 [n, M], mean float64 [n]).

    ``query`` [M, 3] or [n, M, 3], ``points`` [P, 3] or [n, P, 3] (float32 is what the kernel reads).  ``query_scale`` (a number or [n]): the query is
    ``float64(query) * query_scale``.  ``transform`` ([3, 4] or [n, 3, 4], float64, row k = (R0k, R1k, R2k, tk)) with ``point_scale`` s (default 1): the point is
    ``p_k = ((v0 * T[k][0] + v1 * T[k][1]) + v2 * T[k][2]) * s + T[k][3]``, i.e. ``s * v @ R + t`` for ``T = [R.T | t]`` (``similarity_transform``).  The
    distance is ``(dx * dx + dy * dy) + dz * dz`` in float64; on a tie the lowest index wins; ``mean`` is the mean of a head's ``sqdist`` summed in the
    fixed order include/vgh_eval.h states.  With M the ground truth and the points the prediction, ``mean`` is the one-sided chamfer distance."""
    n, M, P, t, qs, ps = check_nearest_arguments(_shape(query), _shape(points), transform, query_scale, point_scale)
    dev = _device_of(query, points)
    q = _to_device(query, dev, torch.float32).reshape(n, M, 3)
    p = _to_device(points, dev, torch.float32).reshape(n, P, 3)
    t, qs, ps = (None if a is None else torch.from_numpy(a).to(dev) for a in (t, qs, ps))
    sqd = torch.empty((n, M), dtype=torch.float64, device=dev)
    idx = torch.empty((n, M), dtype=torch.int32, device=dev)
    mean = torch.empty((n,), dtype=torch.float64, device=dev)
    job = _lib_eval.NearestJob()
    job.n_heads, job.n_queries, job.n_points = n, M, P
    if n:
        job.query_dev, job.points_dev, job.sqdist_dev, job.index_dev, job.mean_dev = q.data_ptr(), p.data_ptr(), sqd.data_ptr(), idx.data_ptr(), mean.data_ptr()
        job.query_scale_dev = None if qs is None else qs.data_ptr()
        job.transform_dev = None if t is None else t.data_ptr()
        job.point_scale_dev = None if ps is None else ps.data_ptr()
    with torch.cuda.device(dev):
        _lib_eval.check(_lib_eval.load().vghev_nearest(job, torch.cuda.current_stream().cuda_stream))
    out = (sqd, idx, mean)
    if len(_shape(query)) == 2:
        out = (sqd[0], idx[0], mean[0])
    return tuple(o.cpu().numpy() for o in out) if to_host else out


# ---- Procrustes (host, float64) -------------------------------------------------------------------------------------------------------------------
def procrustes(X, Y, scaling: bool = True, reflection="best"):
    """MATLAB's ``procrustes``: the similarity transform of the points ``Y`` [n, my] that fits them best, in the least-squares sense, to ``X`` [n, m]
    (my <= m; missing columns count as zeros) -> (d, Z, tform).

    ``Z = b * Y @ T + c`` are the fitted points, ``tform = {"rotation": T [my, m], "scale": b, "translation": c [m]}``, and ``d`` is the residual sum of
    squares divided by the sum of squares of the centred ``X``.  ``scaling=False`` fixes b = 1.  ``reflection``: "best" takes the orthogonal T of the
    smaller residual, True / False force det(T) < 0 / > 0.  Runs on the host in float64 (an SVD of an m x m matrix)."""
    X, Y = _host(X), _host(Y)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0] or Y.shape[1] > X.shape[1] or X.shape[0] < 1:
        raise ValueError(f"X [n, m] and Y [n, my <= m] must hold the same number of points, got {X.shape} and {Y.shape}")
    if reflection not in ("best", True, False):
        raise ValueError(f"reflection must be 'best', True or False, got {reflection!r}")
    m, my = X.shape[1], Y.shape[1]
    centre_x, centre_y = X.mean(axis=0), Y.mean(axis=0)
    Xc, Yc = X - centre_x, Y - centre_y
    ss_x, ss_y = float((Xc * Xc).sum()), float((Yc * Yc).sum())
    if not (ss_x > 0.0 and ss_y > 0.0 and math.isfinite(ss_x) and math.isfinite(ss_y)):
        raise ValueError("procrustes needs finite points that do not all coincide")
    size_x, size_y = math.sqrt(ss_x), math.sqrt(ss_y)
    Xu = Xc / size_x  # both shapes at unit size
    Yu = np.concatenate([Yc / size_y, np.zeros((Y.shape[0], m - my))], axis=1)
    U, sv, Vt = np.linalg.svd(Xu.T @ Yu, full_matrices=False)  # the orthogonal T maximising trace(T' Yu' Xu) is V U'
    V = Vt.T.copy()
    sv = sv.copy()
    T = V @ U.T
    if reflection != "best" and bool(reflection) != bool(np.linalg.det(T) < 0):
        V[:, -1] = -V[:, -1]  # give up the smallest singular value: the best T of the other handedness
        sv[-1] = -sv[-1]
        T = V @ U.T
    trace = float(sv.sum())
    if scaling:
        b = trace * size_x / size_y
        d = 1.0 - trace * trace
        Z = size_x * trace * (Yu @ T) + centre_x
    else:
        b = 1.0
        d = 1.0 + ss_y / ss_x - 2.0 * trace * size_y / size_x
        Z = size_y * (Yu @ T) + centre_x
    T = T[:my, :]
    c = centre_x - b * (centre_y @ T)
    return d, Z, {"rotation": T, "scale": b, "translation": c}


def similarity_transform(tform) -> tuple:
    """A ``procrustes`` result as ``nearest_points`` takes it -> (transform float64 [3, 4] = [R.T | t], point_scale)."""
    R, t = np.asarray(tform["rotation"], dtype=np.float64), np.asarray(tform["translation"], dtype=np.float64)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"a 3-D similarity transform is needed, got rotation {R.shape} and translation {t.shape}")
    return np.concatenate([R.T, t[:, None]], axis=1), float(tform["scale"])


# ---- landmarks ---------------------------------------------------------------------------------------------------------------------------------------
def landmarks_from_embedding(vertices, faces, lmk_face_idx, lmk_b_coords) -> np.ndarray:
    """``mesh_points_by_barycentric_coordinates`` (dad_utils.py:41-53) for [V, 3] or [n, V, 3] -> [L, 3] or [n, L, 3]: landmark l is the point of triangle
    ``faces[lmk_face_idx[l]]`` with the barycentric coordinates ``lmk_b_coords[l]``, summed over the three corners in order.  The embedding
    (flame_static_embedding.pkl / flame_dynamic_embedding.npy of FLAME) is a user-supplied asset like the FLAME pickle.  A host helper; the result has
    the vertices' floating-point type."""
    v = _host(vertices, None)
    if not np.issubdtype(v.dtype, np.floating):
        v = v.astype(np.float64)
    n, V = _points_shape(v.shape, "vertices")
    tri = _host(faces, None)
    idx = _host(lmk_face_idx, None)
    if tri.ndim != 2 or tri.shape[1] != 3 or not np.issubdtype(tri.dtype, np.integer):
        raise ValueError(f"faces must be integers [F, 3], got {tri.dtype} {tri.shape}")
    if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"lmk_face_idx must be integers [L], got {idx.dtype} {idx.shape}")
    b = _host(lmk_b_coords, v.dtype)
    if b.shape != (idx.shape[0], 3):
        raise ValueError(f"lmk_b_coords must be [{idx.shape[0]}, 3], got {b.shape}")
    if idx.size and (idx.min() < 0 or idx.max() >= tri.shape[0]):
        raise ValueError(f"lmk_face_idx outside 0 .. {tri.shape[0] - 1}")
    if tri.size and (tri.min() < 0 or tri.max() >= V):
        raise ValueError(f"faces name a vertex outside 0 .. {V - 1}")
    corners = v.reshape(n, V, 3)[:, tri[idx]]  # [n, L, corner, xyz]
    out = (corners * b[None, :, :, None]).sum(axis=2)
    return out if v.ndim == 3 else out[0]


# ---- chamfer -----------------------------------------------------------------------------------------------------------------------------------------
def chamfer_to_gt(gt_vertices, pred_vertices, gt_landmarks7, pred_landmarks7, gt_subset=None, inter_eye=(1, 2), inter_eye_dist: float = 20.0,
                  to_host: bool = True):
    """``calc_ch_dist`` (dad_utils.py:135-154) without its file reads, for one head or n -> chamfer float64 [n] (a scalar array for one head).

      1. the ground truth is scaled to the standard inter-eye distance: scale = inter_eye_dist / |gt_landmarks7[a] - gt_landmarks7[b]|, (a, b) = inter_eye
      2. ``procrustes`` from the predicted seven landmarks onto the scaled ground-truth seven (host, float64)
      3. that transform is applied to ALL predicted vertices on the device, inside the search (``nearest_points``; nothing is materialised)
      4. the mean squared distance from every scaled ``gt_vertices[gt_subset]`` (the source's face.npy subset; default: all) to its nearest prediction

    ``gt_landmarks7`` / ``pred_landmarks7`` [7, 3] or [n, 7, 3] are the landmarks ``SEVEN_OF_68`` of the UNSCALED ground truth and of the prediction
    (``landmarks_from_embedding``).  The mean squared nearest distance is kaolin's ``chamfer_distance(p1, p2, w1=1.0, w2=0.0)`` by its documented
    definition; kaolin is not available to this project, so the value is UNPINNED against kaolin itself.  The source also rounds the aligned vertices to
    float32 on the way; here they stay float64."""
    n, Vg = _points_shape(_shape(gt_vertices), "gt_vertices")
    n_p, _ = _points_shape(_shape(pred_vertices), "pred_vertices")
    if n_p != n or len(_shape(gt_vertices)) != len(_shape(pred_vertices)):
        raise ValueError(f"gt_vertices {_shape(gt_vertices)} and pred_vertices {_shape(pred_vertices)} must hold the same number of heads")
    gl = _host(gt_landmarks7).reshape((-1,) + tuple(_shape(gt_landmarks7)[-2:]))
    pl = _host(pred_landmarks7).reshape((-1,) + tuple(_shape(pred_landmarks7)[-2:]))
    if gl.shape != (n, 7, 3) or pl.shape != (n, 7, 3):
        raise ValueError(f"gt_landmarks7 and pred_landmarks7 must be [7, 3] or [{n}, 7, 3], got {_shape(gt_landmarks7)} and {_shape(pred_landmarks7)}")
    a, b = (int(i) for i in inter_eye)
    if not (0 <= a < 7 and 0 <= b < 7 and a != b):
        raise ValueError(f"inter_eye must name two different landmarks of the seven, got {inter_eye}")
    subset = None
    if gt_subset is not None:
        subset = _host(gt_subset, None)
        if subset.ndim != 1 or subset.size == 0 or not np.issubdtype(subset.dtype, np.integer) or subset.min() < 0 or subset.max() >= Vg:
            raise ValueError(f"gt_subset must be a non-empty list of vertex indices in 0 .. {Vg - 1}")
    eye = np.linalg.norm(gl[:, a] - gl[:, b], axis=1)
    if not (np.isfinite(eye).all() and (eye > 0).all()):
        raise ValueError("the ground truth's inter-eye distance must be finite and above zero")
    scale = float(inter_eye_dist) / eye
    T, s = np.zeros((n, 3, 4)), np.zeros((n,))
    for h in range(n):
        T[h], s[h] = similarity_transform(procrustes(scale[h] * gl[h], pl[h])[2])
    dev = _device_of(gt_vertices, pred_vertices)
    gt = _to_device(gt_vertices, dev, torch.float32).reshape(n, Vg, 3)
    if subset is not None:
        gt = gt.index_select(1, torch.from_numpy(subset.astype(np.int64)).to(dev))
    pred = _to_device(pred_vertices, dev, torch.float32).reshape(n, -1, 3)
    mean = nearest_points(gt, pred, transform=T, query_scale=scale, point_scale=s, to_host=False)[2] if n else torch.zeros((0,), dtype=torch.float64, device=dev)
    if len(_shape(gt_vertices)) == 2:
        mean = mean[0]
    return mean.cpu().numpy() if to_host else mean


# ---- pose and 2-D landmarks (host, float64) ---------------------------------------------------------------------------------------------------------
def rotation_errors(R_pred, R_gt):
    """evaluate_dad.py:256-266 for [3, 3] or [n, 3, 3] rotation matrices -> (rot_error, angle_error), float64 [n] (scalars for one pair).

    With ``R = R_pred @ R_gt.T``: ``rot_error`` is the Frobenius norm of ``I - R``; ``angle_error`` the geodesic angle of R in degrees, folded by the
    source's ``mae``: min(a, |a - 180|, a + 180).  The angle is ``atan2(|r|, trace(R) - 1)`` with r = (R21 - R12, R02 - R20, R10 - R01), which keeps its
    precision near 0 and 180 degrees where ``arccos`` loses it (the source goes through scipy's rotation vector, equal for proper rotations)."""
    Rp, Rg = _host(R_pred), _host(R_gt)
    if Rp.shape != Rg.shape or Rp.ndim not in (2, 3) or Rp.shape[-2:] != (3, 3):
        raise ValueError(f"R_pred and R_gt must both be [3, 3] or [n, 3, 3], got {Rp.shape} and {Rg.shape}")
    R = Rp.reshape(-1, 3, 3) @ Rg.reshape(-1, 3, 3).transpose(0, 2, 1)
    rot = np.sqrt(((np.eye(3) - R) ** 2).sum(axis=(1, 2)))
    r = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    angle = np.degrees(np.arctan2(np.sqrt((r * r).sum(axis=1)), R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0))
    angle = np.minimum(np.minimum(np.abs(angle), np.abs(angle - 180.0)), np.abs(angle + 180.0))
    return (rot, angle) if Rp.ndim == 3 else (rot[0], angle[0])


def nme_2d(pred_landmarks, gt_landmarks, normaliser):
    """evaluate_dad.py:277-285 for [L, 2] or [n, L, 2] -> float64 [n] (a scalar for one head): the mean over the landmarks of
    ``|gt - pred|_2 / normaliser``, times 100.  The normaliser is explicit, one per head.  Note what the source passes: ``sqrt(bbox[2] * bbox[3])`` of the
    annotation's box, which is an *xyxy* box there -- so its normaliser is sqrt(x2 * y2), not the square root of the box's area."""
    p, g = _host(pred_landmarks), _host(gt_landmarks)
    if p.shape != g.shape or p.ndim not in (2, 3) or p.shape[-1] != 2 or p.shape[-2] < 1:
        raise ValueError(f"pred_landmarks and gt_landmarks must both be [L, 2] or [n, L, 2], got {p.shape} and {g.shape}")
    n = p.shape[0] if p.ndim == 3 else 1
    norm = _per_head(normaliser, n, (), "normaliser")
    if not (norm > 0).all():
        raise ValueError("normaliser must be above zero")
    dist = np.sqrt(((g.reshape(n, -1, 2) - p.reshape(n, -1, 2)) ** 2).sum(axis=2))
    out = (dist / norm[:, None]).mean(axis=1) * 100.0
    return out if p.ndim == 3 else out[0]


# ---- the collection -----------------------------------------------------------------------------------------------------------------------------------
class HeadMeshMetrics:
    """Per-head arrays ([n], NumPy or GPU tensors) of the reference's five metrics; a metric that was not computed is ``None``.  ``z_n_count`` holds the
    integer agreement counts behind ``z_n``.  ``mean()`` gives what ``DadEvaluator.__call__`` returns."""

    def __init__(self, nme_2d=None, z_n=None, rot_error=None, angle_error=None, chamfer=None, z_n_count=None):
        self.nme_2d, self.z_n, self.rot_error, self.angle_error, self.chamfer, self.z_n_count = nme_2d, z_n, rot_error, angle_error, chamfer, z_n_count

    def __len__(self):
        for k in METRIC_KEYS:
            if getattr(self, k) is not None:
                return int(getattr(self, k).shape[0])
        return 0

    def mean(self) -> dict:
        """{"nme_2d", "z_n", "rot_error", "angle_error", "chamfer"}: the mean over the heads, NaN for a metric that was not computed or has no head."""
        out = {}
        for k in METRIC_KEYS:
            a = getattr(self, k)
            out[k] = float("nan") if a is None or a.shape[0] == 0 else float(a.mean())
        return out

    def __repr__(self):
        return f"HeadMeshMetrics(heads={len(self)}, metrics={[k for k in METRIC_KEYS if getattr(self, k) is not None]})"


def compare_heads(heads, gt_vertices, subset=None, top_k: int = 5, neighbours: str = "reference", gt_landmarks7=None, pred_landmarks7=None,
                  chamfer_subset=None, to_host: bool = True) -> HeadMeshMetrics:
    """What ``PredictionResult.compare_meshes`` does: Z_n of every head's ``vertices_3d`` against ``gt_vertices`` [n, V, 3] on the vertices ``subset``
    (the source's head_indices; default: all), and the chamfer distance when both landmark sets are given."""
    n_gt, V = _points_shape(_shape(gt_vertices), "gt_vertices")
    if len(_shape(gt_vertices)) != 3 or n_gt != len(heads):
        raise ValueError(f"gt_vertices must be [{len(heads)}, V, 3] (one mesh per head), got {_shape(gt_vertices)}")
    if (gt_landmarks7 is None) != (pred_landmarks7 is None):
        raise ValueError("chamfer needs both gt_landmarks7 and pred_landmarks7")
    if n_gt == 0:
        pred = np.zeros((0, V, 3), dtype=np.float32)
    else:
        pred = np.stack([np.asarray(h.vertices_3d, dtype=np.float32) for h in heads])
    if pred.shape != (n_gt, V, 3):
        raise ValueError(f"the heads carry vertices_3d {pred.shape[1:]}, the ground truth [{V}, 3]")
    sub = None
    if subset is not None:
        sub = _host(subset, None)
        if sub.ndim != 1 or not np.issubdtype(sub.dtype, np.integer) or (sub.size and (sub.min() < 0 or sub.max() >= V)):
            raise ValueError(f"subset must be a list of vertex indices in 0 .. {V - 1}")
    dev = _device_of(gt_vertices)
    gt = _to_device(gt_vertices, dev, torch.float32)
    pr = torch.from_numpy(pred).to(dev)
    if sub is not None:
        at = torch.from_numpy(sub.astype(np.int64)).to(dev)
        ratio, count = z_order_accuracy(pr.index_select(1, at), gt.index_select(1, at), top_k, neighbours, to_host=to_host)
    else:
        ratio, count = z_order_accuracy(pr, gt, top_k, neighbours, to_host=to_host)
    out = HeadMeshMetrics(z_n=ratio, z_n_count=count)
    if gt_landmarks7 is not None:
        out.chamfer = chamfer_to_gt(gt, pr, gt_landmarks7, pred_landmarks7, gt_subset=chamfer_subset, to_host=to_host)
    return out
