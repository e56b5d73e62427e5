"""Mesh benchmark metrics, the part that needs no GPU: the float64 restatement of Z_n (tests/mesh_metrics_ref.py, what the device is held to in
tests/test_gpu_mesh_metrics.py) against the reference's own ``calc_zn``, and the host functions of ``head_detector_amd.mesh_metrics`` against the reference's
``procrustes``, ``align_pred_to_gt``, ``mesh_points_by_barycentric_coordinates``, ``get_7_landmarks_from_68`` and rotation metrics, all as recorded in
tests/golden/mesh_metrics.npz by tests/golden/make_golden_metrics.py.  Float64 against float64 with different summation orders only: rtol 1e-10."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_metrics_ref as mr  # noqa: E402

from head_detector_amd import _lib_eval, mesh_metrics as mm  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

RTOL = 1e-10


@pytest.fixture(scope="module")
def g():
    return np.load(mr.GOLDEN)


@pytest.fixture(scope="module")
def v_template():
    return np.load(os.path.join(os.path.dirname(mr.GOLDEN), "flame_decode.npz"))["v_template"]


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.allclose(got, want, rtol=RTOL, atol=RTOL * max(1.0, float(np.abs(want).max(initial=0.0)))), (what, float(np.abs(got - want).max()))


@pytest.mark.parametrize("name", mr.ZN_CASES)
def test_restated_reference_mode_is_calc_zn(g, v_template, name):
    """Count equality: the recorded float is count / (N * 5), the mean over heads of it for two heads."""
    head_indices = g["head_indices"].astype(np.int64)
    assert head_indices.shape == (2470,)
    pred, gt = mr.zn_inputs(name, g[f"zn.{name}.seeds"], v_template, head_indices)
    ratio, count = mr.z_order(pred, gt, 5, "reference")
    N = gt.shape[1]
    value = float(g[f"zn.{name}.value"])
    assert round(value * len(gt) * N * 5) == int(count.sum()), (name, value, count)
    assert abs(value - ratio.mean()) < 1e-6
    # the intended reading is a different number on the same inputs: the quirk is real
    assert int(mr.z_order(pred, gt, 5, "nearest")[1].sum()) != int(count.sum())


def test_restatement_planted():
    rng = np.random.default_rng(5)
    gt = rng.normal(size=(1, 30, 3)).astype(np.float32)
    for mode in ("reference", "nearest"):
        assert mr.z_order(gt, gt, 5, mode)[1].tolist() == [150]
        flat = gt.copy()
        flat[..., 2] = 1.5
        assert mr.z_order(flat, flat, 3, mode)[1].tolist() == [90]  # all z equal: >= holds everywhere
        # distinct z, order reversed: only a vertex that is its own partner agrees (the column reading produces some, its own neighbours none)
        own = int((mr.partners(gt[0], 5, mode) == np.arange(30)[:, None]).sum())
        assert mr.z_order(-gt, gt, 5, mode)[1].tolist() == [own] and (own == 0) == (mode == "nearest")
    # nearest mode by brute force; duplicated points resolve by index
    pts = gt[0].copy()
    pts[7] = pts[3]
    want = np.array([sorted(range(30), key=lambda q: (float(mr.sqdist(pts[i:i + 1], pts[q:q + 1])[0, 0]), q))[1:6] for i in range(30)])
    assert np.array_equal(mr.partners(pts, 5, "nearest"), want)
    assert want[3][0] == 7 and want[7][0] == 7  # rank 0 of both is point 3 (the lower index), which is what is dropped: point 7 then meets itself
    sq, idx, mean = mr.nearest_one(pts[[7, 3]], pts)
    assert idx.tolist() == [3, 3] and sq.tolist() == [0.0, 0.0] and mean == 0.0
    x = rng.normal(size=1000)
    assert abs(mr.fixed_order_mean(x) - x.mean()) < 1e-15


def test_procrustes(g):
    for k, (seed, scaling, reflection) in enumerate(mr.PROCRUSTES_CASES):
        X, Y = mr.procrustes_inputs(seed)
        X0, Y0 = X.copy(), Y.copy()
        d, Z, tform = mm.procrustes(X, Y, scaling=scaling, reflection=reflection)
        assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
        close(d, g[f"procrustes.{k}.d"], (k, "d"))
        close(Z, g[f"procrustes.{k}.Z"], (k, "Z"))
        close(tform["rotation"], g[f"procrustes.{k}.rotation"], (k, "rotation"))
        close(tform["scale"], g[f"procrustes.{k}.scale"], (k, "scale"))
        close(tform["translation"], g[f"procrustes.{k}.translation"], (k, "translation"))
        close(tform["scale"] * Y @ tform["rotation"] + tform["translation"], Z, (k, "Z is the transform applied"))
        if reflection != "best":
            assert (np.linalg.det(tform["rotation"]) < 0) == reflection
    # fewer columns in Y, and what cannot be fitted
    X, Y = mr.procrustes_inputs(11)
    d, Z, tform = mm.procrustes(X, Y[:, :2])
    assert tform["rotation"].shape == (2, 3) and Z.shape == (7, 3) and 0.0 <= d <= 1.0
    for bad in ((X, Y[:6]), (X[:, :2], Y), (X, np.ones((7, 3))), (X[0], Y[0])):
        with pytest.raises(ValueError):
            mm.procrustes(*bad)
    with pytest.raises(ValueError):
        mm.procrustes(X, Y, reflection="worst")


def test_transform_is_align_pred_to_gt(g):
    """``align_pred_to_gt``: the Procrustes transform applied to all vertices, in the kernel's operation order (tests/mesh_metrics_ref.transformed); the
    source rounds the result to float32."""
    pv, pl, gl = mr.align_inputs()
    T, s = mm.similarity_transform(mm.procrustes(gl, pl)[2])
    got = mr.transformed(pv, T, s)
    want = g["align.vertices"]
    assert want.dtype == np.float32 and got.shape == want.shape
    assert np.abs(got - want.astype(np.float64)).max() <= 2.0 ** -24 * np.abs(want).max() * 1.01  # half a float32 ulp of the largest coordinate
    with pytest.raises(ValueError):
        mm.similarity_transform({"rotation": np.eye(2), "scale": 1.0, "translation": np.zeros(2)})


def test_landmarks(g):
    vertices, faces, idx, b = mr.embedding_inputs()
    close(mm.landmarks_from_embedding(vertices, faces, idx, b), g["embedding.landmarks"], "landmarks")
    close(mm.landmarks_from_embedding(vertices[1], faces, idx, b), g["embedding.landmarks"][1], "landmarks of one mesh")
    assert mm.landmarks_from_embedding(vertices.astype(np.float32), faces, idx, b).dtype == np.float32
    assert tuple(g["seven_of_68"].tolist()) == mm.SEVEN_OF_68
    for bad in ((vertices, faces, idx + 150, b), (vertices, faces + 90, idx, b), (vertices, faces, idx, b[:5]), (vertices[..., :2], faces, idx, b),
                (vertices, faces.astype(np.float64), idx, b)):
        with pytest.raises(ValueError):
            mm.landmarks_from_embedding(*bad)


def test_rotation_errors(g):
    Rp, Rg = mr.rotation_inputs()
    rot, ang = mm.rotation_errors(Rp, Rg)
    close(rot, g["rotation.rot_error"], "rot_error")
    close(ang, g["rotation.angle_error"], "angle_error")
    r1, a1 = mm.rotation_errors(Rp[3], Rg[3])
    assert r1 == rot[3] and a1 == ang[3]
    same = mm.rotation_errors(Rg, Rg)
    assert np.abs(same[0]).max() < 1e-14 and np.abs(same[1]).max() < 1e-6
    with pytest.raises(ValueError):
        mm.rotation_errors(Rp, Rg[:5])
    with pytest.raises(ValueError):
        mm.rotation_errors(Rp[:, :2], Rg[:, :2])


def test_nme_2d_and_collection():
    rng = np.random.default_rng(8)
    gt = rng.uniform(0, 200, size=(3, 68, 2))
    pred = gt + rng.normal(0, 2, size=gt.shape)
    norm = np.array([150.0, 90.0, 210.0])
    want = np.array([np.mean(np.linalg.norm(gt[h] - pred[h], 2, -1) / norm[h]) * 100.0 for h in range(3)])
    close(mm.nme_2d(pred, gt, norm), want, "nme_2d")
    close(mm.nme_2d(pred[1], gt[1], 90.0), want[1], "nme_2d of one head")
    for bad in ((pred, gt[:2], norm), (pred, gt, norm[:2]), (pred, gt, np.array([1.0, 0.0, 1.0])), (pred[..., :1], gt[..., :1], norm)):
        with pytest.raises(ValueError):
            mm.nme_2d(*bad)
    m = mm.HeadMeshMetrics(nme_2d=want, z_n=np.array([0.5, 1.0, 0.75]))
    mean = m.mean()
    assert tuple(mean) == ("nme_2d", "z_n", "rot_error", "angle_error", "chamfer") and len(m) == 3
    assert mean["z_n"] == 0.75 and mean["nme_2d"] == float(want.mean()) and np.isnan(mean["chamfer"]) and np.isnan(mean["rot_error"])
    assert all(np.isnan(v) for v in mm.HeadMeshMetrics().mean().values()) and len(mm.HeadMeshMetrics()) == 0


def test_argument_errors_need_no_gpu():
    """Everything is validated before a GPU is looked for."""
    pts = np.zeros((2, 8, 3), dtype=np.float32)
    for bad in (dict(top_k=8), dict(top_k=0), dict(top_k=17), dict(neighbours="intended")):
        with pytest.raises(ValueError):
            mm.z_order_accuracy(pts, pts, **bad)
    with pytest.raises(ValueError):
        mm.z_order_accuracy(pts[:, :5], pts[:, :5])  # N = 5 < top_k + 1: the source would index out of range
    with pytest.raises(ValueError):
        mm.z_order_accuracy(pts[:1], pts)
    with pytest.raises(ValueError):
        mm.z_order_accuracy(pts[..., :2], pts[..., :2])
    with pytest.raises(ValueError):
        mm.z_order_accuracy(pts[0], pts[:1])
    for bad in (dict(transform=np.zeros((3, 3))), dict(query_scale=np.ones(3)), dict(point_scale=2.0), dict(transform=np.zeros((3, 3, 4)))):
        with pytest.raises(ValueError):
            mm.nearest_points(pts, pts, **bad)
    with pytest.raises(ValueError):
        mm.nearest_points(pts[:, :0], pts)
    with pytest.raises(ValueError):
        mm.nearest_points(pts, pts[:1])
    l7 = np.arange(42, dtype=np.float64).reshape(2, 7, 3) ** 1.5
    for bad in (dict(inter_eye=(1, 1)), dict(inter_eye=(1, 7)), dict(gt_subset=[8]), dict(gt_subset=[]), dict(gt_subset=[0.5])):
        with pytest.raises(ValueError):
            mm.chamfer_to_gt(pts, pts, l7, l7, **bad)
    with pytest.raises(ValueError):
        mm.chamfer_to_gt(pts, pts, l7[:1], l7)
    with pytest.raises(ValueError):
        mm.chamfer_to_gt(pts, pts, np.zeros((2, 7, 3)), l7)  # no inter-eye distance
    result = PredictionResult(np.zeros((4, 4, 3), dtype=np.uint8), [])
    with pytest.raises(ValueError):
        result.compare_meshes(pts)  # two meshes for no head
    with pytest.raises(ValueError):
        result.compare_meshes(pts[:0], gt_landmarks7=l7[:0])


def test_binding_matches_the_header():
    """Every export of include/vgh_eval.h is bound, the constants agree, and no other library of the package exports a vghev_ symbol."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "vgh_eval.h")).read()
    assert set(re.findall(r"VGHEV_API [^;]*?(vghev_\w+)\(", header)) == set(_lib_eval.SYMBOLS)
    consts = dict(re.findall(r"#define (VGHEV_\w+) (-?\(?-?\d+\)?)", header))
    assert int(consts["VGHEV_MAX_HEADS"]) == _lib_eval.MAX_HEADS and int(consts["VGHEV_MAX_POINTS"]) == _lib_eval.MAX_POINTS
    assert int(consts["VGHEV_MAX_TOP_K"]) == _lib_eval.MAX_TOP_K
    assert {k: int(consts[f"VGHEV_NEIGHBOURS_{k.upper()}"]) for k in _lib_eval.NEIGHBOURS} == _lib_eval.NEIGHBOURS
    lib = _lib_eval.load()
    assert lib.vghev_version().startswith(b"vgheval")
    # the checks of both entry points need no GPU
    job = _lib_eval.ZOrderJob()
    job.n_heads, job.n_points, job.top_k, job.mode = 1, 5, 5, 0
    assert lib.vghev_z_order(job, None) == -1 and b"n_points" in lib.vghev_last_error()
    job.n_points, job.mode = 6, 2
    assert lib.vghev_z_order(job, None) == -1 and b"mode" in lib.vghev_last_error()
    job.mode = 0
    assert lib.vghev_z_order(job, None) == -1 and b"NULL" in lib.vghev_last_error()
    job.n_heads = 0
    assert lib.vghev_z_order(job, None) == 0
    near = _lib_eval.NearestJob()
    near.n_heads, near.n_queries, near.n_points = 1, 0, 4
    assert lib.vghev_nearest(near, None) == -1 and b"n_queries" in lib.vghev_last_error()
    near.n_queries = 3
    assert lib.vghev_nearest(near, None) == -1 and b"NULL" in lib.vghev_last_error()
    near.n_heads = 0
    assert lib.vghev_nearest(near, None) == 0
