"""Mesh benchmark metrics on the MI355X: csrc/mesh_metrics.hip (libvgheval.so) against the float64 restatement tests/mesh_metrics_ref.py and, where
recorded (tests/golden/mesh_metrics.npz), against the reference's own ``calc_zn``.  Every comparison is np.array_equal: counts, indices and float64
distances are exact by construction, so there is no tolerance anywhere."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_metrics_ref as mr  # noqa: E402

from head_detector_amd import mesh_metrics as mm  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu

Z_SIZES = (6, 7, 63, 64, 65, 257, 2470)  # top_k + 1, odd sizes, one lane short of / exactly / one past a wave, past one workgroup, the benchmark's size
Q_SIZES = (1, 65, 2094)
P_SIZES = (1, 64, 300, 5023)  # one point, below / not a multiple of / many times the 512-point LDS tile


@pytest.fixture(scope="module")
def g():
    return np.load(mr.GOLDEN)


@pytest.fixture(scope="module")
def v_template():
    return np.load(os.path.join(os.path.dirname(mr.GOLDEN), "flame_decode.npz"))["v_template"]


def cloud(kind, count, seed):
    """float32 [count, 3].  "lattice": small integers, so that many distances tie exactly and some points coincide: the order is then decided by index."""
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        return rng.integers(-4, 5, size=(count, 3)).astype(np.float32)
    return rng.normal(0.0, 60.0, size=(count, 3)).astype(np.float32)


_partners = {}


def z_case(N):
    """(pred, gt float32 [3, N, 3], {mode: partners int64 [3, N, 5]}): a Gaussian cloud, a lattice and a second cloud; computed once per size."""
    if N not in _partners:
        gt = np.stack([cloud("normal", N, N), cloud("lattice", N, N + 1), cloud("normal", N, N + 2)])
        pred = (gt + np.random.default_rng(N + 3).normal(0.0, 25.0, size=gt.shape)).astype(np.float32)
        pred[1] = np.random.default_rng(N + 4).integers(-2, 3, size=pred[1].shape)  # equal predicted depths too
        top = min(5, N - 1)
        _partners[N] = (pred, gt, {mode: np.stack([mr.partners(h, top, mode) for h in gt]) for mode in ("reference", "nearest")})
    return _partners[N]


def counts(pred, gt, partners):
    gz, pz = gt[..., 2], pred[..., 2]
    take = np.take_along_axis
    p = partners.reshape(len(gt), gt.shape[1] * partners.shape[2])  # no -1: with no head the size is 0 and cannot be inferred
    ok = (np.repeat(gz, partners.shape[2], axis=1) >= take(gz, p, 1)) == (np.repeat(pz, partners.shape[2], axis=1) >= take(pz, p, 1))
    return ok.sum(axis=1).astype(np.int32)


@pytest.mark.parametrize("N", Z_SIZES)
def test_z_order_against_the_restatement(gpu_lib, N):
    pred, gt, partners = z_case(N)
    before = pred.copy(), gt.copy()
    for n in (0, 1, 3):
        for top_k in (1, 5):
            if N < top_k + 1:
                continue
            for mode in ("reference", "nearest"):
                ratio, count = mm.z_order_accuracy(pred[:n], gt[:n], top_k, mode)
                want = counts(pred[:n], gt[:n], partners[mode][:n, :, :top_k])
                print(N, n, top_k, mode, count.tolist(), want.tolist())
                assert count.dtype == np.int32 and ratio.dtype == np.float64 and count.shape == (n,) and ratio.shape == (n,)
                assert np.array_equal(count, want), (N, n, top_k, mode)
                assert np.array_equal(ratio, want.astype(np.float64) / float(N * top_k))
    assert np.array_equal(pred, before[0]) and np.array_equal(gt, before[1])


def test_z_order_other_top_k(gpu_lib):
    """Every register count of the streaming search is a kernel of its own: top_k = 2, 8 and the largest, 16."""
    pred, gt, _ = z_case(257)
    for top_k in (2, 8, 16):
        for mode in ("reference", "nearest"):
            assert np.array_equal(mm.z_order_accuracy(pred, gt, top_k, mode)[1], mr.z_order(pred, gt, top_k, mode)[1]), (top_k, mode)


@pytest.mark.parametrize("name", mr.ZN_CASES)
def test_z_order_is_the_references_calc_zn(gpu_lib, g, v_template, name):
    """The recorded value of the reference's own function on template vertices in millimetres plus jitter, all 2 470 head vertices included."""
    pred, gt = mr.zn_inputs(name, g[f"zn.{name}.seeds"], v_template, g["head_indices"].astype(np.int64))
    ratio, count = mm.z_order_accuracy(pred, gt, 5, "reference")
    value = float(g[f"zn.{name}.value"])
    print(name, count.tolist(), value)
    assert round(value * len(gt) * gt.shape[1] * 5) == int(count.sum())
    assert abs(float(ratio.mean()) - value) < 1e-6
    assert np.array_equal(count, mr.z_order(pred, gt, 5, "reference")[1])


def test_z_order_planted(gpu_lib):
    pred, gt, _ = z_case(65)
    N = 65
    for mode in ("reference", "nearest"):
        for top_k in (1, 5):
            assert mm.z_order_accuracy(gt, gt, top_k, mode)[0].tolist() == [1.0, 1.0, 1.0]  # pred = gt
            flat_p, flat_g = pred.copy(), gt.copy()
            flat_p[..., 2], flat_g[..., 2] = 3.0, -7.0
            assert mm.z_order_accuracy(flat_p, flat_g, top_k, mode)[0].tolist() == [1.0, 1.0, 1.0]  # all z equal: >= holds on both sides
        # distinct depths in reversed order: only a vertex that is its own partner agrees
        own = int((mr.partners(gt[0], 5, mode) == np.arange(N)[:, None]).sum())
        assert mm.z_order_accuracy(-gt[0], gt[0], 5, mode)[1].tolist() == [own]
    # duplicated points resolve by index: points 3 and 40 coincide, so do 10, 11 and 12
    dup = gt[0].copy()
    dup[40] = dup[3]
    dup[11] = dup[12] = dup[10]
    p = (dup + np.random.default_rng(1).normal(0.0, 30.0, size=dup.shape)).astype(np.float32)
    near = mr.partners(dup, 5, "nearest")
    assert near[3][0] == 40 and near[40][0] == 40 and near[10][:2].tolist() == [11, 12] and near[12][:2].tolist() == [11, 12]
    for mode in ("reference", "nearest"):
        assert np.array_equal(mm.z_order_accuracy(p, dup, 5, mode)[1], mr.z_order(p[None], dup[None], 5, mode)[1]), mode


def test_z_order_tensors_and_determinism(gpu_lib):
    pred, gt, partners = z_case(257)
    dev = torch.device("cuda", torch.cuda.current_device())
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    keep_p, keep_g = tp.clone(), tg.clone()
    for mode in ("reference", "nearest"):
        ratio, count = mm.z_order_accuracy(tp, tg, 5, mode, to_host=False)
        assert ratio.is_cuda and count.is_cuda and count.dtype == torch.int32 and ratio.dtype == torch.float64
        want = counts(pred, gt, partners[mode])
        assert np.array_equal(count.cpu().numpy(), want)
        again = mm.z_order_accuracy(tp, tg, 5, mode, to_host=False)
        assert torch.equal(again[1], count) and torch.equal(again[0], ratio)
        # float64 inputs are converted to what the kernel reads; one head may come as [N, 3]
        assert np.array_equal(mm.z_order_accuracy(pred.astype(np.float64), tg.double(), 5, mode)[1], want)
        assert mm.z_order_accuracy(pred[2], gt[2], 5, mode)[1].tolist() == [int(want[2])]
    assert torch.equal(tp, keep_p) and torch.equal(tg, keep_g)


# ---- nearest ------------------------------------------------------------------------------------------------------------------------------------------
def near_case(M, P):
    """Two heads: a Gaussian cloud against a Gaussian cloud, and a lattice against a lattice (ties, coinciding points, queries that ARE points)."""
    query = np.stack([cloud("normal", M, 7 * M + P), cloud("lattice", M, 7 * M + P + 1)])
    points = np.stack([cloud("normal", P, 11 * P + M), cloud("lattice", P, 11 * P + M + 1)])
    rng = np.random.default_rng(M + P)
    Q, _ = np.linalg.qr(rng.normal(size=(2, 3, 3)))
    T = np.concatenate([Q.transpose(0, 2, 1), rng.normal(0.0, 10.0, size=(2, 3, 1))], axis=2)
    T[1] = np.array([[0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, -1.0, 0.0]])  # the lattice stays a lattice: the ties survive the transform
    return query, points, T, np.array([1.0 / 3.0, 2.0]), np.array([0.7310585786300049, 0.5])


def same_nearest(got, want, what):
    for name, a, b, dtype in zip(("sqdist", "index", "mean"), got, want, (np.float64, np.int32, np.float64)):
        assert a.dtype == dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()))


@pytest.mark.parametrize("M", Q_SIZES)
def test_nearest_against_the_restatement(gpu_lib, M):
    for P in P_SIZES:
        query, points, T, qs, ps = near_case(M, P)
        before = query.copy(), points.copy(), T.copy()
        same_nearest(mm.nearest_points(query, points), mr.nearest(query, points), (M, P, "plain"))
        got = mm.nearest_points(query, points, transform=T, query_scale=qs, point_scale=ps)
        same_nearest(got, mr.nearest(query, points, T, qs, ps), (M, P, "transform, both scales"))
        assert (got[1] >= 0).all() and (got[1] < P).all()
        if P == 300:
            same_nearest(mm.nearest_points(query, points, transform=T), mr.nearest(query, points, T), (M, P, "transform alone"))
            same_nearest(mm.nearest_points(query, points, query_scale=qs), mr.nearest(query, points, None, qs), (M, P, "query scale alone"))
            same_nearest(mm.nearest_points(query, points, transform=T[0], query_scale=2.0), mr.nearest(query, points, T[[0, 0]], np.array([2.0, 2.0])),
                         (M, P, "one transform and one scale for all heads"))
        assert np.array_equal(query, before[0]) and np.array_equal(points, before[1]) and np.array_equal(T, before[2])


def test_nearest_planted_tensors_and_determinism(gpu_lib):
    query, points, T, qs, ps = near_case(65, 300)
    # a query equal to a point gives distance 0 at that index; where points coincide, at the lowest of them
    points[0, 200] = points[0, 17]
    query[0, 5], query[0, 6] = points[0, 200], points[0, 299]
    sq, idx, mean = mm.nearest_points(query, points)
    assert sq[0, 5] == 0.0 and idx[0, 5] == 17 and sq[0, 6] == 0.0 and idx[0, 6] == 299
    same_nearest((sq, idx, mean), mr.nearest(query, points), "planted")
    lattice_ties = sum(int((mr.sqdist(query[1, m:m + 1], points[1])[0] == sq[1, m]).sum() > 1) for m in range(65))
    assert lattice_ties > 30  # the lattice head decides most queries by index
    # no heads; one head as [M, 3]
    empty = mm.nearest_points(query[:0], points[:0])
    assert [a.shape for a in empty] == [(0, 65), (0, 65), (0,)]
    one = mm.nearest_points(query[1], points[1], transform=T[1], query_scale=qs[1], point_scale=ps[1])
    want = mr.nearest(query[1:], points[1:], T[1:], qs[1:], ps[1:])
    same_nearest(one, tuple(a[0] for a in want), "one head")
    # GPU tensors in, GPU tensors out, nothing written, bitwise repeatable
    dev = torch.device("cuda", torch.cuda.current_device())
    tq, tp = torch.from_numpy(query).to(dev), torch.from_numpy(points).to(dev)
    keep_q, keep_p = tq.clone(), tp.clone()
    a = mm.nearest_points(tq, tp, transform=T, query_scale=qs, point_scale=ps, to_host=False)
    b = mm.nearest_points(tq, tp, transform=T, query_scale=qs, point_scale=ps, to_host=False)
    assert all(x.is_cuda and torch.equal(x, y) for x, y in zip(a, b))
    same_nearest(tuple(x.cpu().numpy() for x in a), mr.nearest(query, points, T, qs, ps), "tensors")
    assert torch.equal(tq, keep_q) and torch.equal(tp, keep_p)


def test_chamfer_to_gt(gpu_lib, v_template):
    """Steps 1-4 of ``chamfer_to_gt`` restated with tests/mesh_metrics_ref.py at the benchmark's size (a 2 094-vertex subset against 5 023 vertices); a
    prediction that is a similarity transform of the ground truth has chamfer ~ 0."""
    rng = np.random.default_rng(77)
    gt = np.stack([v_template * 1000.0, v_template * 870.0 + 3.0]).astype(np.float32)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    pred = ((gt.astype(np.float64) @ Q) * 2.5 + np.array([300.0, 200.0, -50.0]) + rng.normal(0.0, 1.5, size=gt.shape)).astype(np.float32)
    seven = rng.choice(5023, size=7, replace=False)
    subset = np.sort(rng.choice(5023, size=2094, replace=False))
    gl, pl = gt[:, seven].astype(np.float64), pred[:, seven].astype(np.float64)
    before = gt.copy(), pred.copy()
    got = mm.chamfer_to_gt(gt, pred, gl, pl, gt_subset=subset)
    scale = 20.0 / np.linalg.norm(gl[:, 1] - gl[:, 2], axis=1)
    tf = [mm.similarity_transform(mm.procrustes(scale[h] * gl[h], pl[h])[2]) for h in range(2)]
    want = mr.nearest(gt[:, subset], pred, np.stack([t for t, _ in tf]), scale, np.array([s for _, s in tf]))[2]
    print(got.tolist(), want.tolist())
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(gt, before[0]) and np.array_equal(pred, before[1])
    assert np.array_equal(mm.chamfer_to_gt(gt[1], pred[1], gl[1], pl[1], gt_subset=subset), want[1])
    exact = ((gt.astype(np.float64) @ Q) * 2.5 + np.array([300.0, 200.0, -50.0])).astype(np.float32)
    assert (mm.chamfer_to_gt(gt, exact, gl, exact[:, seven]) < 1e-6).all()  # mm^2 at a head 20 mm between the eyes: float32 rounding of the vertices


def test_compare_meshes(gpu_lib, g, v_template):
    """A PredictionResult of three heads: z_n on the reference's head_indices in both readings, chamfer when landmarks are given; nothing is modified."""
    head_indices = g["head_indices"].astype(np.int64)
    pairs = [mr.jittered(v_template * 1000.0, seed) for seed in (1, 2, 3)]
    gt = np.stack([a for a, _ in pairs])
    heads = [types.SimpleNamespace(vertices_3d=b.copy()) for _, b in pairs]
    result = PredictionResult(np.zeros((8, 8, 3), dtype=np.uint8), heads)
    for mode in ("reference", "nearest"):
        m = result.compare_meshes(gt, subset=head_indices, neighbours=mode)
        want = mr.z_order(np.stack([b for _, b in pairs])[:, head_indices], gt[:, head_indices], 5, mode)
        assert isinstance(m, mm.HeadMeshMetrics) and len(m) == 3 and m.chamfer is None
        assert np.array_equal(m.z_n_count, want[1]) and np.array_equal(m.z_n, want[0])
        assert m.mean()["z_n"] == float(want[0].mean()) and np.isnan(m.mean()["chamfer"])
    whole = result.compare_meshes(gt, top_k=1, to_host=False)
    assert whole.z_n.is_cuda and np.array_equal(whole.z_n_count.cpu().numpy(), mr.z_order(np.stack([b for _, b in pairs]), gt, 1, "reference")[1])
    seven = np.array([3500, 3600, 3700, 3800, 3900, 4000, 4100])
    gl, pl = gt[:, seven], np.stack([b for _, b in pairs])[:, seven]
    both = result.compare_meshes(gt, subset=head_indices, gt_landmarks7=gl, pred_landmarks7=pl, chamfer_subset=head_indices[:500])
    assert np.array_equal(both.chamfer, mm.chamfer_to_gt(gt, np.stack([b for _, b in pairs]), gl, pl, gt_subset=head_indices[:500]))
    assert both.chamfer.shape == (3,) and (both.chamfer > 0).all() and both.mean()["chamfer"] == float(both.chamfer.mean())
    for h, (_, b) in zip(heads, pairs):
        assert np.array_equal(h.vertices_3d, b)
    none = PredictionResult(np.zeros((8, 8, 3), dtype=np.uint8), []).compare_meshes(gt[:0], subset=head_indices)
    assert len(none) == 0 and none.z_n.shape == (0,) and np.isnan(none.mean()["z_n"])
