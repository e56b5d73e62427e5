"""Aligned head crops on the MI355X: csrc/aligned.hip (libvghview.so) through PredictionResult.get_aligned_heads, bit for bit against the
fixture recorded from the reference (tests/golden/aligned_heads.npz) and against the CPU restatement of the warp (tests/warp_affine_ref.py).
The fixture pins the planner; in the other tests the restatement is driven by the planner's own matrices and pins the pixels."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import warp_affine_ref as war  # noqa: E402
from aligned_fixture import fixture_crops, fixture_heads, formula_image, load_fixture  # noqa: E402

from head_detector_amd import aligned  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.head_info import RPY  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _restated(image: np.ndarray, plans):
    out = []
    for p in plans:
        x0, y0, x1, y1 = p.region
        if x1 <= x0 or y1 <= y0:
            out.append(np.zeros(p.shape, dtype=np.uint8))
        else:
            out.append(war.warp_affine(image, p.matrix, p.bounds, region=p.region))
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == b.shape, (what, i, a.shape, b.shape)
        assert np.array_equal(a, b), (what, i, int((a != b).sum()))


def test_get_aligned_heads_equals_the_reference(gpu_lib):
    """Count, shapes (the empty ones included) and bytes of what the reference's own get_aligned_heads returned."""
    g = load_fixture()
    crops = fixture_crops(g)
    for letter in "AB":
        picked = fixture_heads(g, letter)
        img = formula_image(*(int(v) for v in g[f"shape_{letter}"]))
        before = img.copy()
        got = PredictionResult(img, [h for _, _, h in picked], head_indices=g["head_indices"]).get_aligned_heads()
        _assert_same(got, [crops[i] for i, _, _ in picked], letter)
        assert np.array_equal(img, before)
    assert any(c.size == 0 for c in crops) and sum(c.size > 0 for c in crops) >= 10


def _random_heads(rng, n, H, W, V=300):
    heads = []
    for k in range(n):
        cx, cy = rng.uniform(-40, W + 40), rng.uniform(-40, H + 40)  # some heads hang over an edge: clipped and empty crops occur
        rx, ry = rng.uniform(20, 260, 2)
        ang, rad = rng.uniform(0, 2 * np.pi, V), np.sqrt(rng.uniform(0, 1, V))
        v = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang), rng.normal(0, 20, V)], axis=1).astype(np.float32)
        # a translation (padded-640 space) that puts the centre of rotation within ~200 px of the head, so that rotated crops show the image, not its border
        s = 640 / max(H, W)
        t = torch.tensor([[(cx + rng.uniform(-200, 200)) * s + (640 - int(W * s)), (cy + rng.uniform(-200, 200)) * s + (640 - int(H * s)), 0.0]], dtype=torch.float32)
        yaw = rng.uniform(-90, 90)
        roll = float(rng.choice([0.0, 90.0, -90.0, 180.0])) if k % 10 == 0 else rng.uniform(-180, 180)
        heads.append(types.SimpleNamespace(vertices_3d=v, flame_params=types.SimpleNamespace(translation=t), head_pose=RPY(roll=roll, pitch=0.0, yaw=yaw)))
    return heads


def test_hundred_heads_on_a_large_pitched_image(gpu_lib):
    """3000 x 4000, 100 heads with random poses, the source a strided view of a wider GPU tensor; the restatement is evaluated on each crop's region only."""
    H, W, n = 3000, 4000, 100
    gen = torch.Generator().manual_seed(7)
    wide = torch.randint(0, 256, (H, W + 37, 3), dtype=torch.uint8, generator=gen).to(_dev())
    view = wide[:, :W]
    assert view.stride(0) > 3 * W
    img = view.cpu().numpy()
    rng = np.random.default_rng(11)
    heads = _random_heads(rng, n, H, W)
    hidx = np.sort(rng.choice(300, 120, replace=False))
    plans = aligned.aligned_head_plan(img.shape, heads, hidx)
    want = _restated(img, plans)
    assert sum(p.rotated for p in plans) >= 30 and sum(not p.rotated for p in plans) >= 10 and sum(w.size > 0 for w in want) >= 60
    assert sum(bool(w.any()) for w, p in zip(want, plans) if p.rotated) >= 40  # rotated crops that show the image
    got = PredictionResult(view, heads, head_indices=hidx).get_aligned_heads()
    _assert_same(got, want, "pitched view")
    _assert_same(PredictionResult(img, heads, head_indices=hidx).get_aligned_heads(), want, "numpy image")
    for bad in (wide.permute(1, 0, 2)[:W, :H], wide[:, :, :2], wide[:8].float()):
        with pytest.raises(ValueError):
            aligned.warp_crops(bad, [(plans[0].matrix, (0, 0, 8, 8))])


def test_vertically_align_device_results_and_no_heads(gpu_lib):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (333, 517, 3), dtype=np.uint8)
    v = rng.uniform(0, 300, (300, 3)).astype(np.float32)
    for roll, t in ((23.4, (260.0, 300.0)), (-131.0, (100.5, 420.25)), (90.0, (320.0, 320.0)), (0.0, (17.0, 600.0))):
        fp = types.SimpleNamespace(translation=torch.tensor([[t[0], t[1], 0.0]]))
        out, lm = aligned.vertically_align(img, v, fp, roll)
        m, bounds = aligned.get_rotation_mat(img, aligned.flame_params_skull_center(fp, img), roll)
        want = war.warp_affine(img, m, bounds)
        assert out.shape == (bounds[1], bounds[0], 3) and np.array_equal(out, want), roll
        assert lm.shape == (300, 2) and lm.dtype == np.float64 and np.array_equal(lm, np.hstack([v[:, :2], np.ones((300, 1))]) @ m.T)
    heads = _random_heads(rng, 12, 333, 517)
    hidx = np.arange(0, 300, 3)
    res = PredictionResult(img, heads, head_indices=hidx)
    on_host, on_dev = res.get_aligned_heads(), res.get_aligned_heads(to_host=False)
    assert len(on_dev) == len(on_host) == 12
    for a, b in zip(on_host, on_dev):
        assert isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.uint8 and tuple(b.shape) == a.shape
        assert np.array_equal(a, b.cpu().numpy())
    _assert_same(on_host, _restated(img, aligned.aligned_head_plan(img.shape, heads, hidx)), "small image")
    assert PredictionResult(img, [], head_indices=hidx).get_aligned_heads() == []
    assert PredictionResult(img, [], head_indices=hidx).get_aligned_heads(to_host=False) == []
    with pytest.raises(FileNotFoundError):
        PredictionResult(img, heads).get_aligned_heads()


def test_consecutive_calls_of_different_sizes_on_one_stream(gpu_lib):
    """Three calls queued on one non-default stream with nothing waited for in between: one head with a small crop, three heads (the staging block regrows
    while the first call's work may still be queued: the library waits for its event before it frees it), the first call again (in the grown block).
    A device image in, device crops out, one synchronisation at the end; every crop is the restatement's for its own inputs."""
    rng = np.random.default_rng(29)
    H, W = 200, 260
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    hidx = np.arange(0, 300, 3)

    def head(cx, cy, r, roll):
        ang, rad = rng.uniform(0, 2 * np.pi, 300), np.sqrt(rng.uniform(0, 1, 300))
        v = np.stack([cx + r * rad * np.cos(ang), cy + r * rad * np.sin(ang), rng.normal(0, 5, 300)], axis=1).astype(np.float32)
        s = 640 / max(H, W)
        t = torch.tensor([[cx * s + (640 - int(W * s)), cy * s + (640 - int(H * s)), 0.0]], dtype=torch.float32)
        return types.SimpleNamespace(vertices_3d=v, flame_params=types.SimpleNamespace(translation=t), head_pose=RPY(roll=roll, pitch=0.0, yaw=10.0))

    one = [head(60.0, 50.0, 9.0, 25.0)]
    three = [head(130.0, 100.0, 70.0, -40.0), head(200.0, 60.0, 45.0, 0.0), head(100.0, 110.0, 40.0, 90.0)]
    calls = [one, three, one]
    want = [_restated(img, aligned.aligned_head_plan(img.shape, heads, hidx)) for heads in calls]
    assert all(c.size > 0 and c.any() for w in want for c in w) and sum(c.size for c in want[1]) > 20 * sum(c.size for c in want[0])
    src = torch.from_numpy(img).to(_dev())
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = [PredictionResult(src, heads, head_indices=hidx).get_aligned_heads(to_host=False) for heads in calls]
    stream.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert all(isinstance(c, torch.Tensor) and c.is_cuda for c in g)
        _assert_same([c.cpu().numpy() for c in g], w, "ABC"[k])
    _assert_same([c.cpu().numpy() for c in got[0]], [c.cpu().numpy() for c in got[2]], "A == C")


def test_aligned_heads_through_the_facade(gpu_lib, flame_model):
    """HeadDetector(..., mesh_assets=...).detect_batch on two images of different sizes: one crop per head, equal to the restatement driven by the
    same heads.  With synthetic weights the meshes are meaningless and crops may be empty or clipped: the assertion is equality, not plausibility."""
    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.pncc import MeshAssets

    V = 5023
    rng = np.random.default_rng(3)
    faces = np.asarray(flame_model["f"]).astype(np.int64)
    subset = np.sort(rng.choice(V, 3000, replace=False))
    assets = MeshAssets(faces, np.asarray(flame_model["v_template"], dtype=np.float64), subset, subset[:500])
    det = HeadDetector("vgg_heads_m", 320, flame_model=flame_model, weights="synthetic", seed=4, mesh_assets=assets, max_batch=2)
    imgs = [rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((300, 320, 3), (411, 275, 3))]
    image, _ = det._preprocess(imgs[0])
    conf = float(det._process(image)[1][0, 6, 0])
    results = det.detect_batch(imgs, confidence_threshold=conf)
    assert len(results) == 2 and sum(len(r.heads) for r in results) >= 2
    for im, res in zip(imgs, results):
        got = res.get_aligned_heads()
        assert len(got) == len(res.heads)
        _assert_same(got, _restated(im, aligned.aligned_head_plan(im.shape, res.heads, subset[:500])), im.shape)
    single = det(imgs[0], confidence_threshold=conf)
    assert len(single.get_aligned_heads()) == len(single.heads) >= 1
    with pytest.raises(FileNotFoundError):
        HeadDetector("vgg_heads_m", 320, flame_model=flame_model, weights="synthetic", seed=4)(imgs[0], confidence_threshold=conf).get_aligned_heads()
