"""PredictionResult.draw on the MI355X: csrc/draw.hip (libvghview.so), byte for byte against the fixture recorded from the reference's own draw
(tests/golden/draw_heads.npz) and against the CPU restatement of the drawing rules (tests/draw_ref.py) driven by the product's own plan.
Every comparison is np.array_equal.  Parity of the restatement with cv2 itself is UNPINNED where cv2 is absent (tests/test_draw_host.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import draw_ref  # noqa: E402
from draw_fixture import METHODS, expected, fixture_assets, fixture_heads, fixture_image, fixture_result, load_fixture, make_head, render_plan  # noqa: E402

from head_detector_amd import draw  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _same(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape, (what, getattr(got, "shape", None))
    assert np.array_equal(got, want), (what, int((got != want).any(axis=2).sum()), "pixels differ")


def test_draw_equals_the_reference(gpu_lib):
    """All four methods on both fixture images: the bytes the reference's own PredictionResult.draw returned; the input is not modified."""
    g = load_fixture()
    for letter in "AB":
        img = fixture_image(g, letter)
        before = img.copy()
        res = PredictionResult(img, fixture_heads(g, letter), **fixture_assets(g))
        for m in METHODS:
            got = res.draw(m)
            _same(got, fixture_result(g, letter, m), (letter, m))
            assert got is not img and not np.shares_memory(got, img)
        _same(res.draw(), fixture_result(g, letter, "full"), (letter, "default method"))
        assert np.array_equal(img, before)


V, T = 5023, 4816
COLS = 71  # 71 * 71 >= V


def _topology(rng):
    """Triangles over neighbouring vertices of a 71-column boustrophedon grid (edges of about one grid cell, like a real mesh), and 116 triangles of
    arbitrary vertices (edges as long as the head: the wave-cooperative path of the wire kernel)."""
    i = rng.integers(0, V - COLS - 1, 4700)
    local = np.stack([i, i + 1, i + COLS + rng.integers(-1, 2, 4700)], axis=1)
    tri = np.concatenate([local, rng.integers(0, V, (T - 4700, 3))]).astype(np.int32)
    head_idx = np.sort(rng.choice(V, 2470, replace=False))
    face_idx = np.sort(rng.choice(V, 2094, replace=False))
    return tri, head_idx, face_idx


def _grid_heads(rng, n, H, W, lo=40.0, hi=1500.0):
    """Heads of lo .. hi pixels, their centres anywhere up to a tenth of the image outside it, vertices on a jittered grid inside an ellipse."""
    k = np.arange(V)
    row, col = k // COLS, k % COLS
    col = np.where(row % 2 == 1, COLS - 1 - col, col)
    heads = []
    for _ in range(n):
        size = rng.uniform(lo, hi)
        cx, cy = rng.uniform(-0.1 * W, 1.1 * W), rng.uniform(-0.1 * H, 1.1 * H)
        u = (col + rng.uniform(-0.4, 0.4, V)) / (COLS - 1) - 0.5
        v = (row + rng.uniform(-0.4, 0.4, V)) / (COLS - 1) - 0.5
        xyz = np.stack([cx + size * u, cy + 1.2 * size * v, rng.normal(0, 20, V)], axis=1).astype(np.float32)
        x0, y0, x1, y1 = (int(q) for q in (xyz[:, 0].min(), xyz[:, 1].min(), xyz[:, 0].max(), xyz[:, 1].max()))
        heads.append(make_head(xyz, (x0, y0, x1 - x0, y1 - y0)))
    return heads


def test_hundred_heads_on_a_large_pitched_image(gpu_lib):
    """3000 x 4000 (R = 3), a strided view of a wider GPU tensor, 100 overlapping heads of 40 .. 1500 px, some hanging over the edges: "full" against the
    restatement, after showing on the CPU result that order, clipping and every edge are really exercised."""
    H, W, n = 3000, 4000, 100
    gen = torch.Generator().manual_seed(17)
    wide = torch.randint(0, 256, (H, W + 37, 3), dtype=torch.uint8, generator=gen).to(_dev())
    view = wide[:, :W]
    assert view.stride(0) > 3 * W and view.stride(0) % 4 != 0  # rows start at every byte alignment
    img = view.cpu().numpy()
    rng = np.random.default_rng(23)
    tri, head_idx, face_idx = _topology(rng)
    assets = dict(triangles=tri, head_indices=head_idx, face_indices=face_idx)
    heads = _grid_heads(rng, n, H, W)
    plan = draw.draw_plan(img.shape, heads, "full", **assets)
    assert plan.radius == 3 and plan.points.shape == (n, V, 2) and plan.triangles.shape == (T, 3)
    want = render_plan(img, plan)

    # ---- the inputs bite ----
    first = render_plan(img, plan, reverse=True)  # every pixel keeps the colour of the FIRST primitive that covered it
    order_matters = int((first != want).any(axis=2).sum())
    t = tri.astype(np.int64)
    clipped, long_segments = 0, 0
    for P in plan.points.astype(np.int64):
        a, b, c = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
        s, e = np.concatenate([c, a, b]), np.concatenate([a, b, c])
        drawn, x1, y1, x2, y2, moved = draw_ref.clip_lines(W, H, s[:, 0], s[:, 1], e[:, 0], e[:, 1])
        clipped += int(moved.sum())
        long_segments += int((drawn & (np.maximum(np.abs(x2 - x1), np.abs(y2 - y1)) >= 64)).sum())
    R = plan.radius
    c = plan.points[:, head_idx].reshape(-1, 2).astype(np.int64)
    inx, iny = (c[:, 0] >= 0) & (c[:, 0] < W), (c[:, 1] >= 0) & (c[:, 1] < H)
    dots = {"left": int((iny & (c[:, 0] - R < 0) & (c[:, 0] + R >= 0)).sum()), "right": int((iny & (c[:, 0] + R > W - 1) & (c[:, 0] - R <= W - 1)).sum()),
            "top": int((inx & (c[:, 1] - R < 0) & (c[:, 1] + R >= 0)).sum()), "bottom": int((inx & (c[:, 1] + R > H - 1) & (c[:, 1] - R <= H - 1)).sum())}
    B = plan.boxes.astype(np.int64)
    x, y, x2, y2 = B[:, 0], B[:, 1], B[:, 0] + B[:, 2], B[:, 1] + B[:, 3]
    bands = {"left": int(((x < 0) & (x2 > 0)).sum()), "right": int(((x2 > W - 1) & (x < W - 1)).sum()), "top": int(((y < 0) & (y2 > 0)).sum()),
             "bottom": int(((y2 > H - 1) & (y < H - 1)).sum())}
    print(f"order matters on {order_matters} pixels; {clipped} clipped segments; {long_segments} segments of 64+ pixels; clipped dots {dots}; clipped bands {bands}; "
          f"{int((want != img).any(axis=2).sum())} painted pixels")
    assert order_matters >= 1000 and clipped >= 50 and long_segments >= 50
    assert min(dots.values()) >= 1 and min(bands.values()) >= 1, (dots, bands)

    # ---- the pixels ----
    res = PredictionResult(view, heads, **assets)
    _same(res.draw("full"), want, "full, pitched view")
    assert np.array_equal(view.cpu().numpy(), img)
    _same(PredictionResult(img, heads, **assets).draw("full"), want, "full, numpy image")
    few = heads[:12]
    for m in ("bbox", "landmarks", "points"):
        _same(PredictionResult(view, few, **assets).draw(m), expected(img, few, m, **assets), m)


def test_device_results_sizes_and_no_stale_keys(gpu_lib):
    rng = np.random.default_rng(5)
    tri, head_idx, face_idx = _topology(rng)
    assets = dict(triangles=tri, head_indices=head_idx, face_indices=face_idx)
    # R = 2: a 2500 x 2100 image, the large one of this test
    H, W = 2500, 2100
    big = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    heads = _grid_heads(rng, 9, H, W, 60.0, 900.0)
    assert draw.draw_plan(big.shape, heads, "full", **assets).radius == 2
    want = expected(big, heads, "full", **assets)
    res = PredictionResult(big, heads, **assets)
    _same(res.draw(), want, "R = 2")
    # to_host=False: a GPU tensor, equal to the host result, not aliasing a GPU input
    src = torch.from_numpy(big).to(_dev())
    on_dev = PredictionResult(src, heads, **assets).draw("full", to_host=False)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.uint8 and tuple(on_dev.shape) == (H, W, 3)
    assert on_dev.data_ptr() != src.data_ptr() and np.array_equal(on_dev.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), big)
    # a small image right after the large one: the key plane is library scratch, every call clears what it resolves
    small = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    some = _grid_heads(rng, 3, 37, 53, 10.0, 60.0)
    for m in METHODS:
        _same(PredictionResult(small, some, **assets).draw(m), expected(small, some, m, **assets), ("small after large", m))
    _same(PredictionResult(small, some, **assets).draw("bbox"), expected(small, some, "bbox", **assets), "bbox after full: no keys left over")
    # no heads: a copy
    got = PredictionResult(small, [], **assets).draw()
    _same(got, small, "no heads")
    assert got is not small and not np.shares_memory(got, small)
    empty_dev = PredictionResult(torch.from_numpy(small).to(_dev()), []).draw("bbox", to_host=False)
    assert empty_dev.is_cuda and np.array_equal(empty_dev.cpu().numpy(), small)
    # 1 x 1, and odd sizes whose pixel count is not a multiple of four
    one = np.array([[[9, 8, 7]]], dtype=np.uint8)
    for m in METHODS:
        _same(PredictionResult(one, some, **assets).draw(m), expected(one, some, m, **assets), ("1 x 1", m))
    _same(PredictionResult(one, [make_head(np.zeros((V, 3)), (0, 0, 0, 0))], **assets).draw("bbox"), np.array([[[255, 0, 0]]], dtype=np.uint8), "1 x 1 box")
    for shape in ((3, 5, 3), (7, 2, 3), (1, 9, 3), (5, 1, 3)):
        tiny = rng.integers(0, 256, shape, dtype=np.uint8)
        hs = _grid_heads(rng, 2, shape[0], shape[1], 4.0, 12.0)
        _same(PredictionResult(tiny, hs, **assets).draw(), expected(tiny, hs, "full", **assets), shape)


def test_consecutive_calls_of_different_sizes_on_one_stream(gpu_lib):
    """Three draws queued on one non-default stream with nothing waited for in between: small (staging and key plane of a few bytes), larger (both regrow
    while the first call's work may still be queued: the library waits for its event before it frees them), the small one again (in the grown blocks).
    Device images in, device images out, one synchronisation at the end; every result is the restatement's for its own inputs."""
    rng = np.random.default_rng(41)
    tri, head_idx, face_idx = _topology(rng)
    assets = dict(triangles=tri, head_indices=head_idx, face_indices=face_idx)
    small, large = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    one, three = _grid_heads(rng, 1, 16, 16, 4.0, 12.0), _grid_heads(rng, 3, 48, 64, 10.0, 60.0)
    calls = [(small, one, "bbox"), (large, three, "full"), (small, one, "bbox")]
    want = [expected(img, heads, m, **assets) for img, heads, m in calls]
    assert all((w != img).any() for w, (img, _, _) in zip(want, calls))  # every call paints something
    on_dev = [torch.from_numpy(img).to(_dev()) for img, _, _ in calls]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = [PredictionResult(src, heads, **assets).draw(m, to_host=False) for src, (_, heads, m) in zip(on_dev, calls)]
    stream.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, torch.Tensor) and g.is_cuda
        _same(g.cpu().numpy(), w, "ABC"[k])
    assert np.array_equal(got[0].cpu().numpy(), got[2].cpu().numpy())


def test_draw_through_the_facade(gpu_lib, flame_model):
    """HeadDetector(..., mesh_assets=MeshAssets(..., triangles=, face_indices=)).detect_batch on two images of different sizes: every result's draw(m)
    equals the restatement driven by the same heads.  With synthetic weights the meshes are meaningless (they may lie mostly outside the image):
    the assertion is equality, not plausibility.  Seed 4 (the aligned-heads facade test's) keeps every vertex inside +-2**24 pixels."""
    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.pncc import MeshAssets

    rng = np.random.default_rng(3)
    faces = np.asarray(flame_model["f"]).astype(np.int64)
    subset = np.sort(rng.choice(V, 3000, replace=False))
    assets = dict(triangles=faces[:T].astype(np.int32), head_indices=subset[:500], face_indices=subset[500:900])
    mesh = MeshAssets(faces, np.asarray(flame_model["v_template"], dtype=np.float64), subset, subset[:500], triangles=assets["triangles"], face_indices=assets["face_indices"])
    det = HeadDetector("vgg_heads_m", 320, flame_model=flame_model, weights="synthetic", seed=4, mesh_assets=mesh, max_batch=2)
    imgs = [rng.integers(0, 256, shape, dtype=np.uint8) for shape in ((300, 320, 3), (411, 275, 3))]
    image, _ = det._preprocess(imgs[0])
    conf = float(det._process(image)[1][0, 6, 0])
    results = det.detect_batch(imgs, confidence_threshold=conf)
    assert len(results) == 2 and sum(len(r.heads) for r in results) >= 2
    for im, res in zip(imgs, results):
        before = im.copy()
        for m in METHODS:
            want = expected(im, res.heads, m, **assets)
            print(im.shape, m, len(res.heads), "heads,", int((want != im).any(axis=2).sum()), "painted pixels")
            _same(res.draw(m), want, (im.shape, m))
        assert np.array_equal(im, before)
    single = det(imgs[0], confidence_threshold=conf)
    _same(single.draw(), expected(imgs[0], single.heads, "full", **assets), "single image")
    with pytest.raises(draw.DrawAssetsMissing):
        HeadDetector("vgg_heads_m", 320, flame_model=flame_model, weights="synthetic", seed=4)(imgs[0], confidence_threshold=conf).draw()
