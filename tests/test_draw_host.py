"""PredictionResult.draw, the host side (no GPU): the CPU restatement of the drawing rules (tests/draw_ref.py: loop forms against closed forms,
hand-computed cases), the planner of head_detector_amd/draw.py against the fixture recorded from the reference's own draw
(tests/golden/draw_heads.npz, tests/golden/make_golden_draw.py), the new entry point's ABI and the errors of the public interface.

Parity of the three primitives with cv2 itself is UNPINNED where cv2 is absent: ``test_restatement_against_cv2`` pins it wherever cv2 is installed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import draw_ref  # noqa: E402
from draw_fixture import METHODS, expected, fixture_assets, fixture_heads, fixture_image, fixture_result, load_fixture, make_head  # noqa: E402

from head_detector_amd import _lib, _lib_view, draw  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.pncc import MeshAssets  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return load_fixture()


# ---- tests/draw_ref.py ---------------------------------------------------------------------------------------------------------------------
def test_line_loop_form_equals_closed_form():
    """clip + walk, one pixel at a time, against the NumPy forms on random segments: short, long, steep, flat, reversed, far outside."""
    rng = np.random.default_rng(1)
    W, H = 97, 61
    n = 4000
    x1, x2 = rng.integers(-60, W + 60, n), rng.integers(-60, W + 60, n)
    y1, y2 = rng.integers(-60, H + 60, n), rng.integers(-60, H + 60, n)
    x2[:200], y2[:200] = x1[:200], y1[:200] + rng.integers(-3, 4, 200)  # vertical and zero-length ones
    y2[200:400] = y1[200:400]
    drawn, cx1, cy1, cx2, cy2, moved = draw_ref.clip_lines(W, H, x1, y1, x2, y2)
    seen = {"drawn": 0, "moved": 0, "rejected": 0}
    for i in range(n):
        ok, a, b = draw_ref.clip_line_loop(W, H, (x1[i], y1[i]), (x2[i], y2[i]))
        assert ok == bool(drawn[i]), i
        if not ok:
            seen["rejected"] += 1
            continue
        assert (a, b) == ((cx1[i], cy1[i]), (cx2[i], cy2[i])), i
        assert 0 <= a[0] < W and 0 <= b[0] < W and 0 <= a[1] < H and 0 <= b[1] < H
        seen["drawn"] += 1
        seen["moved"] += bool(moved[i])
        xs, ys, _ = draw_ref.line_pixels([a[0]], [a[1]], [b[0]], [b[1]])
        assert list(zip(xs.tolist(), ys.tolist())) == draw_ref.walk_loop(a, b), i
    assert min(seen.values()) >= 300, seen
    # whole pictures: many segments at once against one at a time (the order among segments of one colour cannot matter)
    a = draw_ref.segments(np.zeros((H, W, 3), np.uint8), x1, y1, x2, y2, (1, 2, 3), max_pixels=5000)
    b = np.zeros((H, W, 3), np.uint8)
    for i in range(n):
        draw_ref.line_loop(b, (x1[i], y1[i]), (x2[i], y2[i]), (1, 2, 3))
    assert np.array_equal(a, b) and a.any()
    tri = rng.integers(-20, 90, (40, 3, 1, 2)).astype(np.int32)
    a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    for t in tri:
        draw_ref.polylines(a, [t], isClosed=True, color=(0, 0, 255), thickness=1)
        draw_ref.polylines_loop(b, [t], isClosed=True, color=(0, 0, 255), thickness=1)
    assert np.array_equal(a, b) and a.any()


def test_line_hand_computed():
    # the walk: left to right whatever the direction given, ties toward the start
    want = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert draw_ref.walk_loop((0, 0), (5, 2)) == want and draw_ref.walk_loop((5, 2), (0, 0)) == want
    assert draw_ref.walk_loop((2, 5), (2, 3)) == [(2, 5), (2, 4), (2, 3)]  # dx == 0: not swapped, y steps -1
    assert draw_ref.walk_loop((4, 4), (4, 4)) == [(4, 4)]
    assert draw_ref.walk_loop((0, 3), (2, 0)) == [(0, 3), (1, 2), (1, 1), (2, 0)]  # y-major going up
    # the clip on a 10 x 10 image, one case per branch
    clip = lambda p, q: draw_ref.clip_line_loop(10, 10, p, q)  # noqa: E731
    assert clip((2, -4), (6, 4)) == (True, (4, 0), (6, 4))  # y step: x += trunc(4 * 4 / 8) = 2
    assert clip((3, -5), (0, 2)) == (True, (1, 0), (0, 2))  # y step with a negative quotient: trunc(-15 / 7) = -2, not floor's -3
    assert clip((-3, 2), (5, 6)) == (True, (0, 3), (5, 6))  # x step: y += trunc(3 * 4 / 8) = 1
    assert clip((-6, -3), (12, 15)) == (True, (0, 3), (6, 9))  # both steps; the second end is cut against the first end's new position
    assert clip((-5, 2), (2, -5))[0] is False  # both ends left of the image after the y step
    assert clip((-1, 3), (-1, 8))[0] is False and clip((3, 3), (7, 8)) == (True, (3, 3), (7, 8))


def test_circle_tables_and_forms():
    assert draw_ref.half_widths(1) == [1, 0] and draw_ref.half_widths(2) == [2, 1, 0]
    assert draw_ref.half_widths(3) == [3, 2, 2, 0] and draw_ref.half_widths(4) == [4, 3, 3, 2, 0]
    for R in range(1, 33):
        assert draw.half_widths(R).tolist() == draw_ref.half_widths(R) and draw.half_widths(R).dtype == np.int32
    rng = np.random.default_rng(2)
    for R in (1, 2, 3, 4, 7):
        c = rng.integers(-R - 1, 30 + R + 1, (60, 2))
        a, b, d = (np.zeros((25, 30, 3), np.uint8) for _ in range(3))
        for p in c:
            draw_ref.circle(a, (int(p[0]), int(p[1])), R, (255, 255, 255), -1)
            draw_ref.circle_loop(b, (int(p[0]), int(p[1])), R, (255, 255, 255), -1)
        draw_ref.circles(d, c, R, (255, 255, 255))
        assert np.array_equal(a, b) and np.array_equal(a, d) and a.any()
    plus = draw_ref.circle(np.zeros((5, 5), np.uint8), (2, 2), 1, 1, -1)
    assert plus.tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]


def test_rectangle_pixel_set():
    img = draw_ref.rectangle(np.zeros((12, 12), np.uint8), (3, 3), (8, 7), 1, 2)
    for x, y in ((2, 2), (9, 2), (2, 8), (9, 8)):
        assert img[y, x] == 0  # the outer corner pixels stay unpainted
    for x, y in ((3, 2), (2, 3), (9, 3), (8, 2), (2, 7), (3, 8), (9, 7), (8, 8), (4, 4), (7, 6)):
        assert img[y, x] == 1
    assert img[5, 5] == 0 and img[5, 6] == 0 and int(img.sum()) == 8 * 7 - 4 - 2  # three pixels wide: only two interior pixels are left
    assert img[:2].sum() == 0 and img[9:].sum() == 0 and img[:, :2].sum() == 0 and img[:, 10:].sum() == 0
    rng = np.random.default_rng(3)
    for _ in range(60):
        x, y = (int(v) for v in rng.integers(-4, 16, 2))
        w, h = (int(v) for v in rng.integers(0, 9, 2))
        if rng.random() < 0.3:
            w = 0
        if rng.random() < 0.3:
            h = 0
        a = draw_ref.rectangle(np.zeros((14, 13), np.uint8), (x, y), (x + w, y + h), 1, 2)
        b = draw_ref.rectangle_loop(np.zeros((14, 13), np.uint8), (x, y), (x + w, y + h), 1, 2)
        assert np.array_equal(a, b), (x, y, w, h)
    dot = draw_ref.rectangle(np.zeros((5, 5), np.uint8), (2, 2), (2, 2), 1, 2)  # w == h == 0: a plus
    assert int(dot.sum()) == 5 and dot[2, 1] and dot[1, 2] and not dot[1, 1]


# ---- the planner --------------------------------------------------------------------------------------------------------------------------
def test_planner_reproduces_the_reference_images(g):
    """tests/draw_ref.py driven by draw.py's own plan gives, byte for byte, what the reference's PredictionResult.draw returned: the CPU check of the
    host half (class lists and their order, index lists, truncation, radius, colours).  The pixels themselves exist only on the GPU."""
    for letter in "AB":
        img = fixture_image(g, letter)
        heads = fixture_heads(g, letter)
        assert len(heads) >= 10
        for m in METHODS:
            want = fixture_result(g, letter, m)
            assert (want != img).any()
            got = expected(img, heads, m, **fixture_assets(g))
            assert got.dtype == np.uint8 and np.array_equal(got, want), (letter, m, int((got != want).sum()))
        plan = draw.draw_plan(img.shape, heads, "full", **fixture_assets(g))
        assert plan.points.dtype == np.int32 and plan.points.shape == (len(heads), 300, 2) and plan.radius == 1
        xy = g[f"vertices_{letter}"][:, :, :2]
        neg = (xy > -1) & (xy < 0)
        assert neg.sum() >= 4 and (plan.points[neg] == 0).all()  # truncation toward zero
        assert draw.draw_plan(img.shape, heads, "bbox").triangles is None and draw.draw_plan(img.shape, heads, "bbox").indices is None
        p = draw.draw_plan(img.shape, heads, "points", face_indices=g["face_indices"])
        assert p.boxes is None and p.triangles is None and np.array_equal(p.indices, g["face_indices"])
    assert draw.draw_plan((2500, 2100, 3), [], "bbox").radius == 2 and draw.draw_plan((3000, 4000, 3), [], "bbox").radius == 3


def test_mesh_assets_load_the_draw_files(tmp_path):
    d = tmp_path / "assets"
    (d / "flame_indices").mkdir(parents=True)
    np.save(d / "full_faces.npy", np.array([[0, 1, 2]]))
    np.save(d / "v_template.npy", np.eye(3))
    np.save(d / "flame_indices" / "head_w_ears.npy", np.arange(3))
    a = MeshAssets.load(str(d))
    assert a.triangles is None and a.face_indices is None and a.head_indices is None
    np.savetxt(d / "triangles.txt", np.array([[16.0, 18.0, 17.0], [1.0, 2.0, 0.0]]), delimiter=",")
    np.save(d / "flame_indices" / "face.npy", np.array([2, 0]))
    a = MeshAssets.load(str(d))
    assert a.triangles.dtype == np.int32 and a.triangles.tolist() == [[16, 18, 17], [1, 2, 0]] and a.face_indices.tolist() == [2, 0]
    b = MeshAssets(np.zeros((1, 3)), np.eye(3), np.arange(3), np.arange(2))  # positional arguments keep their meaning
    assert b.head_indices.tolist() == [0, 1] and b.triangles is None and b.face_indices is None


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_draw_entry_point_abi_and_argument_checks():
    hdr = open(os.path.join(ROOT, "include", "vgh_view.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghv_[a-z0-9_]+)\s*\(", hdr))
    assert "vghv_draw_heads" in declared and declared == set(_lib_view.SYMBOLS) and len(declared) <= 6
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_view.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()
    assert {ln.split()[-1] for ln in out if " T " in ln} == declared
    fields = re.search(r"typedef struct vghv_draw_job \{(.*?)\} vghv_draw_job;", hdr, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert names == [f[0] for f in _lib_view.DrawJob._fields_], names
    import ctypes as C

    assert C.sizeof(_lib_view.DrawJob) == 3 * 8 + 8 * 4 + 5 * 8 and _lib_view.DrawJob.points.offset == 56
    for name, const in (("VGHV_MAX_COORD", _lib_view.MAX_COORD), ("VGHV_MAX_RADIUS", _lib_view.MAX_RADIUS), ("VGHV_MAX_DRAW_HEADS", _lib_view.MAX_DRAW_HEADS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == const

    # argument checks happen before the device is touched: they work without a GPU
    lib = _lib_view.load()
    pts = np.zeros((1, 4, 2), np.int32)
    tri = np.array([[0, 1, 2]], np.int32)
    idx = np.array([3], np.int32)
    hw = draw.half_widths(1)
    box = np.array([[0, 0, 2, 2]], np.int32)

    def job(**kw):
        j = _lib_view.DrawJob()
        j.src_dev, j.src_pitch_bytes, j.dst_dev, j.height, j.width, j.channels = 4096, 24, 8192, 8, 8, 3
        j.n_heads, j.n_vertices, j.n_triangles, j.n_indices, j.radius = 1, 4, 1, 1, 1
        j.points, j.boxes, j.triangles, j.indices, j.half_widths = pts.ctypes.data, box.ctypes.data, tri.ctypes.data, idx.ctypes.data, hw.ctypes.data
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(what, **kw):
        assert lib.vghv_draw_heads(job(**kw), None) == -1, what
        assert what.encode() in lib.vghv_last_error(), lib.vghv_last_error()

    refused("null image", src_dev=None)
    refused("null image", dst_dev=None)
    refused("channels", channels=4)
    refused("src_pitch_bytes", src_pitch_bytes=23)
    refused("outside 1 ..", width=40000)
    refused("4-byte aligned", dst_dev=8193)
    bad_tri = np.array([[0, 1, 4]], np.int32)
    refused("triangle 0: index 4 outside the 4 vertices", triangles=bad_tri.ctypes.data)
    bad_idx = np.array([-1], np.int32)
    refused("indices[0] = -1", indices=bad_idx.ctypes.data)
    refused("radius 33", radius=33)
    far = np.full((1, 4, 2), 1 << 24, np.int32)
    refused("head 0: coordinate", points=far.ctypes.data)
    bad_box = np.array([[0, 0, -1, 2]], np.int32)
    refused("head 0: bad box", boxes=bad_box.ctypes.data)
    refused("heads outside", n_heads=-1)
    assert lib.vghv_draw_heads(None, None) == -1 and b"null job" in lib.vghv_last_error()


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_draw_errors(g):
    img = fixture_image(g, "A")
    heads = fixture_heads(g, "A")
    assets = fixture_assets(g)
    with pytest.raises(NotImplementedError, match="pose"):
        PredictionResult(img, heads, **assets).draw("pose")
    with pytest.raises(KeyError, match="nonsense"):
        PredictionResult(img, heads, **assets).draw("nonsense")
    # a missing asset: FileNotFoundError naming the file (the package's convention) AND NotImplementedError (what draw raised before it existed),
    # raised before a GPU is looked for
    some = lambda *keep: {k: v for k, v in assets.items() if k in keep}  # noqa: E731
    for method, kw, file in (("full", some("head_indices", "face_indices"), "triangles.txt"), ("landmarks", some("triangles", "face_indices"), "head_indices.npy"),
                             ("full", some("triangles"), "head_indices.npy"), ("landmarks", some("head_indices"), "triangles.txt"), ("points", some("triangles", "head_indices"), "face.npy")):
        for cls in (FileNotFoundError, NotImplementedError, draw.DrawAssetsMissing):
            with pytest.raises(cls, match=re.escape(file)):
                PredictionResult(img, heads, **kw).draw(method)
    v = g["vertices_A"][0].copy()
    for bad, where in ((np.nan, (7, 1)), (np.inf, (0, 0)), (float(1 << 24), (299, 0)), (-float(1 << 24), (5, 1))):
        w = v.copy()
        w[where] = bad
        with pytest.raises(ValueError, match="head 1"):
            PredictionResult(img, [heads[0], make_head(w, (1, 2, 3, 4))], **assets).draw("points")
    w = v.copy()
    w[3, 2] = np.nan  # z is not drawn
    assert draw.draw_plan(img.shape, [make_head(w, (1, 2, 3, 4))], "full", **assets).points.shape == (1, 300, 2)
    w[0, 0] = float((1 << 24) - 1)
    assert draw.draw_plan(img.shape, [make_head(w, (1, 2, 3, 4))], "full", **assets).points[0, 0, 0] == (1 << 24) - 1
    with pytest.raises(ValueError, match="head 0: bbox"):
        PredictionResult(img, [make_head(v, (5, 5, -1, 4))]).draw("bbox")
    with pytest.raises(ValueError, match="triangles index"):
        PredictionResult(img, heads, triangles=np.array([[0, 1, 300]]), head_indices=g["head_indices"]).draw("landmarks")
    with pytest.raises(ValueError, match="uint8 image"):
        PredictionResult(img.astype(np.float32), heads).draw("bbox")
    if not torch.cuda.is_available():  # no CPU path for the pixels: a missing GPU is an error, never another implementation
        with pytest.raises(_lib.VghError, match="GPU"):
            PredictionResult(img, heads).draw("bbox")
        with pytest.raises(_lib.VghError, match="GPU"):
            PredictionResult(img, heads, **assets).draw()


def test_restatement_against_cv2():
    """Pins tests/draw_ref.py (and with it the kernels, which are bit-exact against it) to OpenCV itself wherever cv2 is installed."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(9)
    H, W = 83, 131
    for _ in range(300):
        a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
        tri = rng.integers(-60, 200, (3, 1, 2)).astype(np.int32)
        cv2.polylines(a, [tri], isClosed=True, color=(0, 0, 255), thickness=1)
        draw_ref.polylines(b, [tri], isClosed=True, color=(0, 0, 255), thickness=1)
        assert np.array_equal(a, b), tri.tolist()
    for _ in range(300):
        a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
        x, y = (int(v) for v in rng.integers(-20, 140, 2))
        w, h = (int(v) for v in rng.integers(0, 60, 2))
        cv2.rectangle(a, (x, y), (x + w, y + h), (255, 0, 0), 2)
        draw_ref.rectangle(b, (x, y), (x + w, y + h), (255, 0, 0), 2)
        assert np.array_equal(a, b), (x, y, w, h)
    for R in (1, 2, 3, 4, 8):
        for _ in range(60):
            a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
            c = (int(rng.integers(-10, W + 10)), int(rng.integers(-10, H + 10)))
            cv2.circle(a, c, R, (255, 255, 255), -1)
            draw_ref.circle(b, c, R, (255, 255, 255), -1)
            assert np.array_equal(a, b), (c, R)
