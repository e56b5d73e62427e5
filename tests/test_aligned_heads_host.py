"""Aligned head crops, the host side (no GPU): the planner against the fixture recorded from the reference's own get_aligned_heads
(tests/golden/aligned_heads.npz, tests/golden/make_golden_aligned.py), the CPU restatement of the warp against its two cv2-free facts, the
companion library's ABI, and the errors of the public entry point."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import warp_affine_ref as war  # noqa: E402
from aligned_fixture import fixture_crops, fixture_heads, formula_image, load_fixture  # noqa: E402

from head_detector_amd import _lib, _lib_view, aligned  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return load_fixture()


def test_planner_matches_the_reference(g):
    """Matrix to 1e-12, everything that went through an int() exactly: rotated or not, bounds, rect, slice and crop shape."""
    assert len(g["names"]) >= 13
    for letter in "AB":
        shape = tuple(int(v) for v in g[f"shape_{letter}"]) + (3,)
        picked = fixture_heads(g, letter)
        plans = aligned.aligned_head_plan(shape, [h for _, _, h in picked], g["head_indices"])
        assert len(plans) == len(picked)
        for (i, _, _), p in zip(picked, plans):
            name = str(g["names"][i])
            assert p.rotated == bool(g["rotated"][i]), name
            assert np.abs(p.matrix - g["matrix"][i]).max() <= 1e-12, name
            assert tuple(p.bounds) == tuple(g["bounds"][i]), name
            assert tuple(p.rect) == tuple(g["rect"][i]), name
            assert p.shape == tuple(g["crop_shape"][i]), name
            x, y, w, h = p.rect
            canvas = np.empty((p.bounds[1], p.bounds[0], 0), dtype=np.uint8)
            x0, y0, x1, y1 = p.region
            assert canvas[y : y + h, x : x + w].shape[:2] == (max(0, y1 - y0), max(0, x1 - x0)), name  # Python slice semantics, negative starts included
    # the situations the fixture exists for are really in it
    shapes = [tuple(s) for s in g["crop_shape"]]
    assert any(s[0] == 0 and s[1] > 0 for s in shapes) and any(s[1] == 0 and s[0] > 0 for s in shapes)
    assert 60.0 in g["yaw"] and not g["rotated"][list(g["yaw"]).index(60.0)]
    assert {0.0, 90.0} <= set(g["roll"][g["rotated"]].tolist()) and (g["roll"][g["rotated"]] < 0).any()


def test_skull_centre_and_helpers_match_the_reference(g):
    for i, letter, head in fixture_heads(g):
        if not g["rotated"][i]:
            continue
        shape = tuple(int(v) for v in g[f"shape_{letter}"])
        img = np.empty(shape + (0,), dtype=np.uint8)
        assert aligned.flame_params_skull_center(head.flame_params, img) == tuple(g["skull_centre"][i])
        m, b = aligned.get_rotation_mat(img, tuple(int(v) for v in g["skull_centre"][i]), head.head_pose.roll)
        assert np.abs(m - g["matrix"][i]).max() <= 1e-12 and tuple(b) == tuple(g["bounds"][i])
    assert aligned.extend_bbox([10, 20, 33, 47], offset=0.1).tolist() == [6, 15, 39, 56] and aligned.extend_bbox([3, 2, 33, 47]).dtype == np.int32
    assert aligned.extend_bbox([3, 2, 33, 47], offset=0.1).tolist() == [0, -2, 39, 56]  # -0.3 and -2.7 truncate toward zero
    assert aligned.extend_to_rect(np.array([5, 7, 40, 31], dtype=np.int32)).tolist() == [5, 3, 40, 40]  # (40 - 31) // 2 = 4
    assert aligned.extend_to_rect(np.array([5, 7, 31, 40], dtype=np.int32)).tolist() == [1, 7, 40, 40]
    assert aligned.extend_to_rect(np.array([5, 7, 40, 40], dtype=np.int32)).tolist() == [5, 7, 40, 40]


def test_restatement_reproduces_the_fixture_crops(g):
    """The fixture's bytes came out of the reference's whole-canvas warp; the region argument of the restatement gives the same bytes from the
    planner's geometry (what the GPU tests rely on for images too large to warp whole on the CPU)."""
    crops = fixture_crops(g)
    for i, letter, head in fixture_heads(g):
        img = formula_image(*(int(v) for v in g[f"shape_{letter}"]))
        (p,) = aligned.aligned_head_plan(img.shape, [head], g["head_indices"])
        x0, y0, x1, y1 = p.region
        if x1 <= x0 or y1 <= y0:
            assert crops[i].size == 0
            continue
        got = war.warp_affine(img, p.matrix, p.bounds, region=p.region)
        assert got.shape == crops[i].shape and np.array_equal(got, crops[i]), str(g["names"][i])
        if not p.rotated:
            assert np.array_equal(got, img[y0:y1, x0:x1])


def test_product_tables_are_the_restatement_tables():
    """aligned.warp_tables (what the kernel consumes) against a direct evaluation of the formulas in include/vgh_view.h."""
    m = war.getRotationMatrix2D((211, 97), 33.3, 1.0)
    m[:, 2] += (17.5, -4.25)
    x0, y0, x1, y1 = 40, 11, 171, 95
    t = aligned.warp_tables(m, (x0, y0, x1, y1))
    a00, a01, b0, a10, a11, b1 = war.invert_affine(m)
    xs, ys = np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64)
    want = np.concatenate([np.rint(a00 * xs * 1024), np.rint(a10 * xs * 1024), np.rint((a01 * ys + b0) * 1024) + 16, np.rint((a11 * ys + b1) * 1024) + 16])
    assert t.dtype == np.int32 and np.array_equal(t, want.astype(np.int32))


def test_warp_restatement_integer_shift_and_rot90():
    """The two facts about the 8-bit bilinear warp that need no cv2: roll 0 about any centre of an image with even sides is a pure integer
    shift, and roll 90 equals np.rot90 up to a shift."""
    img = formula_image(58, 84)
    H, W = img.shape[:2]
    for centre in ((20, 31), (70, 9), (0, 0)):
        m, (bw, bh) = aligned.get_rotation_mat(img, centre, 0.0)
        assert (bw, bh) == (W, H)
        out = war.warp_affine(img, m, (bw, bh))
        sx, sy = W // 2 - centre[0], H // 2 - centre[1]
        want = np.zeros_like(img)
        ys, xs = np.mgrid[0:H, 0:W]
        ok = (ys - sy >= 0) & (ys - sy < H) & (xs - sx >= 0) & (xs - sx < W)
        want[ok] = img[(ys - sy)[ok], (xs - sx)[ok]]
        assert np.array_equal(out, want), centre
    # roll 90 about the image centre: the canvas is [W, H] and holds the image turned counter-clockwise, possibly moved by whole pixels
    m, (bw, bh) = aligned.get_rotation_mat(img, (W // 2, H // 2), 90.0)
    assert (bw, bh) == (H, W)
    out = war.warp_affine(img, m, (bw, bh))
    rot = np.rot90(img)
    assert rot.shape == out.shape
    hits = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            a = out[max(0, dy) : bh + min(0, dy), max(0, dx) : bw + min(0, dx)]
            b = rot[max(0, -dy) : bh + min(0, -dy), max(0, -dx) : bw + min(0, -dx)]
            hits.append(np.array_equal(a, b))
    assert sum(hits) == 1, hits


def test_view_library_abi_and_core_library_untouched():
    """include/vgh_view.h == the loader's bindings == what libvghview.so exports; libvgh.so exports exactly what it did: no vghv_ symbol, nothing new."""
    hdr = open(os.path.join(ROOT, "include", "vgh_view.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghv_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib_view.SYMBOLS) and 3 <= len(declared) <= 6, declared ^ set(_lib_view.SYMBOLS)
    lib = _lib_view.load()
    assert lib.vghv_version().startswith(b"vghview") and lib.vghv_last_error() is not None

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        return {ln.split()[-1] for ln in out if " T " in ln}

    view = exported(_lib_view.LIB_PATH)
    assert view == declared, view ^ declared  # -fvisibility=hidden: no internal function leaves the library
    core = {s for s in exported(_lib.LIB_PATH) if s.startswith("vgh")}
    assert core == set(_lib.SYMBOLS), core ^ set(_lib.SYMBOLS)
    assert not any(s.startswith("vghv_") for s in core) and len(_lib.SYMBOLS) == 86 and _lib.ABI_VERSION == 8
    assert not (set(re.findall(r"\bvgh_[a-z0-9_]+", hdr)) & set(_lib.SYMBOLS)), "vgh_view.h declares nothing of vgh.h"
    # struct layout of the binding against the header's field list
    fields = re.search(r"typedef struct vghv_crop \{(.*?)\} vghv_crop;", hdr, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert names == [f[0] for f in _lib_view.Crop._fields_], names
    # argument checks happen before the device is touched: they work without a GPU
    crop = (_lib_view.Crop * 1)()
    tab = np.zeros(8, dtype=np.int32)
    assert lib.vghv_warp_crops(crop, 0, None, 0, None, 0, None) == 0
    assert lib.vghv_warp_crops(crop, 1, tab.ctypes.data, 8, None, 0, None) == -1 and b"null src_dev" in lib.vghv_last_error()
    crop[0].src_dev, crop[0].src_h, crop[0].src_w, crop[0].src_channels, crop[0].src_pitch_bytes = 4096, 4, 4, 4, 16
    assert lib.vghv_warp_crops(crop, 1, tab.ctypes.data, 8, None, 0, None) == -1 and b"channels" in lib.vghv_last_error()
    crop[0].src_channels, crop[0].src_pitch_bytes = 3, 11
    assert lib.vghv_warp_crops(crop, 1, tab.ctypes.data, 8, None, 0, None) == -1 and b"src_pitch_bytes" in lib.vghv_last_error()
    crop[0].src_pitch_bytes, crop[0].crop_w, crop[0].crop_h = 12, 3, 2
    assert lib.vghv_warp_crops(crop, 1, tab.ctypes.data, 8, 4096, 18, None) == -1 and b"tables" in lib.vghv_last_error()
    tab = np.zeros(10, dtype=np.int32)
    assert lib.vghv_warp_crops(crop, 1, tab.ctypes.data, 10, 4096, 17, None) == -1 and b"destination" in lib.vghv_last_error()
    with pytest.raises(_lib.VghError, match="destination"):
        _lib_view.check(-1)


def test_get_aligned_heads_errors(g):
    img = formula_image(*(int(v) for v in g["shape_A"]))
    heads = [h for _, _, h in fixture_heads(g, "A")]
    with pytest.raises(FileNotFoundError, match="head_indices.npy"):
        PredictionResult(img, heads).get_aligned_heads()
    with pytest.raises(NotImplementedError):
        PredictionResult(img, heads, head_indices=g["head_indices"]).draw()
    assert PredictionResult(img, [], head_indices=g["head_indices"]).get_aligned_heads() == []
    if not torch.cuda.is_available():  # no CPU path for the pixels: a missing GPU is an error, never another implementation
        with pytest.raises(_lib.VghError, match="GPU"):
            PredictionResult(img, heads, head_indices=g["head_indices"]).get_aligned_heads()
    for bad in (img.astype(np.float32), img[:, :, :2], np.zeros((4, 4, 4), dtype=np.uint8), img[:, :, 0]):
        with pytest.raises(ValueError, match="uint8 image"):
            aligned.warp_crops(bad, [(np.eye(2, 3), (0, 0, 2, 2))])


def test_restatement_against_cv2():
    """Pins the restatement (and with it the kernel, which is bit-exact against it) to OpenCV itself wherever cv2 is installed."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(5)
    for h, w in ((58, 84), (121, 77)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for angle in (0.0, 90.0, 17.3, -23.7, 181.0):
            centre = (int(rng.integers(0, w)), int(rng.integers(0, h)))
            assert np.abs(war.getRotationMatrix2D(centre, angle, 1.0) - cv2.getRotationMatrix2D(centre, angle, 1.0)).max() <= 1e-12
            m, bounds = aligned.get_rotation_mat(img, centre, angle)
            assert np.array_equal(war.warp_affine(img, m, bounds), cv2.warpAffine(img, m, bounds, flags=cv2.INTER_LINEAR)), (h, w, angle)
