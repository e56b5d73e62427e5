"""Head visibility buffers on the MI355X: csrc/visibility.hip (libvghvis.so) against the reference's own C++ -- its recorded outputs
(tests/golden/visibility.npz) and, where oracle/_ref provides it, the live library (otherwise the CPU restatement tests/visibility_ref.py, which
tests/test_visibility_host.py holds to the same outputs).  Every comparison is np.array_equal / torch.equal: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import visibility_ref as vr  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402

from head_detector_amd import pncc, visibility  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _live():
    return vr.live() is not None


def _fields(res):
    assert isinstance(res, visibility.HeadVisibility)
    return {k: getattr(res, k) for k in vr.FIELDS}


def _check(heads, tri, H, W, mode, z_sign, what, want=None):
    """The kernel against the reference composition (and ``want``, a recorded result): all seven outputs, the inputs untouched."""
    heads = np.asarray(heads, dtype=np.float32)
    before, tri_before = heads.copy(), np.array(tri, copy=True)
    got = _fields(visibility.rasterize_heads(heads, tri, H, W, occlusion=mode, z_sign=z_sign))
    assert np.array_equal(heads, before, equal_nan=True) and np.array_equal(tri, tri_before)
    ref = vr.compose(heads, tri, H, W, mode, z_sign, _live())
    if want is not None:
        vr.same(ref, want, (what, "fixture against the reference"))
        vr.same(got, want, (what, "recorded"))
    vr.same(got, ref, what)
    return got


def test_scenes_in_both_modes(gpu_lib):
    g = np.load(vr.GOLDEN)
    for letter in ("A", "B"):
        (H, W), heads, tri = vr.scene(letter)
        order = vr.golden_case(g, f"scene_{letter}_order")
        want = {"order": order, "depth": vr.golden_case(g, f"scene_{letter}_depth", order)}
        for mode in ("order", "depth"):
            got = _check(heads, tri, H, W, mode, vr.SCENE_Z_SIGN, (letter, mode), want[mode])
            # without barycentrics: None, everything else the same
            lean = visibility.rasterize_heads(heads, tri, H, W, occlusion=mode, z_sign=vr.SCENE_Z_SIGN, barycentric=False)
            assert lean.barycentric is None
            for k in vr.FIELDS:
                assert k == "barycentric" or np.array_equal(getattr(lean, k), got[k]), k
            # on the device: tensors in, tensors out, nothing modified
            v = torch.from_numpy(heads).to(_dev())
            keep = v.clone()
            dev = visibility.rasterize_heads(v, tri, H, W, occlusion=mode, z_sign=vr.SCENE_Z_SIGN, to_host=False)
            assert torch.equal(v, keep)
            for k in vr.FIELDS:
                t = getattr(dev, k)
                assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.from_numpy(got[k]).dtype, k
                assert torch.equal(t.cpu(), torch.from_numpy(got[k])), k
            assert torch.equal(dev.mask(3).cpu(), torch.from_numpy(got["head_index"] == 3)) and np.array_equal(lean.mask(3), got["head_index"] == 3)
            frac = lean.visible_fraction
            assert np.array_equal(frac, got["visible_pixels"] / np.maximum(got["covered_pixels"], 1)) and np.array_equal(dev.visible_fraction.cpu().numpy(), frac)
        # the other sign of z, float64 vertices and int64 triangles are converted
        _check(heads, tri, H, W, "depth", 1.0, (letter, "z as given"))
        other = visibility.rasterize_heads(heads.astype(np.float64), tri.astype(np.int64), H, W, occlusion="depth", z_sign=-1.0)
        vr.same(_fields(other), want["depth"], (letter, "other dtypes"))


def test_a_copy_of_a_head(gpu_lib):
    """Scene A with a copy of head 2 appended: in painter's order the copy hides head 2 entirely; with the shared z-buffer every depth of the copy is
    equal to head 2's or loses, and equal depth keeps the earlier head."""
    (H, W), heads, tri = vr.scene("A")
    more = np.concatenate([heads, heads[2:3]])
    order = _check(more, tri, H, W, "order", vr.SCENE_Z_SIGN, "copy, order")
    assert order["covered_pixels"][2] == order["covered_pixels"][8] > 0 and order["visible_pixels"][2] == 0 and order["visible_pixels"][8] > 0
    assert not order["vertex_visible"][2].any() and order["vertex_visible"][8].any()
    depth = _check(more, tri, H, W, "depth", vr.SCENE_Z_SIGN, "copy, depth")
    assert depth["covered_pixels"][2] == depth["covered_pixels"][8] > 0 and depth["visible_pixels"][8] == 0 and depth["visible_pixels"][2] > 0
    assert not depth["vertex_visible"][8].any() and not (depth["head_index"] == 8).any()


def test_single_meshes_and_the_inside_rule(gpu_lib):
    g = np.load(vr.GOLDEN)
    for name, (ver, tri, (H, W)) in vr.single_cases().items():
        want = vr.golden_case(g, name)
        for mode in ("order", "depth"):
            got = _check(ver[None], tri, H, W, mode, 1.0, (name, mode), want)
        # pncc.rasterize_triangles: the Sim3DR-shaped entry, the three arrays the binding fills
        d, t, b = pncc.rasterize_triangles(ver, tri, H, W)
        assert d.dtype == np.float32 and d.shape == (H, W) and t.dtype == np.int32 and t.shape == (H, W) and b.dtype == np.float32 and b.shape == (H, 3 * W)
        assert np.array_equal(d, want["depth"]) and np.array_equal(t, want["triangle_index"]) and np.array_equal(b.reshape(H, W, 3), want["barycentric"])
        d2, t2, b2 = pncc.rasterize_triangles(torch.from_numpy(ver).to(_dev()), tri, H, W)  # a GPU tensor is passed through, NumPy comes back
        assert isinstance(d2, np.ndarray) and np.array_equal(d2, d) and np.array_equal(t2, t) and np.array_equal(b2, b)
        # [V, 3] is one head
        vr.same(_fields(visibility.rasterize_heads(ver, tri, H, W)), got, (name, "[V, 3]"))
    corner = visibility.rasterize_heads(*vr.corner_case(), 16, 16)
    assert int((corner.triangle_index == 5).sum()) == 49 and (corner.barycentric[corner.triangle_index == 5] == np.float32([1, 0, 0])).all()  # the zero-determinant triangle
    ver, tri = vr.integer_grid_mesh()
    grid = visibility.rasterize_heads(ver, tri, 16, 16)
    assert not np.array_equal(grid.triangle_index >= 0, vr.compose(ver, tri, 16, 16, rule="gt")["triangle_index"] >= 0)  # not the rule of `_rasterize`
    # two grids, the second shifted by whole pixels and nearer in places: edges on pixel centres, equal and unequal depths, both modes
    two = np.stack([ver, ver + np.float32([2, 1, 0.5])])
    for mode in ("order", "depth"):
        for z in (1.0, -1.0):
            _check(two, tri, 16, 16, mode, z, ("two grids", mode, z))


def test_odd_sizes_edges_and_odd_values(gpu_lib):
    for H, W in ((1, 1), (3, 37), (17, 16), (33, 5)):  # not multiples of 16
        a = ro.random_mesh(5, n_side=6, size=70.0, centre=(W / 2, H / 2))
        b = ro.random_mesh(6, n_side=6, size=50.0, centre=(W / 3, H / 2))  # its vertices with a's triangle list: the same sheet in another triangle order
        for mode in ("order", "depth"):
            got = _check(np.stack([a[0], b[0]]), a[1], H, W, mode, 1.0, ((H, W), mode))
            assert got["covered_pixels"].sum() > 0
    # a mesh over each edge (together, three heads deep in places), and a mesh far larger than the image
    H, W = sr.EDGE_SHAPE[:2]
    sides = [vr.edge_mesh(s) for s in sr.EDGE_CENTRES]
    centre = ro.random_mesh(44, n_side=10, size=38.0, centre=(50.0, 37.0), depth_scale=30.0)
    huge = ro.random_mesh(44, n_side=10, size=5000.0, centre=(50.0, 37.0), depth_scale=30.0)
    for mode in ("order", "depth"):
        _check(np.stack([centre[0]] + [s[0] for s in sides]), centre[1], H, W, mode, 1.0, ("edges", mode))
        got = _check(np.stack([centre[0], huge[0], sides[0][0]]), centre[1], H, W, mode, -1.0, ("huge", mode))
        assert got["covered_pixels"][1] == H * W
    # -0.0 and NaN depths, non-finite corners (the "odd" vertices of the shaded-mesh test)
    ver, tri, _ = ro.random_mesh(2)
    odd = ver.copy()
    odd[::7, 2] = -0.0
    odd[5, 2] = np.nan
    odd[11, 0] = np.inf
    odd[13, 1] = np.nan
    flat = ver.copy()
    flat[:, 2] = 0.0  # +0 everywhere: equal to the -0 depths of `odd`, the earlier owner keeps those pixels
    for mode in ("order", "depth"):
        for z in (1.0, -1.0):
            _check(np.stack([odd, flat, odd]), tri, 128, 128, mode, z, ("odd", mode, z))
            _check(np.stack([flat, odd]), tri, 128, 128, mode, z, ("flat first", mode, z))


def test_head_counts_and_stale_scratch(gpu_lib):
    (H, W), heads, tri = vr.scene("B")
    for mode in ("order", "depth"):
        empty = visibility.rasterize_heads(np.zeros((0, heads.shape[1], 3), np.float32), tri, H, W, occlusion=mode)
        vr.same(_fields(empty), vr.compose(np.zeros((0, heads.shape[1], 3), np.float32), tri, H, W, mode), ("n = 0", mode))
        assert (empty.head_index == -1).all() and (empty.triangle_index == -1).all() and (empty.depth == np.float32(-1e8)).all() and not empty.barycentric.any()
        assert empty.visible_pixels.shape == (0,) and empty.covered_pixels.shape == (0,) and empty.vertex_visible.shape == (0, heads.shape[1])
        assert empty.visible_fraction.shape == (0,)
        for n in (1, 3):
            _check(heads[:n], tri, H, W, mode, vr.SCENE_Z_SIGN, ("n", n, mode))
        none = visibility.rasterize_heads(heads[:3], tri[:0], H, W, occlusion=mode)  # no triangles: pure background
        vr.same(_fields(none), vr.compose(heads[:3], tri[:0], H, W, mode), ("T = 0", mode))
        assert (none.head_index == -1).all() and not none.covered_pixels.any() and not none.vertex_visible.any()
    # two consecutive calls with different image sizes (and head counts): no scratch of the first is seen by the second
    big = _check(heads, tri, H, W, "depth", -1.0, "first call")
    small = _check(heads[:2] * np.float32(0.4), tri, 40, 61, "order", -1.0, "second call, smaller")
    again = _check(heads, tri, H, W, "depth", -1.0, "third call, larger again")
    vr.same(again, big, "repeatable")
    assert small["head_index"].shape == (40, 61)
    # a head wholly outside the image
    away = heads[:2] + np.float32([10000, 0, 0])
    got = _check(np.concatenate([away, heads[:1]]), tri, H, W, "order", -1.0, "heads outside")
    assert got["covered_pixels"].tolist()[:2] == [0, 0] and got["covered_pixels"][2] > 0


def test_prediction_result_get_visibility(gpu_lib):
    g = np.load(vr.GOLDEN)
    (H, W), heads, tri = vr.scene("A")
    hs = [sr.make_head(h) for h in heads]
    image = sr.background(5, (H, W, 3))
    res = PredictionResult(image, hs, faces=tri)
    order = vr.golden_case(g, "scene_A_order")
    want = {"order": order, "depth": vr.golden_case(g, "scene_A_depth", order)}
    got = res.get_visibility()  # painter's order, no barycentrics
    assert got.barycentric is None
    for k in vr.FIELDS:
        assert k == "barycentric" or np.array_equal(getattr(got, k), want["order"][k]), k
    vr.same(_fields(res.get_visibility(occlusion="depth", barycentric=True)), want["depth"], "get_visibility, depth")
    for h, v in zip(hs, heads):
        assert np.array_equal(h.vertices_3d, v)  # unlike get_pncc, no z flip is left behind
    dev = PredictionResult(torch.from_numpy(image).to(_dev()), hs, faces=tri).get_visibility(to_host=False)
    assert dev.head_index.is_cuda and dev.vertex_visible.dtype == torch.bool and torch.equal(dev.head_index.cpu(), torch.from_numpy(want["order"]["head_index"]))
    # no heads: all-background buffers, empty per-head arrays
    none = PredictionResult(image, [], faces=tri).get_visibility(barycentric=True)
    assert (none.head_index == -1).all() and (none.depth == np.float32(-1e8)).all() and not none.barycentric.any() and none.visible_pixels.shape == (0,)
    assert none.head_index.shape == (H, W) and none.covered_pixels.shape == (0,) and none.vertex_visible.shape[0] == 0


def test_hundred_heads_on_twelve_megapixels(gpu_lib):
    """3000 x 4000, 100 ellipsoids of FLAME's size (5 002 vertices, 10 000 triangles) of 100 .. 300 px, some hanging over the edges, against the composition
    of reference calls run on the CPU.  The checker meant for this case is the live library of oracle/_ref (about a second a mode).  Where it cannot be had
    the composition falls back to the Python restatement, which tests/test_visibility_host.py holds to the same recorded outputs: the case then still
    checks the same thing but walks about 10^6 triangles a mode (twice that in depth mode) in Python and takes many minutes; the test says so."""
    H, W, n = 3000, 4000, 100
    if not _live():
        print("oracle/_ref is absent: the 100-head composition runs through the Python restatement and takes many minutes")
    unit, tri = sr.ellipsoid()
    heads = sr.ellipsoid_heads(np.random.default_rng(29), n, H, W, 100.0, 300.0, unit, spread=1.02)
    v = torch.from_numpy(heads).to(_dev())
    for mode in ("order", "depth"):
        want = vr.compose(heads, tri, H, W, mode, -1.0, _live())
        vis, cov = want["visible_pixels"], want["covered_pixels"]
        print(f"{mode}: {int(cov.sum())} covered, {int(vis.sum())} owned pixels, {int(((cov > 0) & (vis < cov)).sum())} heads partly hidden")
        assert int(vis.sum()) > 1_000_000 and int(((cov > 0) & (vis < cov)).sum()) >= 10
        got = visibility.rasterize_heads(v, tri, H, W, occlusion=mode, z_sign=-1.0, to_host=False)
        for k in vr.FIELDS:
            a, b = getattr(got, k).cpu().numpy(), want[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (mode, k, int((a != b).sum()))
        del got, want
    assert torch.equal(v.cpu(), torch.from_numpy(heads))
