"""Head visibility buffers, the host side (no GPU): the CPU restatement of tests/visibility_ref.py against the outputs recorded from the reference's own
C++ (tests/golden/visibility.npz, tests/golden/make_golden_visibility.py) and against the live library where oracle/_ref provides it; what the fixture
exercises; the ABI of libvghvis.so and its argument checks; the errors of the public interface, raised before a GPU is looked for."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import visibility_ref as vr  # noqa: E402

from head_detector_amd import _lib, _lib_view, _lib_vis, pncc, visibility  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return np.load(vr.GOLDEN)


def _sources():
    return [False] + ([True] if vr.live() is not None else [])  # the restatement always; the reference's own C++ where it can be had


def _scene_results(g, letter):
    order = vr.golden_case(g, f"scene_{letter}_order")
    return order, vr.golden_case(g, f"scene_{letter}_depth", order)


# ---- tests/visibility_ref.py ------------------------------------------------------------------------------------------------------------------
def test_compositions_equal_the_recorded_reference(g):
    for letter in ("A", "B"):
        (H, W), heads, tri = vr.scene(letter)
        before = heads.copy()
        want = dict(zip(("order", "depth"), _scene_results(g, letter)))
        for use_live in _sources():
            for mode in ("order", "depth"):
                vr.same(vr.compose(heads, tri, H, W, mode, vr.SCENE_Z_SIGN, use_live), want[mode], (letter, mode, use_live))
        assert np.array_equal(heads, before)


def test_single_meshes_equal_the_recorded_reference(g):
    for name, (ver, tri, (H, W)) in vr.single_cases().items():
        want = vr.golden_case(g, name)
        for use_live in _sources():
            for mode in ("order", "depth"):  # one head: the two modes are the same thing
                vr.same(vr.compose(ver, tri, H, W, mode, 1.0, use_live), want, (name, mode, use_live))
        assert want["depth"].dtype == np.float32 and want["barycentric"].shape == (H, W, 3) and want["vertex_visible"].dtype == bool
        bg = want["triangle_index"] < 0
        assert np.array_equal(bg, want["head_index"] < 0) and (want["depth"][bg] == np.float32(-1e8)).all() and not want["barycentric"][bg].any()
        assert want["visible_pixels"][0] == want["covered_pixels"][0] == int((~bg).sum()) > 0


def test_the_fixture_is_not_trivial(g):
    a_order, a_depth = _scene_results(g, "A")
    b_order, b_depth = _scene_results(g, "B")
    vis, cov = a_depth["visible_pixels"], a_depth["covered_pixels"]
    assert int(((cov > 0) & (vis == 0)).sum()) == 1  # exactly one covered head that cannot be seen at all
    differ = int(((a_order["head_index"] != a_depth["head_index"]) | (a_order["triangle_index"] != a_depth["triangle_index"])).sum())
    assert differ > 1000, differ  # 4 610 when recorded
    for res in (a_order, a_depth, b_order, b_depth):
        vis, cov = res["visible_pixels"], res["covered_pixels"]
        assert (vis <= cov).all() and int(((vis > 0) & (vis < cov)).sum()) >= 6  # partly occluded heads: seen, but not all of what they cover
        assert int(vis.sum()) == int((res["head_index"] >= 0).sum())
        hidden = (cov > 0) & (vis == 0)
        assert not res["vertex_visible"][hidden].any() and res["vertex_visible"][~hidden].any(axis=1).all()
    assert np.array_equal(a_order["covered_pixels"], a_depth["covered_pixels"]) and a_order["covered_pixels"][0] == 1351 and b_order["covered_pixels"][0] == 2823
    # the degenerate triangle owns pixels: a 7 x 7 block with weights (1, 0, 0)
    corner = vr.golden_case(g, "corner")
    block = corner["triangle_index"] == 5
    assert int(block.sum()) > 0 and (corner["barycentric"][block] == np.float32([1, 0, 0])).all()
    ver, tri = vr.corner_case()
    assert tri[5].tolist() == [4, 4, 1] and corner["vertex_visible"][0, [4, 1]].all() and not corner["vertex_visible"][0, 7]
    # on the integer grid the >= 0 rule and the > 0 rule of `_rasterize` own different pixels
    ver, tri = vr.integer_grid_mesh()
    other = vr.compose(ver, tri, 16, 16, "order", 1.0, False, rule="gt")
    grid = vr.golden_case(g, "grid")
    assert not np.array_equal(other["triangle_index"] >= 0, grid["triangle_index"] >= 0) and other["covered_pixels"][0] < grid["covered_pixels"][0]
    # ... and on a random float mesh they agree, which is why such meshes alone would pass a careless kernel
    ver, tri, (H, W) = vr.single_cases()["random"]
    vr.same(vr.compose(ver, tri, H, W, "order", 1.0, False, rule="gt"), vr.golden_case(g, "random"), "random, > 0 rule")


def test_restated_inside_rule():
    p0, p1, p2 = np.float32([0, 0, 0]), np.float32([4, 0, 0]), np.float32([0, 4, 0])
    px, py = np.float32([0, 2, 0, 1, 2, 4, 3]), np.float32([0, 0, 2, 1, 2, 0, 3])
    inside = vr.is_point_in_tri(px, py, p0, p1, p2)[0]
    assert inside.tolist() == [True, True, True, True, False, False, False]  # corner p0 and the edges through it are in, the far edge (u + v = 1) is out
    assert vr.is_point_in_tri(px, py, p0, p1, p2, "gt")[0].tolist() == [False, False, False, True, False, False, False]
    inside, w0, w1, w2 = vr.is_point_in_tri(px, py, p0, p0, p1)  # zero determinant: u = v = 0 everywhere
    assert inside.all() and (w0 == 1).all() and not w1.any() and not w2.any()


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def test_visibility_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_vis.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghvis_[a-z0-9_]+)\s*\(", hdr))
    want = {"vghvis_version", "vghvis_last_error", "vghvis_rasterize_triangles"}
    assert declared == want and set(_lib_vis.SYMBOLS) == want and _exported(_lib_vis.LIB_PATH) == want  # exactly 3
    assert _lib_vis.load().vghvis_version().startswith(b"vghvis")
    fields = re.search(r"typedef struct vghvis_job \{(.*?)\} vghvis_job;", hdr, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    J = _lib_vis.Job
    assert names == [f[0] for f in J._fields_], names
    offsets = {f[0]: getattr(J, f[0]).offset for f in J._fields_}
    assert offsets == {"height": 0, "width": 4, "n_heads": 8, "n_vertices": 12, "n_triangles": 16, "mode": 20, "z_sign": 24, "verts_dev": 32, "triangles": 40, "bounds": 48,
                       "depth_dev": 56, "triangle_dev": 64, "head_dev": 72, "bary_dev": 80, "visible_px_dev": 88, "covered_px_dev": 96, "vertex_visible_dev": 104}, offsets
    assert C.sizeof(J) == 112
    for name, value in (("VGHVIS_MAX_SIDE", _lib_vis.MAX_SIDE), ("VGHVIS_MAX_HEADS", _lib_vis.MAX_HEADS), ("VGHVIS_MODE_ORDER", _lib_vis.MODES["order"]),
                        ("VGHVIS_MODE_DEPTH", _lib_vis.MODES["depth"])):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    # the other two libraries are what they were
    core = {s for s in _exported(_lib.LIB_PATH) if s.startswith("vgh")}
    assert core == set(_lib.SYMBOLS) and len(core) == 86 and _lib.ABI_VERSION == 8 and not any(s.startswith(("vghv_", "vghvis_")) for s in core)
    view = _exported(_lib_view.LIB_PATH)
    assert view == set(_lib_view.SYMBOLS) and len(view) == 6 and not any(s.startswith("vghvis_") for s in view)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib_vis.load()
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    bad_tri = np.array([[0, 1, 2], [1, 4, 2]], np.int32)
    neg_tri = np.array([[0, 1, 2], [1, -1, 2]], np.int32)
    bounds = np.array([[0, 0, 7, 7]], np.int32)

    def job(**kw):
        j = _lib_vis.Job()
        j.height, j.width, j.n_heads, j.n_vertices, j.n_triangles, j.mode, j.z_sign = 8, 8, 1, 4, 2, 0, 1.0
        j.verts_dev, j.triangles, j.bounds = 4096, tri.ctypes.data, bounds.ctypes.data
        j.depth_dev, j.triangle_dev, j.head_dev, j.bary_dev = 8192, 12288, 16384, 20480
        j.visible_px_dev, j.covered_px_dev, j.vertex_visible_dev = 24576, 28672, 32768
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(what, **kw):
        assert lib.vghvis_rasterize_triangles(job(**kw), None) == -1, what
        assert what.encode() in lib.vghvis_last_error(), lib.vghvis_last_error()

    refused("height x width 0 x 8", height=0)
    refused("height x width 8 x 40000", width=40000)
    refused("n_heads", n_heads=-1)
    refused("n_heads", n_heads=65537)
    refused("n_vertices", n_vertices=-1)
    refused("n_vertices 0 with 2 triangles", n_vertices=0, vertex_visible_dev=None)
    refused("vertex_visible_dev with n_vertices 0", n_vertices=0)
    refused("n_triangles", n_triangles=-1)
    refused("mode 2", mode=2)
    refused("mode -1", mode=-1)
    refused("z_sign", z_sign=0.5)
    refused("z_sign", z_sign=float("nan"))
    refused("null depth_dev", depth_dev=None)
    refused("null triangle_dev", triangle_dev=None)
    refused("null head_dev", head_dev=None)
    refused("null verts_dev", verts_dev=None)
    refused("null triangles", triangles=None)
    refused("null bounds", bounds=None)
    refused("triangle 1: index 4 outside the 4 vertices", triangles=bad_tri.ctypes.data)
    refused("triangle 1: index -1 outside the 4 vertices", triangles=neg_tri.ctypes.data)
    for b in ([0, 0, 8, 7], [0, 0, 7, 8], [-1, 0, 7, 7], [0, -1, 7, 7]):
        out = np.array([b], np.int32)
        refused("bounds: head 0: (%d, %d, %d, %d) outside the image" % tuple(b), bounds=out.ctypes.data)
    refused("exceed one launch", n_heads=65536, n_triangles=1 << 20)
    refused("vertex_visible_dev with n_vertices 0", n_vertices=0, n_triangles=0)  # nothing to rasterise, but flags of no vertices were asked for
    for optional in ("bary_dev", "visible_px_dev", "covered_px_dev", "vertex_visible_dev"):  # an optional output left out changes no check
        refused("null depth_dev", depth_dev=None, **{optional: None})
        refused("triangle 1: index 4 outside the 4 vertices", triangles=bad_tri.ctypes.data, **{optional: None})
    assert lib.vghvis_rasterize_triangles(None, None) == -1 and b"null job" in lib.vghvis_last_error()


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_public_argument_errors_come_before_the_gpu():
    (H, W), heads, tri = vr.scene("A")
    hs = [sr.make_head(h) for h in heads]
    image = np.zeros((H, W, 3), np.uint8)
    res = PredictionResult(image, hs, faces=tri)
    with pytest.raises(ValueError, match="occlusion"):
        res.get_visibility(occlusion="nearest")
    with pytest.raises(ValueError, match="no triangle list"):
        PredictionResult(image, hs).get_visibility()
    with pytest.raises(ValueError, match="no triangle list"):
        PredictionResult(image, []).get_visibility()
    with pytest.raises(ValueError, match="triangle index"):
        PredictionResult(image, hs, faces=np.array([[0, 1, heads.shape[1]]])).get_visibility()
    for kw, msg in ((dict(occlusion="painter"), "occlusion"), (dict(z_sign=0.0), "z_sign"), (dict(z_sign=float("nan")), "z_sign")):
        with pytest.raises(ValueError, match=msg):
            visibility.rasterize_heads(heads, tri, H, W, **kw)
    for h, w in ((0, W), (H, 0), (40000, W), (H, 32768)):
        with pytest.raises(ValueError, match="height x width"):
            visibility.rasterize_heads(heads, tri, h, w)
    for bad in (heads[:, :, :2], heads[0, :, 0], heads[None]):
        with pytest.raises(ValueError, match=r"\[n, V, 3\]"):
            visibility.rasterize_heads(bad, tri, H, W)
    with pytest.raises(ValueError, match="triangle index"):
        visibility.rasterize_heads(heads, np.array([[0, 1, -1]]), H, W)
    with pytest.raises(ValueError, match="GPU"):
        visibility.rasterize_heads(torch.zeros(1, 4, 3), tri[:0], H, W)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        pncc.rasterize_triangles(heads, tri, H, W)
    with pytest.raises(ValueError, match="triangle index"):
        pncc.rasterize_triangles(heads[0], np.array([[0, 1, heads.shape[1]]]), H, W)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        pncc.rasterize_triangles(torch.zeros(2, 4, 3), tri[:0], H, W)  # tensors are looked at like arrays
    with pytest.raises(ValueError, match="GPU"):
        pncc.rasterize_triangles(torch.zeros(4, 3), tri[:0], H, W)
    if not torch.cuda.is_available():  # no CPU path: a missing GPU is an error, never another implementation
        with pytest.raises(_lib.VghError, match="GPU"):
            res.get_visibility()
        with pytest.raises(_lib.VghError, match="GPU"):
            visibility.rasterize_heads(heads, tri, H, W)
        with pytest.raises(_lib.VghError, match="GPU"):
            pncc.rasterize_triangles(heads[0], tri, H, W)


def test_head_visibility_class():
    head = np.array([[0, 0, -1], [1, -1, -1]], np.int32)
    hv = visibility.HeadVisibility(head, head.copy(), np.zeros((2, 3), np.float32), None, np.array([2, 1, 0], np.int32), np.array([4, 1, 0], np.int32), np.zeros((3, 5), bool))
    assert hv.mask(0).tolist() == [[True, True, False], [False, False, False]] and hv.mask(0).dtype == bool and not hv.mask(2).any()
    assert hv.visible_fraction.tolist() == [0.5, 1.0, 0.0]
    with pytest.raises(IndexError):
        hv.mask(3)
    t = visibility.HeadVisibility(torch.from_numpy(head), None, None, None, torch.tensor([2, 1, 0], dtype=torch.int32), torch.tensor([4, 1, 0], dtype=torch.int32), None)
    assert t.visible_fraction.tolist() == [0.5, 1.0, 0.0] and t.mask(1).tolist() == [[False, False, False], [True, False, False]]
