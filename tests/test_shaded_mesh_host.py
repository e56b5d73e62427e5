"""The shaded mesh, the host side (no GPU): the CPU restatements of tests/shade_ref.py against the outputs recorded from the reference's own C++
(tests/golden/shaded_mesh.npz, tests/golden/make_golden_shaded.py) and against the live library where oracle/_ref provides it; the two new entry
points' ABI and their argument checks; the errors of the public interface, raised before a GPU is looked for."""
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
from oracle import raster_oracle as ro  # noqa: E402

from head_detector_amd import _lib, _lib_view, mesh_render, pncc  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return np.load(sr.GOLDEN)


def _sources():
    return [False] + ([True] if sr.live() is not None else [])  # the restatement always; the reference's own C++ where it can be had


# ---- tests/shade_ref.py -----------------------------------------------------------------------------------------------------------------------
def test_normals_equal_the_recorded_reference(g):
    unit, etri = sr.ellipsoid()
    cases = [(f"normals_seed{s}",) + ro.random_mesh(s)[:2] for s in sr.NORMAL_SEEDS] + [("normals_corner",) + sr.corner_case_mesh()]
    cases.append(("normals_ellipsoid", sr.ellipsoid_heads(np.random.default_rng(11), 1, 400, 400, 200.0, 200.0, unit)[0], etri))
    for use_live in _sources():
        for key, ver, tri in cases:
            got = sr.normals(ver, tri, use_live)
            assert got.dtype == np.float32 and np.array_equal(got, g[key]), (key, use_live)
    n = g["normals_ellipsoid"]
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert not g["normals_corner"][7].any() and np.isfinite(g["normals_corner"]).all()  # unreferenced vertex: 0 / 1e-6


def test_blended_images_equal_the_recorded_reference(g):
    ver, tri, col = ro.random_mesh(2)
    bg = sr.background(2, sr.BLEND_SHAPE)
    for use_live in _sources():
        for i, alpha in enumerate(sr.ALPHAS):
            for rev in (0, 1):
                want = g[f"blend_a{i}_r{rev}"] ^ bg
                assert np.array_equal(sr.blend(bg.copy(), ver, tri, col, alpha, rev, use_live), want), (alpha, rev, use_live)
        for k, side in enumerate(sr.EDGE_CENTRES):
            ebg = sr.background(10 + k, sr.EDGE_SHAPE)
            assert np.array_equal(sr.blend(ebg.copy(), *sr.edge_mesh(side), 0.6, k % 2, use_live), g[f"edge_{side}"] ^ ebg), (side, use_live)
    # alpha = 1 is the rasteriser this package already had
    assert np.array_equal(g["blend_a3_r0"] ^ bg, ro.rasterize(ver, tri, col, bg)) and np.array_equal(g["blend_a3_r1"] ^ bg, ro.rasterize(ver, tri, col, bg, reverse=True))
    assert not g["blend_a0_r0"].any() and g["blend_a1_r0"].any()
    # the fixture exercises the repeated blend: painting only the winner of every pixel (alpha = 1's winner, blended once) gives another image
    winner = ro.rasterize(ver, tri, col, np.zeros_like(bg))
    covered = (g["blend_a3_r0"] != 0).any(axis=2)
    once = np.where(covered[..., None], (np.float32(0.4) * bg.astype(np.float32) + np.float32(0.6) * winner.astype(np.float32)).astype(np.uint8), bg)
    assert int((once != (g["blend_a2_r0"] ^ bg)).any(axis=2).sum()) >= 1000


def test_render_mesh_composition_equals_the_recorded_reference(g):
    for letter in sr.SCENE_SHAPES:
        bg, heads, tri = sr.scene(letter)
        before = heads.copy()
        for use_live in _sources():
            cols = []
            got = sr.render_mesh(bg, heads, tri, use_live, colors_out=cols)
            assert np.array_equal(got, g[f"scene_{letter}"] ^ bg), (letter, use_live)
            c = np.stack(cols)
            assert c.dtype == np.float32 and c.min() >= 0.35 * 0.75 - 1e-6 and c.max() <= 0.8 and len(np.unique(c[:, :, 0])) > 100
        assert np.array_equal(heads, before)


def test_shade_rule():
    n = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0.6, 0, 0.8], [0, 0, 0]], dtype=np.float32)
    c = sr.shade(n, (0.5, 1.0, 0.25), 0.25, 0.5, (0, 0, 3))
    assert np.array_equal(c[0], np.float32([0.375, 0.75, 0.1875])) and np.array_equal(c[0], c[1])  # two-sided
    assert np.array_equal(c[2], np.float32([0.125, 0.25, 0.0625])) and np.array_equal(c[2], c[4])
    assert np.array_equal(sr.shade(n, (1, 1, 1), 0.75, 0.5, (0, 0, 1))[0], np.float32([1, 1, 1]))  # min(1, .)
    assert np.array_equal(sr.unit_light((0, 0, 1e300)), np.float32([0, 0, 1])) and np.array_equal(sr.unit_light((3, 0, 4)), np.float32([0.6, 0, 0.8]))
    a, col, amb, dif, light = mesh_render.check_shading(0.7, (0.75, 0.75, 0.8), 0.35, 0.65, (3, 0, 4))
    assert np.array_equal(np.float32(light), sr.unit_light((3, 0, 4))) and np.array_equal(np.float32(mesh_render.check_shading(1, (0, 0, 0), 0, 0, (0, 0, 1e300))[4]), [0, 0, 1])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def test_mesh_entry_points_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_view.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghv_[a-z0-9_]+)\s*\(", hdr))
    want = {"vghv_version", "vghv_last_error", "vghv_warp_crops", "vghv_draw_heads", "vghv_vertex_normals", "vghv_render_meshes"}
    assert declared == want and set(_lib_view.SYMBOLS) == want and _exported(_lib_view.LIB_PATH) == want  # exactly 6
    core = {s for s in _exported(_lib.LIB_PATH) if s.startswith("vgh")}
    assert core == set(_lib.SYMBOLS) and len(core) == 86 and _lib.ABI_VERSION == 8 and not any(s.startswith("vghv_") for s in core)
    fields = re.search(r"typedef struct vghv_mesh_job \{(.*?)\} vghv_mesh_job;", hdr, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|$)", decl.strip().replace("*", " "))]
    J = _lib_view.MeshJob
    assert names == [f[0] for f in J._fields_], names
    offsets = {f[0]: getattr(J, f[0]).offset for f in J._fields_}
    assert offsets == {"src_dev": 0, "src_pitch_bytes": 8, "dst_dev": 16, "height": 24, "width": 28, "channels": 32, "n_heads": 36, "n_vertices": 40, "n_triangles": 44,
                       "reverse": 48, "colors_per_head": 52, "shade": 56, "alpha": 60, "z_sign": 64, "ambient": 68, "diffuse": 72, "verts_dev": 80, "triangles": 88, "bounds": 96,
                       "colors_dev": 104, "color": 112, "light": 124}, offsets
    assert C.sizeof(J) == 136


def test_mesh_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib_view.load()
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    bad_tri = np.array([[0, 1, 2], [1, 4, 2]], np.int32)
    bounds = np.array([[0, 0, 7, 7]], np.int32)

    def job(**kw):
        j = _lib_view.MeshJob()
        j.src_dev, j.src_pitch_bytes, j.dst_dev, j.height, j.width, j.channels = 4096, 24, 8192, 8, 8, 3
        j.n_heads, j.n_vertices, j.n_triangles, j.alpha, j.z_sign = 1, 4, 2, 0.5, 1.0
        j.verts_dev, j.triangles, j.bounds, j.colors_dev = 16384, tri.ctypes.data, bounds.ctypes.data, 32768
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(what, **kw):
        assert lib.vghv_render_meshes(job(**kw), None) == -1, what
        assert what.encode() in lib.vghv_last_error(), lib.vghv_last_error()

    refused("null image", src_dev=None)
    refused("null image", dst_dev=None)
    refused("channels", channels=4)
    refused("outside 1 ..", height=40000)
    refused("src_pitch_bytes", src_pitch_bytes=23)
    refused("dst_dev overlaps src_dev", dst_dev=4096 + 100)
    refused("heads outside", n_heads=-1)
    refused("negative count", n_triangles=-1)
    refused("alpha 1.5", alpha=1.5)
    refused("alpha", alpha=float("nan"))
    refused("z_sign", z_sign=0.5)
    refused("shade 2", shade=2)
    refused("colors_per_head", colors_per_head=3)
    refused("null vertices, triangles, bounds or colours", verts_dev=None)
    refused("null vertices, triangles, bounds or colours", bounds=None)
    refused("null vertices, triangles, bounds or colours", colors_dev=None)
    refused("one colour table per head", shade=1, colors_per_head=0)
    refused("not finite", shade=1, colors_per_head=1, ambient=float("inf"))
    refused("colour outside 0 .. 1", shade=1, colors_per_head=1, color=(C.c_float * 3)(0.5, 1.5, 0.5))
    refused("triangle 1: index 4 outside the 4 vertices", triangles=bad_tri.ctypes.data)
    out = np.array([[0, 0, 8, 7]], np.int32)
    refused("head 0: bounds (0, 0, 8, 7) outside the image", bounds=out.ctypes.data)
    assert lib.vghv_render_meshes(None, None) == -1 and b"null job" in lib.vghv_last_error()

    def normals_refused(what, *args):
        assert lib.vghv_vertex_normals(*args, None) == -1, what
        assert what.encode() in lib.vghv_last_error(), lib.vghv_last_error()

    normals_refused("bad sizes", 4096, 1, 0, tri.ctypes.data, 2, 8192)
    normals_refused("bad sizes", 4096, -1, 4, tri.ctypes.data, 2, 8192)
    normals_refused("null vertices or normals", None, 1, 4, tri.ctypes.data, 2, 8192)
    normals_refused("null vertices or normals", 4096, 1, 4, tri.ctypes.data, 2, None)
    normals_refused("null triangles", 4096, 1, 4, None, 2, 8192)
    normals_refused("overlaps", 4096, 1, 4, tri.ctypes.data, 2, 4096)
    normals_refused("triangle 1: index 4 outside the 4 vertices", 4096, 1, 4, bad_tri.ctypes.data, 2, 8192)
    assert lib.vghv_vertex_normals(None, 0, 4, None, 0, None, None) == 0  # no meshes: nothing to do


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_public_argument_errors_come_before_the_gpu():
    bg, heads, tri = sr.scene("A")
    hs = [sr.make_head(h) for h in heads]
    res = PredictionResult(bg, hs, faces=tri)
    for kw, msg in ((dict(alpha=1.5), "alpha"), (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(color=(0.5, 1.2, 0.5)), "color"),
                    (dict(color=(0.5, 0.5)), "color"), (dict(ambient=-1.0), "ambient"), (dict(diffuse=float("inf")), "diffuse"), (dict(light=(0, 0, 0)), "zero vector"),
                    (dict(light=(0, float("nan"), 1)), "light")):
        with pytest.raises(ValueError, match=msg):
            res.render_mesh(**kw)
    with pytest.raises(ValueError, match="no triangle list"):
        PredictionResult(bg, hs).render_mesh()
    with pytest.raises(ValueError, match="triangle index"):
        PredictionResult(bg, hs, faces=np.array([[0, 1, heads.shape[1]]])).render_mesh()
    with pytest.raises(ValueError, match="uint8 image"):
        PredictionResult(bg.astype(np.float32), hs, faces=tri).render_mesh()
    ver, mtri, col = ro.random_mesh(2)
    for alpha in (1.5, -0.25, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            pncc.rasterize(ver, mtri, col, bg=bg.copy(), alpha=alpha)
    with pytest.raises(ValueError, match="3 channels"):
        pncc.rasterize(ver, mtri, np.zeros((ver.shape[0], 4), np.float32), height=16, width=16, channel=4, alpha=0.5)
    with pytest.raises(ValueError, match="triangle index"):
        pncc.rasterize(ver, np.array([[0, 1, ver.shape[0]]], np.int32), col, bg=bg.copy(), alpha=0.5)
    with pytest.raises(ValueError, match="triangle index"):
        pncc.get_normal(ver, np.array([[0, 1, ver.shape[0]]], np.int32))
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        pncc.get_normal(ver[:, :2], mtri)
    with pytest.raises(ValueError, match="GPU"):
        pncc.get_normal(torch.zeros(1, 4, 3), mtri[:0])
    import inspect

    assert list(inspect.signature(pncc.rasterize).parameters)[-1] == "alpha" and inspect.signature(pncc.rasterize).parameters["alpha"].default == 1.0
    if not torch.cuda.is_available():  # no CPU path: a missing GPU is an error, never another implementation
        with pytest.raises(_lib.VghError, match="GPU"):
            res.render_mesh()
        with pytest.raises(_lib.VghError, match="GPU"):
            pncc.rasterize(ver, mtri, col, bg=bg.copy(), alpha=0.5)
        with pytest.raises(_lib.VghError, match="GPU"):
            pncc.get_normal(ver, mtri)
