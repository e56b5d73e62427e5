"""The shaded mesh on the MI355X: csrc/mesh_render.hip (libvghview.so) against the reference's own C++ -- its recorded outputs (tests/golden/shaded_mesh.npz)
and, where oracle/_ref provides it, the live library (otherwise the CPU restatement tests/shade_ref.py, which tests/test_shaded_mesh_host.py holds to the
same outputs).  Every comparison is np.array_equal / torch.equal: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402

from head_detector_amd import mesh_render, pncc  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _live():
    return sr.live() is not None


def _same(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, getattr(got, "shape", None))
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, int((got != want).sum()), "values differ")


def test_normals_equal_the_reference(gpu_lib):
    g = np.load(sr.GOLDEN)
    for seed in sr.NORMAL_SEEDS:
        ver, tri, _ = ro.random_mesh(seed)
        got = pncc.get_normal(ver, tri)
        _same(got, g[f"normals_seed{seed}"], ("recorded", seed))
        _same(got, sr.normals(ver, tri, _live()), ("random_mesh", seed))
    ver, tri = sr.corner_case_mesh()  # a zero-area triangle, an unreferenced vertex, a triangle naming one vertex twice
    got = pncc.get_normal(ver, tri)
    _same(got, g["normals_corner"], "corner cases")
    assert not got[7].any()
    _same(pncc.get_normal(ver, tri[:0]), np.zeros_like(ver), "no triangles")
    _same(pncc.get_normal(ver.astype(np.float64), tri.astype(np.int64)), g["normals_corner"], "other dtypes are converted")
    unit, etri = sr.ellipsoid()
    assert unit.shape == (5002, 3) and etri.shape == (10000, 3)
    one = sr.ellipsoid_heads(np.random.default_rng(11), 1, 400, 400, 200.0, 200.0, unit)
    _same(pncc.get_normal(one[0], etri), g["normals_ellipsoid"], "ellipsoid, recorded")
    heads = sr.ellipsoid_heads(np.random.default_rng(12), 100, 3000, 4000, 100.0, 300.0, unit)
    for n in (1, 3, 100):
        v = torch.from_numpy(heads[:n]).to(_dev())
        before = v.clone()
        got = pncc.get_normal(v, etri)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, 5002, 3) and torch.equal(v, before)
        want = torch.from_numpy(np.stack([sr.normals(h, etri, _live()) for h in heads[:n]]))
        assert torch.equal(got.cpu(), want), (n, int((got.cpu() != want).sum()))
    assert tuple(pncc.get_normal(torch.zeros(0, 5002, 3, device=_dev()), etri).shape) == (0, 5002, 3)
    bad = heads[0].copy()
    bad[17] = np.nan  # NaN spreads to the neighbours exactly as in the reference
    _same(pncc.get_normal(bad, etri), sr.normals(bad, etri, _live()), "a NaN vertex")


def _c_call(bg, ver, tri, col, alpha, reverse):
    out = mesh_render.blend_meshes(bg, torch.from_numpy(ver).to(_dev()).unsqueeze(0), tri, alpha=alpha, z_sign=1.0, reverse=reverse, colors=torch.from_numpy(col).to(_dev()))
    return out.cpu().numpy()


def test_blended_raster_equals_the_reference(gpu_lib):
    g = np.load(sr.GOLDEN)
    ver, tri, col = ro.random_mesh(2)
    bg = sr.background(2, sr.BLEND_SHAPE)
    for i, alpha in enumerate(sr.ALPHAS):
        for rev in (0, 1):
            want = g[f"blend_a{i}_r{rev}"] ^ bg
            _same(want, sr.blend(bg.copy(), ver, tri, col, alpha, rev, _live()), ("fixture against the reference", alpha, rev))
            _same(_c_call(bg, ver, tri, col, alpha, bool(rev)), want, ("C call", alpha, rev))
            img = bg.copy()
            ret = pncc.rasterize(ver, tri, col, bg=img, reverse=bool(rev), alpha=alpha)  # alpha == 1.0: the old path, untouched
            assert ret is img  # like the reference, bg itself is painted and returned
            _same(img, want, ("pncc.rasterize", alpha, rev))
    _same(pncc.rasterize(ver, tri, col, bg=bg.copy()), g["blend_a3_r0"] ^ bg, "no alpha given")
    _same(pncc.rasterize(ver, tri, col, height=128, width=128, channel=3, alpha=0.6), sr.blend(np.zeros_like(bg), ver, tri, col, 0.6, 0, _live()), "no bg given")
    # sizes that are not multiples of 16, a mesh hanging over each edge
    for k, side in enumerate(sr.EDGE_CENTRES):
        ebg = sr.background(10 + k, sr.EDGE_SHAPE)
        ever, etri, ecol = sr.edge_mesh(side)
        want = g[f"edge_{side}"] ^ ebg
        _same(pncc.rasterize(ever, etri, ecol, bg=ebg.copy(), reverse=bool(k % 2), alpha=0.6), want, ("edge", side))
        for alpha in (0.0, 0.25, 1.0):
            for rev in (False, True):
                _same(_c_call(ebg, ever, etri, ecol, alpha, rev), sr.blend(ebg.copy(), ever, etri, ecol, alpha, rev, _live()), ("edge", side, alpha, rev))
    # odd little images, a mesh far larger than the image, -0.0 and NaN depths, a non-finite corner
    rng = np.random.default_rng(8)
    for shape in ((1, 1, 3), (3, 37, 3), (17, 16, 3), (33, 5, 3)):
        small = rng.integers(0, 256, shape, dtype=np.uint8)
        mver, mtri, mcol = ro.random_mesh(5, n_side=6, size=70.0, centre=(shape[1] / 2, shape[0] / 2))
        for rev in (False, True):
            _same(_c_call(small, mver, mtri, mcol, 0.25, rev), sr.blend(small.copy(), mver, mtri, mcol, 0.25, rev, _live()), (shape, rev))
    odd = ver.copy()
    odd[::7, 2] = -0.0
    odd[5, 2] = np.nan
    odd[11, 0] = np.inf
    odd[13, 1] = np.nan
    _same(_c_call(bg, odd, tri, col, 0.6, False), sr.blend(bg.copy(), odd, tri, col, 0.6, False, _live()), "odd depths and corners")
    # a GPU image that is a pitched view, shared and per-mesh colours, two meshes in order
    wide = torch.from_numpy(sr.background(3, (128, 141, 3))).to(_dev())
    view = wide[:, 5:133]
    vbg = view.cpu().numpy()
    v2 = ro.random_mesh(2, centre=(50.0, 70.0))[0]
    c2 = col[::-1].copy()
    both = torch.from_numpy(np.stack([ver, v2])).to(_dev())
    want = sr.blend(sr.blend(vbg.copy(), ver, tri, col, 0.25, False, _live()), v2, tri, c2, 0.25, False, _live())
    got = mesh_render.blend_meshes(view, both, tri, alpha=0.25, z_sign=1.0, colors=torch.from_numpy(np.stack([col, c2])).to(_dev()))
    _same(got.cpu().numpy(), want, "two meshes, per-mesh colours")
    want = sr.blend(sr.blend(vbg.copy(), ver, tri, col, 0.25, False, _live()), v2, tri, col, 0.25, False, _live())
    _same(mesh_render.blend_meshes(view, both, tri, alpha=0.25, z_sign=1.0, colors=torch.from_numpy(col).to(_dev())).cpu().numpy(), want, "two meshes, shared colours")
    assert np.array_equal(view.cpu().numpy(), vbg)


def test_render_mesh_equals_the_composition(gpu_lib):
    g = np.load(sr.GOLDEN)
    for letter in sr.SCENE_SHAPES:
        bg, heads, tri = sr.scene(letter)
        hs = [sr.make_head(h) for h in heads]
        before = bg.copy()
        res = PredictionResult(bg, hs, faces=tri)
        want = g[f"scene_{letter}"] ^ bg
        got = res.render_mesh()
        _same(got, want, ("scene", letter))
        assert got is not bg and not np.shares_memory(got, bg) and np.array_equal(bg, before)
        for h, v in zip(hs, heads):
            assert np.array_equal(h.vertices_3d, v)  # unlike get_pncc, no z flip is left behind
        on_dev = PredictionResult(torch.from_numpy(bg).to(_dev()), hs, faces=tri).render_mesh(to_host=False)
        assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.uint8 and torch.equal(on_dev.cpu(), torch.from_numpy(want))
        # the colours the device computed, and other shading arguments
        kw = dict(alpha=0.4, color=(1.0, 0.5, 0.25), ambient=0.1, diffuse=1.2, light=(1.0, -2.0, 0.5))
        cols = []
        want2 = sr.render_mesh(bg, heads, tri, _live(), colors_out=cols, **kw)
        got2, dev_cols = mesh_render.render_mesh(bg, hs, tri, return_colors=True, **kw)
        assert torch.equal(dev_cols.cpu(), torch.from_numpy(np.stack(cols))), "per-vertex colours"
        assert float(dev_cols.max()) == 1.0  # min(1, .) bites with diffuse = 1.2
        _same(got2, want2, ("scene, other shading", letter))
        _same(res.render_mesh(alpha=1.0), sr.render_mesh(bg, heads, tri, _live(), alpha=1.0), ("opaque", letter))
        _same(res.render_mesh(alpha=0.0), bg, ("alpha = 0", letter))
        _same(PredictionResult(bg, hs[::-1], faces=tri).render_mesh(), sr.render_mesh(bg, heads[::-1], tri, _live()), ("reversed heads", letter))
        # no heads: a copy
        empty = PredictionResult(bg, [], faces=tri).render_mesh()
        _same(empty, bg, "no heads")
        assert empty is not bg and not np.shares_memory(empty, bg)
        e = PredictionResult(torch.from_numpy(bg).to(_dev()), [], faces=tri).render_mesh(to_host=False)
        assert e.is_cuda and np.array_equal(e.cpu().numpy(), bg)


def test_hundred_heads_on_a_large_pitched_image(gpu_lib):
    """3000 x 4000, a strided view of a wider GPU tensor, 100 ellipsoids of FLAME's size (5 002 vertices, 10 000 triangles) of 100 .. 300 px, some hanging over
    the edges, against the composition run on the CPU."""
    H, W, n = 3000, 4000, 100
    gen = torch.Generator().manual_seed(19)
    wide = torch.randint(0, 256, (H, W + 37, 3), dtype=torch.uint8, generator=gen).to(_dev())
    view = wide[:, :W]
    assert view.stride(0) > 3 * W
    img = view.cpu().numpy()
    unit, tri = sr.ellipsoid()
    heads = sr.ellipsoid_heads(np.random.default_rng(29), n, H, W, 100.0, 300.0, unit, spread=1.02)
    x, y = heads[:, :, 0], heads[:, :, 1]
    over = {"left": int((x.min(1) < 0).sum()), "right": int((x.max(1) > W - 1).sum()), "top": int((y.min(1) < 0).sum()), "bottom": int((y.max(1) > H - 1).sum())}
    print("heads over the edges:", over)
    assert min(over.values()) >= 1, over
    cols = []
    want = sr.render_mesh(img, heads, tri, _live(), colors_out=cols)
    hs = [sr.make_head(h) for h in heads]
    got, dev_cols = mesh_render.render_mesh(view, hs, tri, to_host=False, return_colors=True)
    assert got.is_cuda and torch.equal(dev_cols.cpu(), torch.from_numpy(np.stack(cols)))
    painted = int((want != img).any(axis=2).sum())
    print(f"{painted} painted pixels")
    assert painted > 1_000_000
    _same(got.cpu().numpy(), want, "100 heads, pitched view")
    assert np.array_equal(view.cpu().numpy(), img)
    for h, v in zip(hs, heads):
        assert np.array_equal(h.vertices_3d, v)
    _same(PredictionResult(img, hs[:16], faces=tri).render_mesh(), sr.render_mesh(img, heads[:16], tri, _live()), "16 heads, numpy image")
