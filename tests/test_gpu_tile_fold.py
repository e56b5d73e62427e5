"""The one piece csrc/mesh_render.hip, csrc/visibility.hip and csrc/texture.hip share on the device (csrc/tile_fold.h: boxes, set-up, the compaction of a
256-triangle chunk) on the MI355X.  A stack of T triangles that all overlap one 16 x 16 tile, almost all of them beating the depth so far, so that the
blended byte of a pixel depends on the ORDER in which the lanes walk the compacted list: T = 255 / 256 / 257 / 513 put the chunk boundary, the fourth
wave's prefix and a partial last chunk under it, 17 x 33 adds partial tiles.  Bit for bit against the CPU restatements (tests/shade_ref.py,
tests/visibility_ref.py, tests/texture_ref.py), which the host tests hold to the reference's recorded outputs.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import texture_ref as tr  # noqa: E402
import visibility_ref as vr  # noqa: E402

from head_detector_amd import mesh_render, texture, visibility  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
OFFSETS = (f32([0.0, 0.0, 0.0]), f32([13.25, 0.5, 100.25]))  # the second head reaches the 17 x 33 image's other tiles and lies in front of most of the first


def stack(T: int):
    """T triangles of their own three vertices each ([3 T, 3], [T, 3]) around the middle of tile (0, 0): triangle k is the first one turned by k small steps,
    a little smaller or larger, at depth about k -- so it beats everything before it wherever it lies -- but for every seventh, which lies behind its
    predecessors.  The three depths of a triangle differ, so the interpolated depth does too."""
    rng = np.random.default_rng(T)
    k = np.arange(T, dtype=np.float64)
    angle = k[:, None] * 0.37 + np.array([0.0, 2.1, 4.2])[None, :] + rng.uniform(-0.2, 0.2, (T, 3))
    radius = rng.uniform(5.0, 11.0, (T, 3))
    ver = np.zeros((T, 3, 3), np.float64)
    ver[..., 0], ver[..., 1] = 7.6 + radius * np.cos(angle), 7.4 + radius * np.sin(angle)
    ver[..., 2] = np.where(k % 7 == 6, k - 20.0, k)[:, None] + rng.uniform(0.0, 0.5, (T, 3))
    return ver.reshape(3 * T, 3).astype(f32), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


@pytest.fixture(scope="module", params=[1, 255, 256, 257, 513])
def case(request):
    """The stack and what goes with it, built once per T: per-vertex colours, texture coordinates and a texture."""
    T = request.param
    ver, tri = stack(T)
    rng = np.random.default_rng(1000 + T)
    return dict(T=T, ver=ver, tri=tri, col=rng.uniform(0.0, 1.0, (3 * T, 3)).astype(f32), coords=np.concatenate([rng.uniform(-1.0, 9.0, (3 * T, 2)), np.zeros((3 * T, 1))], axis=1).astype(f32),
                tex=rng.uniform(0.0, 255.0, (8, 9, 3)).astype(f32))


def _heads(case, n):
    return np.stack([case["ver"] + OFFSETS[i] for i in range(n)])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("shape", [(16, 16), (17, 33)])
def test_blended_mesh(gpu_lib, case, shape, n):
    H, W = shape
    heads, tri, col = _heads(case, n), case["tri"], case["col"]
    bg = sr.background(case["T"], (H, W, 3))
    want, counts = bg.copy(), np.zeros((H, W), np.int64)
    for v in heads:
        sr.rasterize(want, v, tri, col, 0.5, counts=counts)
    if n == 1:  # the inputs bite: six triangles of seven beat their predecessors, so a pixel they all hold is blended by most of them, in their order
        assert counts.max() >= (case["T"] + 1) // 2, counts.max()
    dev = torch.device("cuda", torch.cuda.current_device())
    got = mesh_render.blend_meshes(bg, torch.from_numpy(heads).to(dev), tri, alpha=0.5, z_sign=1.0, colors=torch.from_numpy(col).to(dev)).cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (case["T"], shape, n, int((got != want).sum()), "bytes differ")


@pytest.mark.parametrize("mode", ["order", "depth"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("shape", [(16, 16), (17, 33)])
def test_visibility(gpu_lib, case, shape, n, mode):
    H, W = shape
    heads, tri = _heads(case, n), case["tri"]
    res = visibility.rasterize_heads(heads, tri, H, W, occlusion=mode, z_sign=1.0)
    want = vr.compose(heads, tri, H, W, mode, 1.0, False)
    vr.same({k: getattr(res, k) for k in vr.FIELDS}, want, (case["T"], shape, n, mode))


@pytest.mark.parametrize("mode", ["order", "depth"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("shape", [(16, 16), (17, 33)])
def test_texture_wrap(gpu_lib, case, shape, n, mode):
    H, W = shape
    heads, tri = _heads(case, n), case["tri"]
    out = texture.render_texture(heads, tri, case["tex"], case["coords"], H, W, channels=3, mapping="nearest", occlusion=mode, z_sign=1.0, with_buffers=True)
    want = tr.compose(heads, tri, case["tex"], case["coords"], H, W, 3, "nearest", mode, 1.0)
    tr.same(dict(zip(tr.FIELDS, out)), want, (case["T"], shape, n, mode))
