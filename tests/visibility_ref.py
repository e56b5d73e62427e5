"""TEST INFRASTRUCTURE.  Head visibility buffers on the CPU: restatements of

  is_point_in_tri(p, p0, p1, p2)                        head_detector/Sim3DR/lib/rasterize_kernel.cpp:26-52   (u >= 0 && v >= 0 && u + v < 1)
  rasterize_triangles(vertices, triangles, depth, triangle, weights)    ``_rasterize_triangles`` (:295-353), writing the three buffers in place

and the composition ``head_detector_amd.visibility`` is defined as (``compose``): per head one solo call on fresh buffers, then either the painter's
order or one shared z-buffer, and the per-head pixel counts and vertex flags derived from them.  Where oracle/_ref/libsim3dr_ref.so exists
(oracle/build_ref.py), ``live()`` binds the reference's own C++ ``ref_rasterize_triangles`` and ``compose(..., use_live=True)`` runs it instead:
PINNED, tests/golden/visibility.npz holds that library's outputs and tests/test_visibility_host.py holds the restatement to them.  All arithmetic is
float32 in the reference's operation order.

Also the inputs the fixture and the tests share (generated from seeds, never stored) and the fixture's compact encoding."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "visibility.npz")
BACKGROUND = f32(-1e8)
FIELDS = ("head_index", "triangle_index", "depth", "barycentric", "visible_pixels", "covered_pixels", "vertex_visible")


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------
def is_point_in_tri(px, py, p0, p1, p2, rule: str = "ge"):
    """-> (inside, w0, w1, w2) for arrays of pixel centres.  u and v are get_point_weight's (the two functions compute them by the same operations).
    ``rule="gt"`` is NOT the reference: the inside rule of ``_rasterize`` (all three weights > 0), kept to show that the two differ."""
    w0, v, u = ro._weights(px, py, p0, p1, p2)
    if rule == "gt":
        return (u > 0) & (v > 0) & (w0 > 0), w0, v, u
    return (u >= 0) & (v >= 0) & ((u + v).astype(f32) < 1), w0, v, u


def rasterize_triangles(vertices, triangles, depth, triangle, weights, rule: str = "ge") -> None:
    """``_rasterize_triangles`` on the caller's buffers (float32 [H, W], int32 [H, W], float32 [H, W, 3]), in place.  A triangle with a non-finite x or
    y is skipped ((int)ceil(nan) is undefined in C; such a triangle never covers a pixel)."""
    h, w = depth.shape
    ver, tri = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for t in range(tri.shape[0]):
            i0, i1, i2 = (int(k) for k in tri[t])
            p0, p1, p2 = ver[i0], ver[i1], ver[i2]
            xs, ys = (p0[0], p1[0], p2[0]), (p0[1], p1[1], p2[1])
            if not all(math.isfinite(float(q)) for q in xs + ys):
                continue
            x_min, x_max = max(int(math.ceil(min(xs))), 0), min(int(math.floor(max(xs))), w - 1)
            y_min, y_max = max(int(math.ceil(min(ys))), 0), min(int(math.floor(max(ys))), h - 1)
            if x_max < x_min or y_max < y_min:
                continue
            py, px = np.meshgrid(np.arange(y_min, y_max + 1, dtype=f32), np.arange(x_min, x_max + 1, dtype=f32), indexing="ij")
            inside, w0, w1, w2 = is_point_in_tri(px, py, p0, p1, p2, rule)
            pd = (((w0 * p0[2]).astype(f32) + (w1 * p1[2]).astype(f32)).astype(f32) + (w2 * p2[2]).astype(f32)).astype(f32)
            sub = depth[y_min : y_max + 1, x_min : x_max + 1]
            win = inside & (pd > sub)  # false for NaN
            if not win.any():
                continue
            sub[win] = pd[win]
            triangle[y_min : y_max + 1, x_min : x_max + 1][win] = t
            weights[y_min : y_max + 1, x_min : x_max + 1][win] = np.stack([w0, w1, w2], axis=-1)[win]


# ---- the reference's own C++ -------------------------------------------------------------------------------------------------------------------
def live():
    """oracle/_ref/libsim3dr_ref.so (``ref_rasterize_triangles``), or None where the library cannot be had."""
    return sr.live()


def one_call(vertices, triangles, depth, triangle, weights, use_live: bool, rule: str = "ge") -> None:
    """One ``Sim3DR_Cython.rasterize_triangles`` call on the caller's contiguous buffers."""
    if not use_live:
        return rasterize_triangles(vertices, triangles, depth, triangle, weights, rule)
    assert rule == "ge"
    v, t = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    for a, dt in ((depth, f32), (triangle, np.int32), (weights, f32)):
        assert a.flags.c_contiguous and a.dtype == dt
    h, w = depth.shape
    live().ref_rasterize_triangles(v.ctypes.data, t.ctypes.data, depth.ctypes.data, triangle.ctypes.data, weights.ctypes.data, t.shape[0], h, w)


def _window(v, H, W):
    """Rows and columns that hold every pixel the mesh can cover (the whole image for a mesh with a non-finite coordinate)."""
    xy = v[:, :2]
    if xy.size == 0 or not np.isfinite(xy).all():
        return slice(0, H), slice(0, W)
    x0, y0 = max(math.ceil(float(xy[:, 0].min())), 0), max(math.ceil(float(xy[:, 1].min())), 0)
    x1, y1 = min(math.floor(float(xy[:, 0].max())), W - 1), min(math.floor(float(xy[:, 1].max())), H - 1)
    return slice(y0, max(y1 + 1, y0)), slice(x0, max(x1 + 1, x0))


def compose(heads_vertices, triangles, H: int, W: int, occlusion: str = "order", z_sign: float = 1.0, use_live: bool = False, rule: str = "ge") -> dict:
    """The composition ``visibility.rasterize_heads`` is defined as -> the seven outputs (``FIELDS``).  The solo buffers are allocated once and only the
    head's window is looked at and reset, so that many heads on a large image stay affordable."""
    assert occlusion in ("order", "depth")
    heads = np.asarray(heads_vertices, dtype=f32)
    heads = heads[None] if heads.ndim == 2 else heads
    tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    n, V = heads.shape[0], heads.shape[1]
    out = dict(head_index=np.full((H, W), -1, np.int32), triangle_index=np.full((H, W), -1, np.int32), depth=np.full((H, W), BACKGROUND, f32),
               barycentric=np.zeros((H, W, 3), f32), visible_pixels=np.zeros(n, np.int32), covered_pixels=np.zeros(n, np.int32), vertex_visible=np.zeros((n, V), bool))
    s_depth, s_tri, s_bary = np.full((H, W), BACKGROUND, f32), np.full((H, W), -1, np.int32), np.zeros((H, W, 3), f32)
    for i in range(n):
        v = np.array(heads[i], dtype=f32)  # a copy: the head's own array is not modified
        v[:, 2] *= f32(z_sign)
        one_call(v, tri, s_depth, s_tri, s_bary, use_live, rule)
        win = _window(v, H, W)
        m = s_tri[win] >= 0
        out["covered_pixels"][i] = int(m.sum())
        if occlusion == "order":
            out["head_index"][win][m] = i
            for key, buf in (("triangle_index", s_tri), ("depth", s_depth), ("barycentric", s_bary)):
                out[key][win][m] = buf[win][m]
        else:
            before = out["depth"][win].copy()
            one_call(v, tri, out["depth"], out["triangle_index"], out["barycentric"], use_live, rule)
            out["head_index"][win][out["depth"][win] != before] = i
        s_depth[win], s_tri[win], s_bary[win] = BACKGROUND, -1, 0
    derive(out, tri)
    return out


def derive(out: dict, tri: np.ndarray) -> None:
    """visible_pixels and vertex_visible from the final owner buffers."""
    n = out["visible_pixels"].shape[0]
    own = out["head_index"] >= 0
    out["visible_pixels"][:] = np.bincount(out["head_index"][own], minlength=n)[:n] if n else 0
    out["vertex_visible"][:] = False
    if n and own.any():
        pairs = np.unique(np.stack([out["head_index"][own], out["triangle_index"][own]], axis=1), axis=0)
        for k in range(3):
            out["vertex_visible"][pairs[:, 0], tri[pairs[:, 1], k]] = True


def same(got: dict, want: dict, what) -> None:
    """Exact equality of all seven outputs (no tolerance)."""
    for key in FIELDS:
        a, b = got[key], want[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, key, int((a != b).sum()), "values differ")


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------------------
def integer_grid_mesh():
    """Vertices on integer pixel positions (every edge and every vertex lies on pixel centres, where the inside rules differ), two triangles a cell with
    alternating diagonals, a depth that varies, on a 16 x 16 canvas."""
    g = np.arange(5) * 3 + 1
    yy, xx = np.meshgrid(g, g, indexing="ij")
    ver = np.stack([xx.ravel(), yy.ravel(), ((xx * 7 + yy * 3) % 5).ravel()], axis=1).astype(f32)
    idx = np.arange(25).reshape(5, 5)
    tri = []
    for r in range(4):
        for c in range(4):
            a, b, d, e = idx[r, c], idx[r, c + 1], idx[r + 1, c], idx[r + 1, c + 1]
            tri += [[a, b, d], [b, e, d]] if (r + c) % 2 == 0 else [[a, b, e], [a, e, d]]
    return ver, np.array(tri, dtype=np.int32)


def corner_case():
    """shade_ref.corner_case_mesh scaled by 3 on 16 x 16: its triangle 5 ([4, 4, 1]) has a zero determinant and holds a 7 x 7 block."""
    ver, tri = sr.corner_case_mesh()
    return (ver * f32(3)).astype(f32), tri


def scene(letter: str):
    """(H, W), the 8 overlapping heads and the triangles of shade_ref.scene."""
    bg, heads, tri = sr.scene(letter)
    return bg.shape[:2], heads, tri


def edge_mesh(side: str):
    """A folded sheet hanging over one edge of shade_ref.EDGE_SHAPE (sides that are not multiples of 16); smaller than shade_ref.edge_mesh to keep the
    fixture small."""
    return ro.random_mesh(40 + list(sr.EDGE_CENTRES).index(side), n_side=10, size=38.0, centre=sr.EDGE_CENTRES[side], depth_scale=30.0)[:2]


def single_cases():
    """name -> (vertices [V, 3], triangles, (H, W)): one mesh each, z_sign = +1."""
    cases = {"corner": corner_case() + ((16, 16),), "grid": integer_grid_mesh() + ((16, 16),), "random": ro.random_mesh(2, size=55.0)[:2] + ((128, 128),)}
    for side in sr.EDGE_CENTRES:
        cases[f"edge_{side}"] = edge_mesh(side) + (sr.EDGE_SHAPE[:2],)
    return cases


SCENE_Z_SIGN = -1.0  # what PredictionResult.get_visibility uses


# ---- the fixture's encoding ------------------------------------------------------------------------------------------------------------------------
# Depth and weights are functions of (head, triangle, pixel); a case stores them only for owned pixels, and a scene's depth mode only where (head,
# triangle) differs from its order mode.  w0 is stored as what it is: float32(float32(1 - u) - v) (asserted when the fixture is recorded).
def encode(res: dict, base: dict = None) -> dict:
    own = res["head_index"] >= 0
    keep = own if base is None else own & ((res["head_index"] != base["head_index"]) | (res["triangle_index"] != base["triangle_index"]))
    b = res["barycentric"]
    enc = dict(head=res["head_index"].astype(np.int16), tri=res["triangle_index"].astype(np.int16), depth=res["depth"][keep], u=b[..., 2][keep], v=b[..., 1][keep],
               visible=res["visible_pixels"], covered=res["covered_pixels"], vv=np.packbits(res["vertex_visible"], axis=1), nv=np.int32(res["vertex_visible"].shape[1]))
    assert np.array_equal(enc["head"], res["head_index"]) and np.array_equal(enc["tri"], res["triangle_index"])
    return enc


def decode(enc: dict, base: dict = None) -> dict:
    head, tri = enc["head"].astype(np.int32), enc["tri"].astype(np.int32)
    own = head >= 0
    keep = own if base is None else own & ((head != base["head_index"]) | (tri != base["triangle_index"]))
    depth, bary = np.full(head.shape, BACKGROUND, f32), np.zeros(head.shape + (3,), f32)
    if base is not None:
        share = own & ~keep
        depth[share], bary[share] = base["depth"][share], base["barycentric"][share]
    u, v = enc["u"].astype(f32), enc["v"].astype(f32)
    depth[keep] = enc["depth"]
    bary[keep] = np.stack([((f32(1.0) - u).astype(f32) - v).astype(f32), v, u], axis=-1)
    vv = np.unpackbits(enc["vv"], axis=1)[:, : int(enc["nv"])].astype(bool)
    return dict(head_index=head, triangle_index=tri, depth=depth, barycentric=bary, visible_pixels=enc["visible"].astype(np.int32),
                covered_pixels=enc["covered"].astype(np.int32), vertex_visible=vv)


def golden_case(g, name: str, base: dict = None) -> dict:
    keys = ("head", "tri", "depth", "u", "v", "visible", "covered", "vv", "nv")
    return decode({k: g[f"{name}.{k}"] for k in keys}, base)
