"""TEST INFRASTRUCTURE.  The shaded mesh on the CPU, for machines without the reference's library: restatements of the three rules

  get_normal(vertices, triangles)                      Sim3DR ``_get_normal`` (head_detector/Sim3DR/lib/rasterize_kernel.cpp:158-215)
  shade(normals, color, ambient, diffuse, light)       the lighting rule of head_detector_amd/mesh_render.py (ours, not the reference's)
  rasterize(image, vertices, triangles, colors, alpha, reverse)   Sim3DR ``_rasterize`` with any alpha (:219-293), painting ``image`` in place

and the composition ``render_mesh`` they define.  Where oracle/_ref/libsim3dr_ref.so exists (oracle/build_ref.py), ``live()`` binds the reference's own
C++ and ``normals`` / ``blend`` / ``render_mesh`` run it instead (``use_live=True``): PINNED, tests/golden/shaded_mesh.npz holds that library's outputs
and tests/test_shaded_mesh_host.py holds the restatements to them.  All arithmetic is float32 in the reference's operation order.

Also the inputs the fixture and the tests share (meshes and scenes are generated from seeds, never stored)."""
from __future__ import annotations

import ctypes
import math
import os
import sys
import types
from typing import Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import raster_oracle as ro  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "shaded_mesh.npz")
DEFAULTS = dict(alpha=0.7, color=(0.75, 0.75, 0.8), ambient=0.35, diffuse=0.65, light=(0.0, 0.0, 1.0))


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------
def get_normal(vertices: np.ndarray, triangles: np.ndarray) -> np.ndarray:
    v = np.ascontiguousarray(vertices, dtype=f32)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        a, b = p1 - p0, p2 - p0
        tn = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)
        acc = np.zeros_like(v)
        np.add.at(acc, t.reshape(-1), np.repeat(tn, 3, axis=0))  # unbuffered, in the order given: triangle by triangle, corner 0, 1, 2
        det = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]).astype(f32)
        det = np.where(det <= 0, f32(1e-6), det)
        return (acc / det[:, None]).astype(f32)


def unit_light(light) -> np.ndarray:
    """float64 normalisation (scaled by the largest component first), rounded to float32: what render_mesh hands to the device."""
    m = max(abs(float(c)) for c in light)
    s = [float(c) / m for c in light]
    n = math.sqrt(sum(c * c for c in s))
    return np.array([c / n for c in s], dtype=f32)


def shade(normals: np.ndarray, color=DEFAULTS["color"], ambient=DEFAULTS["ambient"], diffuse=DEFAULTS["diffuse"], light=DEFAULTS["light"]) -> np.ndarray:
    n = np.asarray(normals, dtype=f32)
    l, col = unit_light(light), np.array(color, dtype=f32)
    with np.errstate(all="ignore"):
        s = np.abs((n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2]).astype(f32)
        a = (f32(ambient) + f32(diffuse) * s).astype(f32)
        t = np.where(a < 1, a, f32(1.0)).astype(f32)
        return (t[:, None] * col[None, :]).astype(f32)


def rasterize(image: np.ndarray, vertices: np.ndarray, triangles: np.ndarray, colors: np.ndarray, alpha: float, reverse: bool = False,
              counts: Optional[np.ndarray] = None) -> np.ndarray:
    """``_rasterize`` with a fresh depth buffer of -1e8; paints uint8 [H, W, 3] ``image`` in place.  ``counts`` (int [H, W], geometry rows) is incremented for
    every paint of a pixel."""
    h, w, c = image.shape
    ver, col, tri = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(colors, dtype=f32), np.ascontiguousarray(triangles, dtype=np.int32)
    zb = np.full((h, w), f32(-1e8), dtype=f32)
    alpha = f32(alpha)
    one_minus, a255 = f32(f32(1.0) - alpha), f32(alpha * f32(255.0))
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
            w0, w1, w2 = ro._weights(px, py, p0, p1, p2)
            pd = (((w0 * p0[2]).astype(f32) + (w1 * p1[2]).astype(f32)).astype(f32) + (w2 * p2[2]).astype(f32)).astype(f32)
            sub = zb[y_min : y_max + 1, x_min : x_max + 1]
            win = (w2 > 0) & (w1 > 0) & (w0 > 0) & (pd > sub)
            if not win.any():
                continue
            view = image[h - 1 - y_max : h - y_min, x_min : x_max + 1][::-1] if reverse else image[y_min : y_max + 1, x_min : x_max + 1]
            for k in range(c):
                pc = (((w0 * col[i0, k]).astype(f32) + (w1 * col[i1, k]).astype(f32)).astype(f32) + (w2 * col[i2, k]).astype(f32)).astype(f32)
                val = ((one_minus * view[..., k].astype(f32)).astype(f32) + (a255 * pc).astype(f32)).astype(f32)
                view[..., k] = np.where(win, (val.astype(np.int64) & 0xFF).astype(np.uint8), view[..., k])
            sub[win] = pd[win]
            if counts is not None:
                counts[y_min : y_max + 1, x_min : x_max + 1] += win
    return image


# ---- the reference's own C++ --------------------------------------------------------------------------------------------------------------
_live = [False, None]


def live():
    """oracle/_ref/libsim3dr_ref.so with ``_get_normal`` bound through its mangled name, or None where the library cannot be had."""
    if not _live[0]:
        from oracle import build_ref

        lib = build_ref.load()
        if lib is not None:
            fn = getattr(lib, "_Z11_get_normalPfS_Piii")
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int], None
            lib.get_normal = fn
        _live[:] = [True, lib]
    return _live[1]


def normals(vertices, triangles, use_live: bool) -> np.ndarray:
    if not use_live:
        return get_normal(vertices, triangles)
    v, t = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(triangles, dtype=np.int32)
    out = np.zeros_like(v)  # Sim3DR.py:10
    live().get_normal(out.ctypes.data, v.ctypes.data, t.ctypes.data, v.shape[0], t.shape[0])
    return out


def blend(image, vertices, triangles, colors, alpha, reverse, use_live: bool) -> np.ndarray:
    """One ``Sim3DR_Cython.rasterize`` call with depth = -1e8 everywhere; ``image`` (contiguous uint8 [H, W, 3]) is painted in place."""
    if not use_live:
        return rasterize(image, vertices, triangles, colors, alpha, reverse)
    v, t, c = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(triangles, dtype=np.int32), np.ascontiguousarray(colors, dtype=f32)
    assert image.flags.c_contiguous and image.dtype == np.uint8
    h, w, ch = image.shape
    zb = np.zeros((h, w), dtype=f32) - 1e8  # Sim3DR.py:31
    live().ref_rasterize(image.ctypes.data, v.ctypes.data, t.ctypes.data, c.ctypes.data, zb.ctypes.data, t.shape[0], h, w, ch, float(alpha), int(bool(reverse)))
    return image


def render_mesh(image, heads_vertices, faces, use_live: bool, alpha=DEFAULTS["alpha"], color=DEFAULTS["color"], ambient=DEFAULTS["ambient"], diffuse=DEFAULTS["diffuse"],
                light=DEFAULTS["light"], colors_out: Optional[list] = None) -> np.ndarray:
    """The composition PredictionResult.render_mesh is defined as."""
    img = np.ascontiguousarray(image).copy()
    for vertices in heads_vertices:
        v = np.array(vertices, dtype=f32)
        v[:, 2] *= -1
        c = shade(normals(v, faces, use_live), color, ambient, diffuse, light)
        if colors_out is not None:
            colors_out.append(c)
        blend(img, v, faces, c, alpha, False, use_live)
    return img


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------------
def ellipsoid(n_lat: int = 51, n_lon: int = 100):
    """A closed latitude / longitude sphere: vertices [2 + (n_lat - 1) * n_lon, 3] on the unit sphere (float64) and its triangles, outward winding.  The
    default has FLAME's size: 5 002 vertices, 10 000 triangles."""
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)), np.outer(np.cos(lat), np.ones_like(lon))], axis=-1).reshape(-1, 3)
    ver = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    a, b, c, d = idx[:-1].ravel(), nxt[:-1].ravel(), idx[1:].ravel(), nxt[1:].ravel()
    south = ver.shape[0] - 1
    tri = np.concatenate([np.stack([np.zeros(n_lon, np.int64), idx[0], nxt[0]], 1), np.stack([a, c, b], 1), np.stack([b, c, d], 1),
                          np.stack([np.full(n_lon, south), nxt[-1], idx[-1]], 1)]).astype(np.int32)
    return ver, tri


def ellipsoid_heads(rng, n: int, H: int, W: int, lo: float, hi: float, unit: np.ndarray, spread: float = 1.1):
    """n bumpy, rotated ellipsoids of lo .. hi pixels whose centres may lie a little outside the image -> float32 [n, V, 3]."""
    out = []
    for _ in range(n):
        size = rng.uniform(lo, hi)
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        radii = size * 0.5 * np.array([1.0, rng.uniform(1.0, 1.3), rng.uniform(0.8, 1.1)])
        bump = 1.0 + 0.08 * np.sin(5 * unit[:, 0] + rng.uniform(0, 6)) * np.cos(4 * unit[:, 1] + rng.uniform(0, 6))
        p = (unit * bump[:, None] * radii) @ q.T
        centre = np.array([rng.uniform((1 - spread) * W, spread * W), rng.uniform((1 - spread) * H, spread * H), rng.uniform(-50, 50)])
        out.append((p + centre).astype(f32))
    return np.stack(out)


def corner_case_mesh():
    """A zero-area triangle, a vertex no triangle names (7), a triangle naming one vertex twice, next to ordinary ones."""
    ver = np.array([[0, 0, 0], [4, 0, 1], [0, 3, 2], [4, 4, -1], [2, 2, 5], [1, 1, 1], [2, 2, 2], [9, 9, 9], [3, 3, 3]], dtype=f32)
    tri = np.array([[0, 1, 2], [1, 3, 2], [5, 6, 8], [0, 4, 4], [2, 4, 3], [4, 4, 1], [3, 1, 4]], dtype=np.int32)
    return ver, tri


NORMAL_SEEDS = (1, 2, 3)
ALPHAS = (0.0, 0.25, 0.6, 1.0)
BLEND_SHAPE = (128, 128, 3)
EDGE_SHAPE = (75, 101, 3)  # not multiples of 16
EDGE_CENTRES = {"left": (4.0, 40.0), "right": (97.0, 36.0), "top": (50.0, 3.0), "bottom": (52.0, 72.0)}


def background(seed: int, shape) -> np.ndarray:
    return np.random.default_rng(1000 + seed).integers(0, 256, shape, dtype=np.uint8)


def edge_mesh(side: str):
    return ro.random_mesh(40 + list(EDGE_CENTRES).index(side), n_side=10, size=60.0, centre=EDGE_CENTRES[side], depth_scale=30.0)


SCENE_SHAPES = {"A": (150, 190, 3), "B": (131, 167, 3)}


def scene(letter: str):
    """Image, 8 overlapping heads (float32 [8, 802, 3]) and the triangles of one of the two render_mesh scenes."""
    shape = SCENE_SHAPES[letter]
    unit, tri = ellipsoid(21, 40)
    rng = np.random.default_rng({"A": 71, "B": 72}[letter])
    heads = ellipsoid_heads(rng, 8, shape[0], shape[1], 30.0, 60.0, unit, spread=0.8)
    return background({"A": 5, "B": 6}[letter], shape), heads, tri


def make_head(vertices):
    return types.SimpleNamespace(vertices_3d=np.array(vertices, dtype=f32))
