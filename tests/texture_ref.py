"""TEST INFRASTRUCTURE.  Head textures on the CPU: a restatement of

  render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth, mapping)
                                   Sim3DR ``_render_texture_core`` (head_detector/Sim3DR/lib/rasterize_kernel.cpp:358-463), painting image and depth in place

and the compositions ``head_detector_amd.texture`` is defined as: ``compose`` (one call per head, in head order, into one image in painter's order or
through one shared z-buffer, or into one image per head), ``unwrap`` (the photograph as the texture, the heads' own vertices as texture coordinates),
``get_textures`` and ``paint`` (what the two ``PredictionResult`` methods return).  Where oracle/_ref/libsim3dr_ref.so exists (oracle/build_ref.py),
``live()`` binds the reference's own C++ through its mangled name and ``use_live=True`` runs it instead: PINNED, tests/golden/texture.npz holds that
library's outputs and tests/test_texture_host.py holds the restatement to them.  The C++ returns no triangle index; with ``use_live`` the triangles are fed
to it one at a time and a pixel's triangle is the last one that changed its depth (a win writes a strictly greater depth).  All arithmetic is float32 in
the reference's operation order.

Also the inputs the fixture and the tests share (generated from seeds, never stored) and the fixture's encoding, which stores written pixels only."""
from __future__ import annotations

import ctypes
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import visibility_ref as vr  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "texture.npz")
BACKGROUND = f32(-1e8)
MAPPINGS = {"nearest": 0, "bilinear": 1}
SYMBOL = "_Z20_render_texture_corePfS_PiS_S_S0_S_iiiiiiiiii"


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def _clamp_like_std(a, hi):
    """max(min(a, hi), 0) with std::min / std::max as the source calls them: min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a."""
    a = np.where(f32(hi) < a, f32(hi), a).astype(f32)
    return np.where(a < 0, f32(0.0), a).astype(f32)


def _index(a, last):
    return np.clip(np.nan_to_num(a, nan=0.0, posinf=last, neginf=0.0), 0, last).astype(np.int64)


def _mix(q0, q1, q2, w0, w1, w2):
    """(q0 * w0 + q1 * w1) + q2 * w2 in float32."""
    return (((q0 * w0).astype(f32) + (q1 * w1).astype(f32)).astype(f32) + (q2 * w2).astype(f32)).astype(f32)


def render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth, mapping, tri_out=None, frame: bool = True, quirk: bool = True,
                        stats: dict = None) -> None:
    """``_render_texture_core`` on the caller's buffers (float32 [H, W, c] and [H, W]), in place; ``texture`` float32 [th, tw, tc >= c], ``mapping`` 0 = nearest,
    else bilinear.  A triangle with a non-finite x or y is skipped.  ``tri_out`` (int32 [H, W]) receives the index of every winning triangle.
    NOT the reference, kept to show that the inputs bite: ``frame=False`` drops the rule that in a frame two pixels wide every pixel of a triangle's box is
    inside, ``quirk=False`` reads a corner's texture y through ``tex_triangles`` like its x.  ``stats`` counts, per painted (pixel, triangle): "clamped"
    texture positions, nearest lookups at exactly "half", bilinear lookups at "integer" positions, pixels of "zero_det" triangles."""
    h, w, c = image.shape
    th, tw, tc = texture.shape
    assert tc >= c and texture.dtype == f32 and image.dtype == f32 and depth.dtype == f32
    ver, q = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(tex_coords, dtype=f32)
    tri, ttri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3), np.ascontiguousarray(tex_triangles, dtype=np.int32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for t in range(tri.shape[0]):
            i0, i1, i2 = (int(k) for k in tri[t])
            j0, j1, j2 = (int(k) for k in ttri[t])
            p0, p1, p2 = ver[i0], ver[i1], ver[i2]
            xs, ys = (p0[0], p1[0], p2[0]), (p0[1], p1[1], p2[1])
            if not all(math.isfinite(float(k)) for k in xs + ys):
                continue
            x_min, x_max = max(int(math.ceil(min(xs))), 0), min(int(math.floor(max(xs))), w - 1)
            y_min, y_max = max(int(math.ceil(min(ys))), 0), min(int(math.floor(max(ys))), h - 1)
            if x_max < x_min or y_max < y_min:
                continue
            py, px = np.meshgrid(np.arange(y_min, y_max + 1, dtype=f32), np.arange(x_min, x_max + 1, dtype=f32), indexing="ij")
            w0, w1, w2 = ro._weights(px, py, p0, p1, p2)  # (1 - u - v, v, u); a zero determinant gives u = v = 0
            inside = (w2 >= 0) & (w1 >= 0) & ((w2 + w1).astype(f32) < 1)
            if frame:
                inside = inside | (px < 2) | (px > w - 3) | (py < 2) | (py > h - 3)
            pd = _mix(p0[2], p1[2], p2[2], w0, w1, w2)
            sub = depth[y_min : y_max + 1, x_min : x_max + 1]
            win = inside & (pd > sub)  # false for NaN
            if not win.any():
                continue
            y0, y1, y2 = (i0, i1, i2) if quirk else (j0, j1, j2)  # the source reads a corner's texture y through the MESH's index
            w0, w1, w2 = w0[win], w1[win], w2[win]
            raw_x, raw_y = _mix(q[j0, 0], q[j1, 0], q[j2, 0], w0, w1, w2), _mix(q[y0, 1], q[y1, 1], q[y2, 1], w0, w1, w2)
            qx, qy = _clamp_like_std(raw_x, tw - 1), _clamp_like_std(raw_y, th - 1)
            fx, fy = np.floor(qx).astype(f32), np.floor(qy).astype(f32)
            xd, yd = (qx - fx).astype(f32), (qy - fy).astype(f32)
            if mapping == 0:  # int(round(.)): halves away from zero; the positions are >= 0 here and q - floor(q) is exact
                col = texture[_index(fy + (yd >= 0.5), th - 1), _index(fx + (xd >= 0.5), tw - 1), :c]
            else:
                xf, xc, yf, yc = _index(fx, tw - 1), _index(np.ceil(qx), tw - 1), _index(fy, th - 1), _index(np.ceil(qy), th - 1)
                ax, ay = (f32(1.0) - xd).astype(f32)[:, None], (f32(1.0) - yd).astype(f32)[:, None]
                bx, by = xd[:, None], yd[:, None]
                ul, ur, dl, dr = texture[yf, xf, :c], texture[yf, xc, :c], texture[yc, xf, :c], texture[yc, xc, :c]
                col = ((ul * ax).astype(f32) * ay).astype(f32)
                col = (col + ((ur * bx).astype(f32) * ay).astype(f32)).astype(f32)
                col = (col + ((dl * ax).astype(f32) * by).astype(f32)).astype(f32)
                col = (col + ((dr * bx).astype(f32) * by).astype(f32)).astype(f32)
            image[y_min : y_max + 1, x_min : x_max + 1][win] = col
            sub[win] = pd[win]
            if tri_out is not None:
                tri_out[y_min : y_max + 1, x_min : x_max + 1][win] = t
            if stats is not None:
                stats["clamped"] = stats.get("clamped", 0) + int(((raw_x != qx) | (raw_y != qy)).sum())
                stats["half"] = stats.get("half", 0) + (int(((xd == 0.5) | (yd == 0.5)).sum()) if mapping == 0 else 0)
                stats["integer"] = stats.get("integer", 0) + (int(((xd == 0) & (yd == 0)).sum()) if mapping != 0 else 0)
                v0, v1 = p2[:2] - p0[:2], p1[:2] - p0[:2]
                d00, d01, d11 = f32(v0[0] * v0[0]) + f32(v0[1] * v0[1]), f32(v0[0] * v1[0]) + f32(v0[1] * v1[1]), f32(v1[0] * v1[0]) + f32(v1[1] * v1[1])
                stats["zero_det"] = stats.get("zero_det", 0) + (int(win.sum()) if f32(d00 * d11) - f32(d01 * d01) == 0 else 0)


# ---- the reference's own C++ -------------------------------------------------------------------------------------------------------------------
_live = [False, None]


def live():
    """``_render_texture_core`` of oracle/_ref/libsim3dr_ref.so, taken by its mangled name, or None where the library cannot be had."""
    if not _live[0]:
        from oracle import build_ref

        fn = None
        path = build_ref.build()
        if path is not None:
            P, I = ctypes.c_void_p, ctypes.c_int
            fn = getattr(ctypes.CDLL(path), SYMBOL)
            fn.argtypes, fn.restype = [P] * 7 + [I] * 10, None
        _live[:] = [True, fn]
    return _live[1]


def one_call(image, vertices, triangles, texture, tex_coords, tex_triangles, depth, mapping, use_live: bool, tri_out=None, **rule) -> None:
    """One ``_render_texture_core`` call on the caller's contiguous buffers."""
    if not use_live:
        return render_texture_core(image, vertices, triangles, texture, tex_coords, tex_triangles, depth, mapping, tri_out, **rule)
    assert not rule
    v, q, tex = np.ascontiguousarray(vertices, dtype=f32), np.ascontiguousarray(tex_coords, dtype=f32), np.ascontiguousarray(texture, dtype=f32)
    t, tt = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3), np.ascontiguousarray(tex_triangles, dtype=np.int32).reshape(-1, 3)
    for a in (image, depth):
        assert a.flags.c_contiguous and a.dtype == f32
    (h, w, c), (th, tw, tc) = image.shape, tex.shape
    finite = np.isfinite(v[t.reshape(-1), :2]).reshape(-1, 6).all(axis=1) if t.size else np.zeros(0, bool)  # the contract skips what is undefined in C

    def call(first, count):
        live()(image.ctypes.data, v.ctypes.data, t.ctypes.data + 12 * first, tex.ctypes.data, q.ctypes.data, tt.ctypes.data + 12 * first, depth.ctypes.data, v.shape[0],
               q.shape[0], count, h, w, c, th, tw, tc, int(mapping))

    if tri_out is None and finite.all():
        return call(0, t.shape[0])
    for k in range(t.shape[0]):  # one triangle at a time: the pixels whose depth changes are the ones it wins
        if not finite[k]:
            continue
        before = depth.copy() if tri_out is not None else None
        call(k, 1)
        if tri_out is not None:
            tri_out[depth != before] = k


def _per_head(a, n, ndim):
    a = np.asarray(a)
    return [a] * n if a.ndim == ndim else [a[i] for i in range(n)]


def compose(heads_vertices, triangles, textures, tex_coords, H: int, W: int, c: int, mapping: str, occlusion: str = "order", z_sign: float = 1.0, tex_triangles=None,
            image=None, per_head_dst: bool = False, use_live: bool = False, **rule) -> dict:
    """The composition ``texture.render_texture`` is defined as -> dict(image, depth, triangle, head).  ``textures`` [th, tw, tc] or [n, th, tw, tc], uint8 or
    float32 (a uint8 texel is converted exactly); ``tex_coords`` [Vt, 3] or [n, Vt, 3].  ``per_head_dst``: head i paints slice i of [n, H, W, ...]."""
    assert occlusion in ("order", "depth")
    heads = np.asarray(heads_vertices, dtype=f32)
    heads = heads[None] if heads.ndim == 2 else heads
    n = heads.shape[0]
    tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    ttri = tri if tex_triangles is None else np.ascontiguousarray(tex_triangles, dtype=np.int32).reshape(-1, 3)
    texs = [np.ascontiguousarray(t).astype(f32) for t in _per_head(textures, n, 3)]
    qs = _per_head(np.asarray(tex_coords, dtype=f32), n, 2)
    lead = (n,) if per_head_dst else ()
    out = dict(image=np.zeros(lead + (H, W, c), f32) if image is None else np.ascontiguousarray(image, dtype=f32).copy(), depth=np.full(lead + (H, W), BACKGROUND, f32),
               triangle=np.full(lead + (H, W), -1, np.int32), head=np.full(lead + (H, W), -1, np.int32))
    assert out["image"].shape == lead + (H, W, c)
    m_id = MAPPINGS[mapping]
    for i in range(n):
        v = np.array(heads[i], dtype=f32)  # a copy: the head's own array is not modified
        v[:, 2] *= f32(z_sign)
        s_tri = np.full((H, W), -1, np.int32)
        if per_head_dst:
            one_call(out["image"][i], v, tri, texs[i], qs[i], ttri, out["depth"][i], m_id, use_live, s_tri, **rule)
            out["triangle"][i] = s_tri
            out["head"][i][s_tri >= 0] = i
            continue
        depth = out["depth"] if occlusion == "depth" else np.full((H, W), BACKGROUND, f32)
        one_call(out["image"], v, tri, texs[i], qs[i], ttri, depth, m_id, use_live, s_tri, **rule)
        m = s_tri >= 0
        out["triangle"][m], out["head"][m], out["depth"][m] = s_tri[m], i, depth[m]
    return out


def atlas_vertices(uv, th: int, tw: int) -> np.ndarray:
    uv = np.asarray(uv).astype(f32)
    out = np.zeros((uv.shape[0], 3), f32)
    out[:, 0], out[:, 1] = uv[:, 0] * f32(tw - 1), uv[:, 1] * f32(th - 1)
    return out


def unwrap(image, heads_vertices, triangles, uv, th: int, tw: int, mapping: str, use_live: bool = False, **rule) -> dict:
    """``texture.unwrap_heads``: the atlas as the image, the vertices' UV positions as the mesh, the photograph as the texture, the heads' vertices as texture
    coordinates -> dict(image [n, th, tw, C], depth, triangle, head)."""
    heads = np.asarray(heads_vertices, dtype=f32)
    heads = heads[None] if heads.ndim == 2 else heads
    atlas = atlas_vertices(uv, th, tw)
    return compose(np.repeat(atlas[None], heads.shape[0], axis=0), triangles, image, heads, th, tw, np.shape(image)[2], mapping, tex_triangles=triangles, per_head_dst=True,
                   use_live=use_live, **rule)


def get_textures(image, heads_vertices, faces, uv, th: int, tw: int, mapping: str = "bilinear", visible_only: bool = True, occlusion: str = "order",
                 use_live: bool = False) -> dict:
    """What ``PredictionResult.get_textures`` returns -> dict(texture, triangle, written, mask)."""
    heads = np.asarray(heads_vertices, dtype=f32)
    res = unwrap(image, heads, faces, uv, th, tw, mapping, use_live)
    written = res["triangle"] >= 0
    mask = written.copy()
    if visible_only:
        H, W = np.shape(image)[:2]
        vis = vr.compose(heads, faces, H, W, occlusion, -1.0, use_live and vr.live() is not None)
        for i in range(heads.shape[0]):
            seen = np.unique(vis["triangle_index"][vis["head_index"] == i])
            mask[i] &= np.isin(res["triangle"][i], seen)
    return dict(texture=res["image"], triangle=res["triangle"], written=written, mask=mask)


def paint(image, heads_vertices, faces, textures, uv, mapping: str = "bilinear", occlusion: str = "order", use_live: bool = False) -> np.ndarray:
    """What ``PredictionResult.render_texture`` returns: uint8 [H, W, 3]."""
    H, W = np.shape(image)[:2]
    th, tw = np.shape(textures)[-3:-1]
    res = compose(heads_vertices, faces, textures, atlas_vertices(uv, th, tw), H, W, 3, mapping, occlusion, -1.0, image=np.asarray(image).astype(f32), use_live=use_live)
    return np.clip(res["image"], f32(0.0), f32(255.0)).astype(np.uint8)  # truncation: the values are >= 0


FIELDS = ("image", "depth", "triangle", "head")


def same(got: dict, want: dict, what, fields=FIELDS) -> None:
    """Exact equality (no tolerance)."""
    for key in fields:
        a, b = got[key], want[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b), (what, key, int((a != b).sum()), "values differ")


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------------------
SHAPE_A, SHAPE_B = (61, 83), (37, 40)  # (H, W): no multiples of the 16-pixel tile, more than one tile
ATLAS_A, ATLAS_B = (48, 48), (29, 33)  # (th, tw)


def patch_mesh(n_side: int = 13):
    """A half-sphere "head" over a square patch: unit vertices [n_side^2, 3] (x, y in [-1, 1], z the dome), 2 (n_side - 1)^2 triangles, uv [n_side^2, 2]."""
    g = np.linspace(-1.0, 1.0, n_side)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    zz = np.sqrt(np.maximum(2.0 - xx * xx - yy * yy, 0.0)) - 0.4
    unit = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    uv = np.stack([(xx + 1) / 2, 0.12 + 0.39 * (yy + 1)], axis=-1).reshape(-1, 2).astype(f32)  # the whole width, rows 0.12 .. 0.90 of the atlas
    return unit, tri, uv


def heads(seed: int, n: int, H: int, W: int) -> np.ndarray:
    """n tilted copies of the patch in image coordinates, float32 [n, 169, 3]: the first four hang over the left, right, top and bottom border (a single head
    over the top left corner), the others lie between them; they overlap and hide one another."""
    rng = np.random.default_rng(seed)
    unit = patch_mesh()[0]
    border = [(1.0, H * 0.45), (W - 2.0, H * 0.55), (W * 0.45, 1.0), (W * 0.55, H - 2.0)]
    out = []
    for i in range(n):
        size = rng.uniform(0.2, 0.32) * min(H, W)
        ax, ay, az = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(-np.pi, np.pi)
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        centre = (4.0, 5.0) if n == 1 else border[i] if i < 4 else (rng.uniform(0.25, 0.75) * W, rng.uniform(0.25, 0.75) * H)
        p = (unit * size) @ (rz @ ry @ rx).T + np.array([centre[0], centre[1], rng.uniform(-10, 10)])
        out.append(p.astype(f32))
    return np.stack(out) if n else np.zeros((0, unit.shape[0], 3), f32)


def random_texture(seed: int, shape, dtype):
    rng = np.random.default_rng(2000 + seed)
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.uniform(-3.0, 260.0, shape).astype(f32)


def wrap_coords(seed: int, n, uv, th: int, tw: int) -> np.ndarray:
    """Texture coordinates [Vt, 3] (n = None) or [n, Vt, 3] that overshoot the texture a little on every side (clamped positions); the third column is junk
    that must never be read."""
    rng = np.random.default_rng(3000 + seed)
    k = 1 if n is None else n
    out = np.zeros((k, uv.shape[0], 3), f32)
    for i in range(k):
        s, dx, dy = rng.uniform(1.0, 1.1), rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0)
        out[i, :, 0] = ((uv[:, 0] - 0.5) * s + 0.5) * (tw - 1) + dx
        out[i, :, 1] = ((uv[:, 1] - 0.5) * s + 0.5) * (th - 1) + dy
        out[i, :, 2] = rng.uniform(-1e6, 1e6, uv.shape[0])
    return out[0] if n is None else out


def permuted_topology(seed: int, tri, coords):
    """A texture topology of its own: vertex i of the mesh is texture vertex perm[i] -> (tex_triangles = perm[tri], the coordinates reordered to match).  Read
    properly (x and y through tex_triangles) this is the same picture as before; the source reads y through ``tri``."""
    perm = np.random.default_rng(4000 + seed).permutation(coords.shape[-2])
    out = np.empty_like(coords)
    out[..., perm, :] = coords
    return perm[tri].astype(np.int32), out


def photograph(seed: int, H: int, W: int, C: int, dtype, noise: float = 4.0, smooth: float = 1.0):
    """A smooth picture with a little noise."""
    rng = np.random.default_rng(5000 + seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([127 + 100 * np.sin(xx / (smooth * (7.0 + k)) + k) * np.cos(yy / (smooth * (9.0 - k))) for k in range(C)], axis=-1) + rng.normal(0, noise, (H, W, C))
    return np.clip(img, 0, 255).astype(np.uint8) if dtype == np.uint8 else img.astype(f32)


def quad_case(scale: float):
    """Two triangles on integer pixel positions (an 8 x 8 square whose determinant is a power of two, so every weight is exact) with texture coordinates =
    ``scale`` x the position inside the square: 0.5 puts every other pixel at exactly .5, 1.0 puts every pixel at integer coordinates."""
    ver = np.array([[3, 4, 1], [11, 4, 2], [3, 12, 3], [11, 12, 4]], f32)
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    coords = np.zeros((4, 3), f32)
    coords[:, :2] = (ver[:, :2] - f32([3, 4])) * f32(scale) + f32(1.0)
    return ver, tri, coords


def corner_case():
    """shade_ref.corner_case_mesh scaled by 3 and moved off the frame: its triangle 5 ([4, 4, 1]) has a zero determinant and holds a block of pixels."""
    ver, tri = sr.corner_case_mesh()
    ver = (ver * f32(3) + f32([4, 3, 0])).astype(f32)
    coords = np.zeros((ver.shape[0], 3), f32)
    coords[:, 0], coords[:, 1] = ver[:, 1] * f32(0.7), ver[:, 0] * f32(0.9)
    return ver, tri, coords


def cases():
    """name -> keyword arguments of ``compose``: every wrap case of the fixture.  Together: both image sizes, both atlases, 1, 5 and 12 heads, c = 1, 3, 4 with
    tex_c > c, u8 and f32 textures, shared and per-head textures and coordinates, both mappings, both modes, a texture topology of its own, a background."""
    _, tri, uv = patch_mesh()
    out = {}
    (H, W), (th, tw) = SHAPE_A, ATLAS_B
    a = dict(heads_vertices=heads(11, 12, H, W), triangles=tri, textures=random_texture(1, (12, th, tw, 4), f32), tex_coords=wrap_coords(1, None, uv, th, tw), H=H, W=W, c=3,
             mapping="bilinear", z_sign=-1.0)
    out["A_order"], out["A_depth"] = dict(a, occlusion="order"), dict(a, occlusion="depth")
    (H, W), (th, tw) = SHAPE_B, ATLAS_A
    ttri, coords = permuted_topology(2, tri, wrap_coords(2, 5, uv, th, tw))
    b = dict(heads_vertices=heads(15, 5, H, W), triangles=tri, textures=random_texture(2, (th, tw, 3), np.uint8), tex_coords=coords, tex_triangles=ttri, H=H, W=W, c=1,
             mapping="nearest", z_sign=1.0)
    out["B_order"], out["B_depth"] = dict(b, occlusion="order"), dict(b, occlusion="depth")
    out["C"] = dict(heads_vertices=heads(13, 1, H, W), triangles=tri, textures=random_texture(3, (1, th, tw, 5), np.uint8), tex_coords=wrap_coords(3, 1, uv, th, tw), H=H, W=W,
                    c=4, mapping="bilinear", occlusion="depth", image=random_texture(4, (H, W, 4), f32))
    for name, scale, mapping in (("quad_half", 0.5, "nearest"), ("quad_integer", 1.0, "bilinear")):
        ver, qtri, qc = quad_case(scale)
        out[name] = dict(heads_vertices=ver, triangles=qtri, textures=random_texture(5, (9, 10, 3), f32), tex_coords=qc, H=16, W=16, c=3, mapping=mapping)
    ver, ctri, cc = corner_case()
    out["corner"] = dict(heads_vertices=ver, triangles=ctri, textures=random_texture(6, (12, 14, 1), f32), tex_coords=cc, H=20, W=24, c=1, mapping="bilinear")
    return out


BASES = {"A_depth": "A_order", "B_depth": "B_order"}  # stored as the difference to the other mode


def unwrap_cases():
    """name -> keyword arguments of ``unwrap``."""
    _, tri, uv = patch_mesh()
    (H, W) = SHAPE_A
    return {"unwrap_A": dict(image=photograph(1, H, W, 3, np.uint8), heads_vertices=heads(21, 5, H, W), triangles=tri, uv=uv, th=ATLAS_B[0], tw=ATLAS_B[1], mapping="bilinear"),
            "unwrap_B": dict(image=photograph(2, SHAPE_B[0], SHAPE_B[1], 1, f32), heads_vertices=heads(22, 2, *SHAPE_B), triangles=tri, uv=uv, th=ATLAS_A[0], tw=ATLAS_A[1],
                             mapping="nearest")}


def roundtrip_scene():
    """The photograph, one head in the middle of it and the atlas size of the unwrap-then-wrap case."""
    H, W = 80, 96
    unit, tri, uv = patch_mesh()
    ver = (unit * np.array([30.0, 30.0, 30.0]) + np.array([48.0, 40.0, 0.0])).astype(f32)
    return photograph(3, H, W, 3, np.uint8, noise=0.0, smooth=3.0), ver, tri, uv, ATLAS_A


def roundtrip(use_live: bool = False) -> dict:
    """Unwrap the photograph into the atlas, then paint the atlas back onto a black image (depth = z)."""
    img, ver, tri, uv, (th, tw) = roundtrip_scene()
    tex = unwrap(img, ver, tri, uv, th, tw, "bilinear", use_live)
    back = compose(ver, tri, tex["image"][0], atlas_vertices(uv, th, tw), img.shape[0], img.shape[1], 3, "bilinear", use_live=use_live)
    back["texels"] = int((tex["triangle"] >= 0).sum())
    return back


def result_scene():
    """The planted heads of the ``PredictionResult`` tests: unwrap_A's photograph and heads (they hide one another in part)."""
    k = unwrap_cases()["unwrap_A"]
    return k["image"], k["heads_vertices"], k["triangles"], k["uv"], (k["th"], k["tw"])


# ---- the fixture's encoding: written pixels only ------------------------------------------------------------------------------------------------
# Colour and depth are functions of (head, triangle, pixel): a case stores them for written pixels only, and a case with a base (the other mode of the
# same scene) only where (head, triangle) differs from the base.
def encode(res: dict, base: dict = None) -> dict:
    own = res["triangle"] >= 0
    keep = own if base is None else own & ((res["head"] != base["head"]) | (res["triangle"] != base["triangle"]))
    enc = dict(head=res["head"].astype(np.int16), tri=res["triangle"].astype(np.int16), depth=res["depth"][keep], colour=res["image"][keep])
    assert np.array_equal(enc["head"], res["head"]) and np.array_equal(enc["tri"], res["triangle"])
    return enc


def decode(enc: dict, background=None, base: dict = None) -> dict:
    """``background``: what the image held before (default zeros)."""
    head, tri = enc["head"].astype(np.int32), enc["tri"].astype(np.int32)
    own = tri >= 0
    keep = own if base is None else own & ((head != base["head"]) | (tri != base["triangle"]))
    c = enc["colour"].shape[-1]
    image = np.zeros(head.shape + (c,), f32) if background is None else np.array(background, dtype=f32)
    depth = np.full(head.shape, BACKGROUND, f32)
    if base is not None:
        share = own & ~keep
        depth[share], image[share] = base["depth"][share], base["image"][share]
    depth[keep], image[keep] = enc["depth"], enc["colour"]
    return dict(image=image, depth=depth, triangle=tri, head=head)


def golden_case(g, name: str, background=None, base: dict = None) -> dict:
    return decode({k: g[f"{name}.{k}"] for k in ("head", "tri", "depth", "colour")}, background, base)
