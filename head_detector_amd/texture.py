"""Head textures: Sim3DR's ``render_texture`` for all heads of an image on the GPU (csrc/texture.hip, libvghtex.so), in both directions.

  render_texture(vertices, triangles, texture, tex_coords, height, width, ...)   -> float32 [H, W, c]     the reference function, one mesh or many
  unwrap_heads(image, vertices, triangles, uv, size=256, ...)                     -> HeadTextures          photograph -> one UV atlas per head
  cylindrical_uv(template_vertices, triangles)                                    -> (uv, keep)            a UV layout from the template alone (host)

defined as these compositions of reference calls (``rt`` = ``_render_texture_core`` of head_detector/Sim3DR/lib/rasterize_kernel.cpp, depth = ``z_sign * z``
on a copy of the vertices):

  render_texture   for i in order: rt(image, v_i, triangles, texture_i, tex_coords_i, tex_triangles, depth, mapping) on the SAME image;
                   occlusion="order": ``depth`` is fresh (-1e8) for every head, so a later head paints over an earlier one (the rule of
                   PNCCProcessor.__call__ and of render_mesh); occlusion="depth": one depth buffer for all heads
  unwrap_heads     ``rt`` reads ``tex_coords`` with stride 3, so a head's own ``vertices_3d`` (image x, y, z) serve as texture coordinates:
                   for every head i: rt(atlas_i = 0, atlas_vertices, triangles, texture = image, tex_coords = v_i, tex_triangles = triangles, fresh depth),
                   atlas_vertices = (u * (tw - 1), v * (th - 1), 0) in float32, no flip

The source's quirks are kept (include/vgh_tex.h states the per-pixel rule): a corner's texture y is read through the MESH's triangle list even where
``tex_triangles`` differs, and in a frame two pixels wide every pixel of a triangle's bounding box counts as inside.  Every output is bit-identical to the
reference's C++ (tests/test_gpu_texture.py).  There is no CPU path."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib_tex
from .mesh_geometry import check_raster_arguments, check_triangles, device_of, head_vertices, pixel_bounds, require_faces, shape_of, to_device


class HeadTextures:
    """What ``unwrap_heads`` / ``PredictionResult.get_textures`` return.  NumPy arrays (``to_host=True``) or GPU tensors: ``texture`` float32 [n, th, tw, C]
    (0 where nothing was written), ``triangle`` int32 [n, th, tw] (the triangle a texel shows, -1 = none), ``written`` bool [n, th, tw], ``mask`` bool
    [n, th, tw]: ``written``, and for ``get_textures(visible_only=True)`` also seen in the photograph."""

    def __init__(self, texture, triangle, written, mask=None):
        self.texture = texture
        self.triangle = triangle
        self.written = written
        self.mask = written if mask is None else mask

    def __len__(self):
        return int(self.texture.shape[0])

    def __repr__(self):
        return f"HeadTextures(heads={len(self)}, size={tuple(self.texture.shape[1:3])}, channels={int(self.texture.shape[3])})"


def _device_of(*candidates):
    return device_of(*candidates, what="render_texture", lib="libvghtex.so")


def _texture_dtype(texture) -> torch.dtype:
    """uint8 stays uint8 (the kernel converts a texel exactly); everything else is looked up as float32."""
    is_u8 = texture.dtype == (torch.uint8 if isinstance(texture, torch.Tensor) else np.uint8)
    return torch.uint8 if is_u8 else torch.float32


def check_arguments(v_shape, height, width, mapping, occlusion, z_sign):
    """Validates what needs no GPU -> (n, V, height, width, mapping, mode, z_sign); ``v_shape`` is the vertices' shape."""
    if mapping not in _lib_tex.MAPPINGS:
        raise ValueError(f"mapping must be 'bilinear' or 'nearest', got {mapping!r}")
    n, V, height, width, mode, z_sign = check_raster_arguments(v_shape, height, width, occlusion, z_sign, _lib_tex)
    return n, V, height, width, _lib_tex.MAPPINGS[mapping], mode, z_sign


def _check_texture(t_shape, n, what="texture"):
    t_shape = tuple(t_shape)
    if len(t_shape) not in (3, 4) or min(t_shape[-3:]) < 1:
        raise ValueError(f"{what} must be [th, tw, C] or [n, th, tw, C] with no empty side, got {t_shape}")
    if len(t_shape) == 4 and t_shape[0] != n:
        raise ValueError(f"{what} holds {t_shape[0]} textures for {n} heads")
    if max(t_shape[-3:-1]) > _lib_tex.MAX_SIDE:
        raise ValueError(f"{what}: sides must lie in 1 .. {_lib_tex.MAX_SIDE}, got {t_shape[-3]} x {t_shape[-2]}")
    return len(t_shape) == 4


def _launch(v, tri, tex_tri, coords, coords_per_head, texture, tex_per_head, dst, depth, tri_buf, head_buf, dst_per_head, mapping, mode, z_sign):
    """One vghtex_render_texture call on device tensors that are already shaped and typed: v [n, V, 3], coords [n or 1, Vt, 3], texture [n or 1, th, tw, tc],
    dst [(n,) H, W, c]."""
    n, V = int(v.shape[0]), int(v.shape[1])
    H, W, c = (int(s) for s in dst.shape[-3:])
    bounds = pixel_bounds(v, tri, H, W)  # one amin / amax on the device, 4 n floats to the host
    job = _lib_tex.Job()
    job.height, job.width, job.channels, job.n_heads, job.n_vertices, job.n_triangles = H, W, c, n, V, tri.shape[0]
    job.n_tex_vertices, job.tex_height, job.tex_width, job.tex_channels = int(coords.shape[1]), int(texture.shape[1]), int(texture.shape[2]), int(texture.shape[3])
    job.tex_dtype = _lib_tex.TEX_DTYPES["uint8" if texture.dtype == torch.uint8 else "float32"]
    job.tex_per_head, job.tex_coords_per_head, job.dst_per_head = int(tex_per_head), int(coords_per_head), int(dst_per_head)
    job.mapping, job.mode, job.z_sign = mapping, mode, z_sign
    job.dst_dev, job.depth_dev = dst.data_ptr() or None, depth.data_ptr() or None
    job.triangle_dev = None if tri_buf is None else (tri_buf.data_ptr() or None)
    job.head_dev = None if head_buf is None else (head_buf.data_ptr() or None)
    if n and tri.shape[0]:
        job.verts_dev, job.triangles, job.bounds = v.data_ptr(), tri.ctypes.data, bounds.ctypes.data
        job.tex_coords_dev, job.tex_triangles, job.texture_dev = coords.data_ptr(), tex_tri.ctypes.data, texture.data_ptr()
    with torch.cuda.device(v.device):
        _lib_tex.check(_lib_tex.load().vghtex_render_texture(job, torch.cuda.current_stream().cuda_stream))


def render_texture(vertices, triangles, texture, tex_coords, height, width, *, tex_triangles=None, image=None, channels=None, mapping: str = "bilinear",
                   occlusion: str = "order", z_sign: float = 1.0, to_host: bool = True, with_buffers: bool = False):
    """Sim3DR's ``render_texture`` for one mesh ([V, 3]) or many ([n, V, 3]) -> float32 [H, W, c].

    ``texture`` [th, tw, tc] (shared) or [n, th, tw, tc], uint8 or float; ``tex_coords`` [Vt, 3] (shared) or [n, Vt, 3] in texel units (x, y, unused);
    ``tex_triangles`` [T, 3] (default: ``triangles``).  ``image``: a float32 [H, W, c] background (default zeros), copied.  ``channels`` (default: the
    image's, else the texture's) may be below the texture's.  NumPy or GPU tensors; float64 and int64 inputs are converted, nothing is modified.
    ``with_buffers`` returns (image, depth float32 [H, W], triangle int32 [H, W], head int32 [H, W]) instead: what the z-buffer ends with (-1e8 where
    nothing was painted) and the triangle and head every painted pixel shows (-1).  Arguments are validated before a GPU is looked for."""
    n, V, H, W, mapping_id, mode, z_sign = check_arguments(shape_of(vertices), height, width, mapping, occlusion, z_sign)
    tex_per_head = _check_texture(shape_of(texture), n)
    c_shape = shape_of(tex_coords)
    if len(c_shape) not in (2, 3) or c_shape[-1] != 3:
        raise ValueError(f"tex_coords must be [Vt, 3] or [n, Vt, 3], got {c_shape}")
    if len(c_shape) == 3 and c_shape[0] != n:
        raise ValueError(f"tex_coords holds {c_shape[0]} sets for {n} heads")
    Vt = c_shape[-2]
    tri = check_triangles(triangles, min(V, Vt), "render_texture")  # a corner's texture y is read through the mesh's index
    tex_tri = tri if tex_triangles is None else check_triangles(tex_triangles, Vt, "render_texture: tex_triangles")
    if tex_tri.shape != tri.shape:
        raise ValueError(f"tex_triangles must have the shape of triangles {tri.shape}, got {tex_tri.shape}")
    tc = shape_of(texture)[-1]
    if image is not None:
        i_shape = shape_of(image)
        if len(i_shape) != 3 or i_shape[:2] != (H, W):
            raise ValueError(f"image must be [{H}, {W}, c], got {i_shape}")
        if channels is not None and int(channels) != i_shape[2]:
            raise ValueError(f"channels = {channels} with an image of {i_shape[2]} channels")
        channels = i_shape[2]
    c = tc if channels is None else int(channels)
    if not 1 <= c <= min(tc, _lib_tex.MAX_CHANNELS):
        raise ValueError(f"channels must lie in 1 .. {min(tc, _lib_tex.MAX_CHANNELS)} (the texture has {tc}), got {c}")
    dev = _device_of(vertices, texture, tex_coords, image)
    v = to_device(vertices, dev, torch.float32).reshape(n, V, 3)
    coords = to_device(tex_coords, dev, torch.float32).reshape(-1, Vt, 3)
    tex = to_device(texture, dev, _texture_dtype(texture))
    tex = tex.reshape((-1,) + tuple(tex.shape[-3:]))
    dst = torch.zeros((H, W, c), dtype=torch.float32, device=dev) if image is None else to_device(image, dev, torch.float32).clone()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    tri_buf = torch.empty((H, W), dtype=torch.int32, device=dev) if with_buffers else None
    head_buf = torch.empty((H, W), dtype=torch.int32, device=dev) if with_buffers else None
    _launch(v, tri, tex_tri, coords, len(c_shape) == 3, tex, tex_per_head, dst, depth, tri_buf, head_buf, False, mapping_id, mode, z_sign)
    out = (dst, depth, tri_buf, head_buf) if with_buffers else (dst,)
    if to_host:
        out = tuple(t.cpu().numpy() for t in out)
    return out if with_buffers else out[0]


def _atlas_size(size):
    th, tw = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
    if not (1 <= th <= _lib_tex.MAX_SIDE and 1 <= tw <= _lib_tex.MAX_SIDE):
        raise ValueError(f"size must lie in 1 .. {_lib_tex.MAX_SIDE}, got {th} x {tw}")
    return th, tw


def atlas_vertices(uv, V: int, th: int, tw: int) -> np.ndarray:
    """float32 [V, 3]: the atlas position of every vertex, (u * (tw - 1), v * (th - 1), 0) in float32, no flip."""
    uv = np.asarray(uv.detach().cpu() if isinstance(uv, torch.Tensor) else uv)
    if uv.shape != (V, 2):
        raise ValueError(f"uv must be [{V}, 2] (one position per vertex), got {uv.shape}")
    uv = uv.astype(np.float32)
    out = np.zeros((V, 3), dtype=np.float32)
    out[:, 0] = uv[:, 0] * np.float32(tw - 1)
    out[:, 1] = uv[:, 1] * np.float32(th - 1)
    return out


def unwrap_heads(image, vertices, triangles, uv, size=256, *, mapping: str = "bilinear", to_host: bool = True) -> HeadTextures:
    """Every head's appearance as a UV texture map cut out of ``image`` (uint8 or float [H, W, C], NumPy or a GPU tensor; a uint8 image is looked up as it
    is, never expanded to floats).  ``vertices`` [V, 3] or [n, V, 3] in image coordinates, ``uv`` [V, 2] in [0, 1] per vertex, ``size`` the atlas side or
    (th, tw).  A texel shows the FIRST triangle of the list that holds it (all atlas depths are 0 and ties keep the earlier triangle)."""
    th, tw = _atlas_size(size)
    n, V, th, tw, mapping_id, mode, z_sign = check_arguments(shape_of(vertices), th, tw, mapping, "order", 1.0)
    i_shape = shape_of(image)
    if len(i_shape) != 3:
        raise ValueError(f"image must be [H, W, C], got {i_shape}")
    _check_texture(i_shape, n, "image")
    C = i_shape[2]
    if C > _lib_tex.MAX_CHANNELS:
        raise ValueError(f"image: {C} channels exceed {_lib_tex.MAX_CHANNELS}")
    tri = check_triangles(triangles, V, "unwrap_heads")
    atlas = atlas_vertices(uv, V, th, tw)
    dev = _device_of(vertices, image)
    coords = to_device(vertices, dev, torch.float32).reshape(n, V, 3)
    tex = to_device(image, dev, _texture_dtype(image)).reshape(1, i_shape[0], i_shape[1], C)
    v = torch.from_numpy(atlas).to(dev).unsqueeze(0).expand(n, V, 3).contiguous()
    dst = torch.zeros((n, th, tw, C), dtype=torch.float32, device=dev)
    depth = torch.empty((n, th, tw), dtype=torch.float32, device=dev)
    tri_buf = torch.empty((n, th, tw), dtype=torch.int32, device=dev)
    _launch(v, tri, tri, coords, True, tex, False, dst, depth, tri_buf, None, True, mapping_id, mode, z_sign)
    written = tri_buf >= 0
    if to_host:
        return HeadTextures(dst.cpu().numpy(), tri_buf.cpu().numpy(), written.cpu().numpy())
    return HeadTextures(dst, tri_buf, written)


def cylindrical_uv(template_vertices, triangles):
    """A UV layout from the template mesh alone (FLAME's own UV file is not among the reference's assets): the unwrap about the vertical (y) axis through
    the mesh's centre.  u = 0.5 + atan2(x, z) / 2 pi (the face, which looks along +z, lands in the middle), v = (y_max - y) / (y_max - y_min) (the top
    of the head at v = 0) -> (uv float32 [V, 2] in [0, 1], keep bool [T]).  ``keep`` marks the triangles that do not cross the seam at the back of the
    head (u span below one half); callers pass ``faces[keep]``.  A host helper."""
    ver = np.asarray(template_vertices, dtype=np.float64)
    if ver.ndim != 2 or ver.shape[1] != 3 or ver.shape[0] == 0:
        raise ValueError(f"template_vertices must be [V, 3], got {ver.shape}")
    tri = check_triangles(triangles, ver.shape[0], "cylindrical_uv")
    lo, hi = ver.min(axis=0), ver.max(axis=0)
    centre = (lo + hi) / 2
    u = 0.5 + np.arctan2(ver[:, 0] - centre[0], ver[:, 2] - centre[2]) / (2 * math.pi)
    v = (hi[1] - ver[:, 1]) / max(hi[1] - lo[1], np.finfo(np.float64).tiny)
    uv = np.clip(np.stack([u, v], axis=1), 0.0, 1.0).astype(np.float32)
    tu = uv[:, 0][tri]
    keep = (tu.max(axis=1) - tu.min(axis=1)) < 0.5 if tri.shape[0] else np.zeros((0,), dtype=bool)
    return uv, keep


# ---- what PredictionResult.get_textures and PredictionResult.render_texture do -------------------------------------------------------------------
def head_textures(image, heads, faces, uv, size=256, mapping: str = "bilinear", visible_only: bool = True, occlusion: str = "order", to_host: bool = True) -> HeadTextures:
    """``unwrap_heads`` over every head's ``vertices_3d``.  ``mask`` = ``written``; with ``visible_only`` the texel's triangle must also own at least one pixel of
    that head in ``visibility.head_visibility(heads, faces, occlusion)`` (depth = -z, like get_pncc and render_mesh)."""
    if mapping not in _lib_tex.MAPPINGS:
        raise ValueError(f"mapping must be 'bilinear' or 'nearest', got {mapping!r}")
    if occlusion not in _lib_tex.MODES:
        raise ValueError(f"occlusion must be 'order' or 'depth', got {occlusion!r}")
    faces = np.asarray(require_faces(faces))
    th, tw = _atlas_size(size)
    i_shape = shape_of(image)
    if len(i_shape) != 3:
        raise ValueError(f"the image must be [H, W, C], got {i_shape}")
    n = len(heads)
    if n == 0:
        dev = _device_of(image)
        tex = HeadTextures(torch.zeros((0, th, tw, i_shape[2]), dtype=torch.float32, device=dev), torch.zeros((0, th, tw), dtype=torch.int32, device=dev),
                           torch.zeros((0, th, tw), dtype=torch.bool, device=dev))
    else:
        tex = unwrap_heads(image, head_vertices(heads), faces, uv, (th, tw), mapping=mapping, to_host=False)
        if visible_only:
            from .visibility import head_visibility

            vis = head_visibility(heads, faces, i_shape[0], i_shape[1], occlusion=occlusion, barycentric=False, to_host=False)
            T = int(np.asarray(faces).reshape(-1, 3).shape[0])
            own = vis.head_index >= 0
            seen = torch.zeros((n * T + 1,), dtype=torch.bool, device=tex.triangle.device)  # the last entry stands for "no triangle"
            seen[(vis.head_index[own].long() * T + vis.triangle_index[own].long())] = True
            key = torch.arange(n, device=seen.device).view(n, 1, 1) * T + tex.triangle.long()
            tex.mask = tex.written & seen[torch.where(tex.written, key, torch.full_like(key, n * T))]
    if to_host:
        return HeadTextures(tex.texture.cpu().numpy(), tex.triangle.cpu().numpy(), tex.written.cpu().numpy(), tex.mask.cpu().numpy())
    return tex


def paint_heads(image, heads, faces, textures, uv, mapping: str = "bilinear", occlusion: str = "order", to_host: bool = True):
    """A NEW uint8 [H, W, 3] image: every head painted from its own texture ([n, th, tw, C]) or from a shared one ([th, tw, C]), uint8 or float, over a float32
    copy of ``image``, depth = -z; the float32 result is clamped to [0, 255] and truncated to bytes."""
    if mapping not in _lib_tex.MAPPINGS:
        raise ValueError(f"mapping must be 'bilinear' or 'nearest', got {mapping!r}")
    if occlusion not in _lib_tex.MODES:
        raise ValueError(f"occlusion must be 'order' or 'depth', got {occlusion!r}")
    faces = np.asarray(require_faces(faces))
    if isinstance(textures, HeadTextures):
        textures = textures.texture
    i_shape, t_shape = shape_of(image), shape_of(textures)
    if len(i_shape) != 3 or i_shape[2] != 3:
        raise ValueError(f"the image must be [H, W, 3], got {i_shape}")
    n = len(heads)
    _check_texture(t_shape, n, "textures")
    if t_shape[-1] < 3:
        raise ValueError(f"textures need at least 3 channels, got {t_shape[-1]}")
    dev = _device_of(image, textures)
    base = to_device(image, dev, torch.float32)  # a new tensor: uint8 -> float32 is exact
    if n:
        verts = head_vertices(heads)
        atlas = atlas_vertices(uv, verts.shape[1], t_shape[-3], t_shape[-2])
        base = render_texture(verts, faces, textures, atlas, i_shape[0], i_shape[1], image=base, mapping=mapping, occlusion=occlusion, z_sign=-1.0, to_host=False)
    elif isinstance(image, torch.Tensor) and image.dtype == torch.float32:
        base = base.clone()
    out = base.clamp(0.0, 255.0).to(torch.uint8)
    return out.cpu().numpy() if to_host else out
