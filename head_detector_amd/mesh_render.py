"""The shaded mesh over the photograph: Sim3DR's ``get_normal`` and its alpha-blended ``_rasterize`` on the GPU (csrc/mesh_render.hip, libvghview.so).

  vertex_normals(vertices, triangles)        Sim3DR.get_normal for one mesh (NumPy in, NumPy out) or n meshes of one topology on the device
  blend_meshes(image, vertices, triangles, colors | shading, alpha, ...)   one ``_rasterize(alpha, reverse)`` per mesh, in order, over a copy of the image
  render_mesh(image, heads, faces, ...)      what ``PredictionResult.render_mesh`` returns, defined as this composition of reference calls:

      img = image.copy()
      for head in heads:
          v = float32 copy of head.vertices_3d, z negated            # get_pncc's convention: larger = nearer; the head's array is not modified
          n = Sim3DR.get_normal(v, faces)
          c = shade(n)
          Sim3DR_Cython.rasterize(img, v, faces, c, depth = -1e8 everywhere, T, H, W, 3, alpha, reverse=False)

  ``shade``, all float32 in this order without contraction: ``s = |(nx*lx + ny*ly) + nz*lz|``, ``t = min(1, ambient + diffuse*s)``, ``c_k = t*color_k``,
  with ``light`` normalised in float64 and rounded to float32.  Two-sided on purpose: which way a mesh's winding faces in image coordinates is not
  something this package can know, and hidden faces lose the depth test anyway.

Normals and images are bit-identical to the reference's C++ (tests/test_gpu_shaded_mesh.py).  There is no CPU path."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib_view
from .aligned import _device_image
from .mesh_geometry import check_triangles as _triangles, device_of, head_vertices, pixel_bounds, require_faces, to_device  # noqa: F401  (pixel_bounds is part of this module's surface)


def check_shading(alpha, color, ambient, diffuse, light) -> Tuple[float, Tuple[float, float, float], float, float, Tuple[float, float, float]]:
    """Validates the arguments of ``render_mesh`` (no GPU needed) -> (alpha, color, ambient, diffuse, unit light), the light normalised in float64."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:  # false for NaN
        raise ValueError(f"alpha must lie in 0 .. 1, got {alpha}")
    color = tuple(float(c) for c in color)
    if len(color) != 3 or not all(0.0 <= c <= 1.0 for c in color):
        raise ValueError(f"color must be three values in 0 .. 1, got {color}")
    ambient, diffuse = float(ambient), float(diffuse)
    if not (math.isfinite(ambient) and math.isfinite(diffuse) and ambient >= 0.0 and diffuse >= 0.0):
        raise ValueError(f"ambient and diffuse must be finite and >= 0, got {ambient}, {diffuse}")
    light = tuple(float(c) for c in light)
    if len(light) != 3 or not all(math.isfinite(c) for c in light):
        raise ValueError(f"light must be three finite values, got {light}")
    m = max(abs(c) for c in light)
    if m == 0.0:
        raise ValueError("light must not be the zero vector")
    scaled = [c / m for c in light]  # no overflow in the squares
    length = math.sqrt(sum(c * c for c in scaled))
    return alpha, color, ambient, diffuse, tuple(c / length for c in scaled)


def vertex_normals(vertices, triangles):
    """``Sim3DR.get_normal``: NumPy [V, 3] + [T, 3] -> float32 [V, 3]; a GPU tensor [n, V, 3] (n meshes, one topology) -> a GPU tensor [n, V, 3]
    without a visit to the host."""
    on_device = isinstance(vertices, torch.Tensor)
    shape = tuple(vertices.shape)
    if len(shape) != (3 if on_device else 2) or shape[-1] != 3 or shape[-2] < 1:
        raise ValueError(f"vertices must be {'a tensor [n, V, 3]' if on_device else 'an array [V, 3]'}, got {shape}")
    V = shape[-2]
    tri = _triangles(triangles, V, "get_normal")
    lib = _lib_view.load()
    dev = device_of(vertices, what="get_normal", lib="libvghview.so")
    v = to_device(vertices, dev, torch.float32)
    if not on_device:
        v = v.unsqueeze(0)
    out = torch.empty_like(v)
    with torch.cuda.device(dev):
        _lib_view.check(lib.vghv_vertex_normals(v.data_ptr(), v.shape[0], V, tri.ctypes.data, tri.shape[0], out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out if on_device else out[0].cpu().numpy()


def blend_meshes(image, vertices: torch.Tensor, triangles: np.ndarray, *, alpha: float, z_sign: float, reverse: bool = False, colors: Optional[torch.Tensor] = None,
                 shading: Optional[Tuple[Sequence[float], float, float, Sequence[float]]] = None, return_colors: bool = False):
    """``vghv_render_meshes``: a new GPU uint8 [H, W, 3] tensor = ``image`` with the n meshes ``vertices`` [n, V, 3] (GPU float32) blended over it in order.
    ``colors``: GPU float32 [V, 3] (all meshes) or [n, V, 3]; or ``shading`` = (color, ambient, diffuse, unit light): the colours are computed by the
    call.  ``return_colors=True`` also returns the per-vertex colours the rasteriser used."""
    lib = _lib_view.load()
    src = _device_image(image, "mesh renders")
    dev = src.device
    H, W = int(src.shape[0]), int(src.shape[1])
    v = vertices.detach().to(dev, torch.float32).contiguous()
    n, V = int(v.shape[0]), int(v.shape[1])
    tri = np.ascontiguousarray(triangles, dtype=np.int32)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    job = _lib_view.MeshJob()
    job.src_dev, job.src_pitch_bytes, job.dst_dev = src.data_ptr(), (src.stride(0) if H > 1 else 3 * W), out.data_ptr()
    job.height, job.width, job.channels, job.n_heads, job.n_vertices, job.n_triangles = H, W, 3, n, V, tri.shape[0]
    job.reverse, job.alpha, job.z_sign = int(bool(reverse)), alpha, z_sign
    if shading is not None:
        color, ambient, diffuse, light = shading
        colors = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
        job.shade, job.colors_per_head, job.ambient, job.diffuse = 1, 1, ambient, diffuse
        job.color, job.light = (_lib_view.C.c_float * 3)(*color), (_lib_view.C.c_float * 3)(*light)
    else:
        colors = colors.detach().to(dev, torch.float32).contiguous()
        job.colors_per_head = int(colors.dim() == 3)
    bounds = pixel_bounds(v, tri, H, W)
    if n and tri.shape[0]:
        job.verts_dev, job.triangles, job.bounds, job.colors_dev = v.data_ptr(), tri.ctypes.data, bounds.ctypes.data, colors.data_ptr()
    with torch.cuda.device(dev):
        _lib_view.check(lib.vghv_render_meshes(job, torch.cuda.current_stream().cuda_stream))
    return (out, colors) if return_colors else out


def render_mesh(image, heads, faces, alpha=0.7, color=(0.75, 0.75, 0.8), ambient=0.35, diffuse=0.65, light=(0.0, 0.0, 1.0), to_host: bool = True, return_colors: bool = False):
    """A NEW uint8 [H, W, 3] image: every head's mesh, lit and blended with ``alpha``, over a copy of ``image`` (NumPy, or a GPU uint8 tensor whose rows may
    be pitched; never modified), in the order of ``heads``.  ``to_host=False`` returns a GPU tensor.  Arguments are validated before a GPU is looked for."""
    alpha, color, ambient, diffuse, light = check_shading(alpha, color, ambient, diffuse, light)
    require_faces(faces)
    n = len(heads)
    verts = head_vertices(heads) if n else np.zeros((0, 1, 3), dtype=np.float32)
    tri = _triangles(faces, verts.shape[1], "render_mesh") if n else np.zeros((0, 3), dtype=np.int32)
    src = _device_image(image, "mesh renders")  # ValueError for a bad image, then VghError for a missing GPU
    f32 = lambda q: float(np.float32(q))  # noqa: E731
    shading = (tuple(f32(c) for c in color), f32(ambient), f32(diffuse), tuple(f32(c) for c in light))
    res = blend_meshes(src, torch.from_numpy(verts).to(src.device), tri, alpha=f32(alpha), z_sign=-1.0, shading=shading, return_colors=return_colors)
    out, cols = res if return_colors else (res, None)
    out = out.cpu().numpy() if to_host else out
    return (out, cols) if return_colors else out
