"""Head visibility buffers: Sim3DR's ``rasterize_triangles`` for all heads of an image on the GPU (csrc/visibility.hip, libvghvis.so).

  rasterize_heads(vertices, triangles, height, width, occlusion=..., z_sign=...)   -> HeadVisibility

defined as this composition of reference calls (``rt`` = ``Sim3DR_Cython.rasterize_triangles``, depth = ``z_sign * z`` on a copy of the vertices):

      solo_i = rt(v_i, triangles, depth = -1e8 everywhere, triangle = -1 everywhere, weights = 0)           # one per head, fresh buffers
      occlusion="order"   for i in order: where solo_i.triangle >= 0, head i's index, triangle, depth and weights replace what is there
                          (the rule of PNCCProcessor.__call__ and of render_mesh: a later head paints over an earlier one)
      occlusion="depth"   for i in order: rt(v_i, ...) on the SAME buffers; head i owns the pixels whose depth changed during its call
                          (strict >: on equal depth the earlier head and the earlier triangle keep the pixel)
      covered_pixels[i]   = pixels with solo_i.triangle >= 0
      visible_pixels[i]   = pixels head i owns at the end
      vertex_visible[i,v] = v is a corner of a triangle t such that some pixel ends with owner (i, t)

Background: depth -1e8, triangle -1, head -1, weights 0.  Note the inside rule of ``rasterize_triangles``: ``u >= 0 and v >= 0 and u + v < 1``, not the
``w0 > 0 and w1 > 0 and w2 > 0`` of ``rasterize``.  Every output is bit-identical to the reference's C++ (tests/test_gpu_visibility.py).  There is no
CPU path."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib_vis
from .mesh_geometry import check_raster_arguments, check_triangles, device_of, head_vertices, pixel_bounds, require_faces, shape_of, to_device


class HeadVisibility:
    """What ``rasterize_heads`` measured.  NumPy arrays (``to_host=True``) or GPU tensors:
    ``head_index`` int32 [H, W] (-1 = background), ``triangle_index`` int32 [H, W] (-1), ``depth`` float32 [H, W] (-1e8), ``barycentric`` float32 [H, W, 3]
    (weights of the triangle's corners 0, 1, 2; 0) or None, ``visible_pixels`` int32 [n], ``covered_pixels`` int32 [n], ``vertex_visible`` bool [n, V]."""

    def __init__(self, head_index, triangle_index, depth, barycentric, visible_pixels, covered_pixels, vertex_visible):
        self.head_index = head_index
        self.triangle_index = triangle_index
        self.depth = depth
        self.barycentric = barycentric
        self.visible_pixels = visible_pixels
        self.covered_pixels = covered_pixels
        self.vertex_visible = vertex_visible

    def mask(self, i: int):
        """bool [H, W]: the pixels head ``i`` owns."""
        n = int(self.visible_pixels.shape[0])
        if not 0 <= int(i) < n:
            raise IndexError(f"head {i} outside the {n} heads")
        return self.head_index == int(i)

    @property
    def visible_fraction(self):
        """float64 [n]: visible_pixels / covered_pixels, 0 where a head covers nothing."""
        if isinstance(self.covered_pixels, torch.Tensor):
            vis, cov = self.visible_pixels.double(), self.covered_pixels.double()
            return torch.where(cov > 0, vis / cov.clamp(min=1.0), torch.zeros_like(vis))
        vis, cov = self.visible_pixels.astype(np.float64), self.covered_pixels.astype(np.float64)
        return np.where(cov > 0, vis / np.maximum(cov, 1.0), 0.0)

    def __repr__(self):
        return f"HeadVisibility(image={tuple(self.head_index.shape)}, heads={int(self.visible_pixels.shape[0])}, barycentric={self.barycentric is not None})"


def check_arguments(shape, height, width, occlusion, z_sign):
    """Validates what needs no GPU -> (n, V, height, width, mode, z_sign); ``shape`` is the vertices' shape."""
    return check_raster_arguments(shape, height, width, occlusion, z_sign, _lib_vis)


def rasterize_heads(vertices, triangles, height, width, *, occlusion: str = "order", z_sign: float = 1.0, barycentric: bool = True, to_host: bool = True) -> HeadVisibility:
    """``vertices``: NumPy or a GPU tensor, [V, 3] (one head) or [n, V, 3]; other dtypes are converted, nothing is modified.  ``triangles`` [T, 3], shared by all
    heads.  Arguments are validated before a GPU is looked for."""
    n, V, H, W, mode, z_sign = check_arguments(shape_of(vertices), height, width, occlusion, z_sign)
    tri = check_triangles(triangles, V, "rasterize_heads")
    dev = device_of(vertices, what="rasterize_heads", lib="libvghvis.so")
    v = to_device(vertices, dev, torch.float32).reshape(n, V, 3)
    lib = _lib_vis.load()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    tri_buf = torch.empty((H, W), dtype=torch.int32, device=dev)
    head_buf = torch.empty((H, W), dtype=torch.int32, device=dev)
    bary = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if barycentric else None
    visible = torch.empty((n,), dtype=torch.int32, device=dev)
    covered = torch.empty((n,), dtype=torch.int32, device=dev)
    vv = torch.empty((n, V), dtype=torch.uint8, device=dev)
    bounds = pixel_bounds(v, tri, H, W)  # one amin / amax on the device, 4 n floats to the host
    job = _lib_vis.Job()
    job.height, job.width, job.n_heads, job.n_vertices, job.n_triangles, job.mode, job.z_sign = H, W, n, V, tri.shape[0], mode, z_sign
    job.depth_dev, job.triangle_dev, job.head_dev = depth.data_ptr(), tri_buf.data_ptr(), head_buf.data_ptr()
    job.bary_dev = bary.data_ptr() if barycentric else None
    if n:
        job.visible_px_dev, job.covered_px_dev = visible.data_ptr(), covered.data_ptr()
        job.vertex_visible_dev = vv.data_ptr() if V else None
        if tri.shape[0]:
            job.verts_dev, job.triangles, job.bounds = v.data_ptr(), tri.ctypes.data, bounds.ctypes.data
    with torch.cuda.device(dev):
        _lib_vis.check(lib.vghvis_rasterize_triangles(job, torch.cuda.current_stream().cuda_stream))
    out = (head_buf, tri_buf, depth, bary, visible, covered, vv.bool())
    if to_host:
        out = tuple(None if t is None else t.cpu().numpy() for t in out)
    return HeadVisibility(*out)


def head_visibility(heads, faces, height, width, occlusion: str = "order", barycentric: bool = False, to_host: bool = True) -> HeadVisibility:
    """What ``PredictionResult.get_visibility`` returns: ``rasterize_heads`` over every head's ``vertices_3d`` with the FLAME model's own triangles and
    ``z_sign = -1`` (the negation get_pncc and render_mesh apply; no head's array is touched)."""
    if occlusion not in _lib_vis.MODES:
        raise ValueError(f"occlusion must be 'order' or 'depth', got {occlusion!r}")
    require_faces(faces)
    n = len(heads)
    if n:
        verts, tri = head_vertices(heads), faces
    else:  # all-background buffers, empty per-head arrays
        verts, tri = np.zeros((0, 1, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    return rasterize_heads(verts, tri, height, width, occlusion=occlusion, z_sign=-1.0, barycentric=barycentric, to_host=to_host)
