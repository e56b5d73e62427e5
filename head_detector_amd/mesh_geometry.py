"""What the mesh rasterisers' Python wrappers share (``mesh_render`` for libvghview.so, ``visibility`` for libvghvis.so, ``texture`` for libvghtex.so) and
what belongs to no one library: the argument checks that need no GPU, the placement of host or device data on a GPU, the heads' stacked vertices, the check
of a triangle list and the per-mesh pixel bounds all three C calls take as a contract.  Loads no library."""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import VghError


def shape_of(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def device_of(*candidates, what: str, lib: str):
    """The device of the first GPU tensor among the arguments; host data alone needs a GPU to be present (``what`` and ``lib`` word the error)."""
    for c in candidates:
        if isinstance(c, torch.Tensor):
            if not c.is_cuda:
                raise ValueError("a torch tensor must live on the GPU (pass NumPy for host data)")
            return c.device
    if not torch.cuda.is_available():
        raise VghError(f"{what} needs a GPU: the HIP kernels of {lib} are the only implementation")
    return torch.device("cuda", torch.cuda.current_device())


def to_device(a, dev, dtype):
    """A contiguous tensor of ``dtype`` on ``dev``; the caller's array or tensor is never written."""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError("a torch tensor must live on the GPU (pass NumPy for host data)")
        return a.detach().to(device=dev, dtype=dtype).contiguous()
    np_dtype = {torch.float32: np.float32, torch.uint8: np.uint8}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(dev)


def check_raster_arguments(v_shape, height, width, occlusion, z_sign, lib):
    """Validates what needs no GPU -> (n, V, height, width, mode, z_sign); ``v_shape`` is the vertices' shape, ``lib`` the binding whose limits and mode
    table hold (``_lib_vis``, ``_lib_tex``)."""
    if occlusion not in lib.MODES:
        raise ValueError(f"occlusion must be 'order' or 'depth', got {occlusion!r}")
    z_sign = float(z_sign)
    if z_sign not in (1.0, -1.0):
        raise ValueError(f"z_sign must be +1 or -1, got {z_sign}")
    v_shape = tuple(v_shape)
    if len(v_shape) not in (2, 3) or v_shape[-1] != 3:
        raise ValueError(f"vertices must be [V, 3] or [n, V, 3], got {v_shape}")
    height, width = int(height), int(width)
    if not (1 <= height <= lib.MAX_SIDE and 1 <= width <= lib.MAX_SIDE):
        raise ValueError(f"height x width must lie in 1 .. {lib.MAX_SIDE}, got {height} x {width}")
    n = v_shape[0] if len(v_shape) == 3 else 1
    if n > lib.MAX_HEADS:
        raise ValueError(f"{n} heads exceed {lib.MAX_HEADS}")
    return n, v_shape[-2], height, width, lib.MODES[occlusion], z_sign


def head_vertices(heads) -> np.ndarray:
    """float32 [n, V, 3]: every head's ``vertices_3d``, stacked (n >= 1); no head's array is touched."""
    verts = np.stack([np.asarray(h.vertices_3d, dtype=np.float32) for h in heads])
    if verts.ndim != 3 or verts.shape[2] != 3:
        raise ValueError(f"heads must carry vertices_3d [V, 3], got {verts.shape[1:]}")
    return verts


def require_faces(faces):
    if faces is None:
        raise ValueError("no triangle list available (FLAME model without faces)")
    return faces


def check_triangles(triangles, V: int, what: str) -> np.ndarray:
    tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3), dtype=np.int32)
    if tri.size and (int(tri.min()) < 0 or int(tri.max()) >= V):
        raise ValueError(f"{what}: triangle index outside the {V} vertices")
    return tri


def pixel_bounds(vertices: torch.Tensor, triangles: np.ndarray, H: int, W: int) -> np.ndarray:
    """int32 [n, 4] (x0, y0, x1, y1), inclusive: per mesh the union of its triangles' clamped integer boxes -- max(ceil(min x), 0) ..
    min(floor(max x), W - 1) over the vertices the triangles name, y alike; x1 < x0 = paints nothing.  A mesh with a non-finite coordinate gets
    the whole image (its finite triangles may lie anywhere).  One reduction on the device, 4 n floats to the host."""
    n = vertices.shape[0]
    out = np.zeros((n, 4), dtype=np.int32)
    out[:, 2:] = -1
    if n == 0 or triangles.size == 0:
        return out
    used = torch.from_numpy(np.unique(triangles).astype(np.int64)).to(vertices.device)
    xy = vertices[:, used, :2]
    ext = torch.cat([torch.amin(xy, dim=1), torch.amax(xy, dim=1)], dim=1).cpu().numpy().astype(np.float64)  # NaN propagates through amin / amax
    for i in range(n):
        x0, y0, x1, y1 = ext[i]
        if not all(math.isfinite(q) for q in (x0, y0, x1, y1)):
            out[i] = (0, 0, W - 1, H - 1)
            continue
        out[i] = (max(math.ceil(max(x0, -1.0)), 0), max(math.ceil(max(y0, -1.0)), 0), min(math.floor(min(x1, float(W))), W - 1), min(math.floor(min(y1, float(H))), H - 1))
    return out
