"""What the mesh rasterisers' Python wrappers share (``mesh_render`` for libvghview.so, ``visibility`` for libvghvis.so) and what belongs to neither
library: the check of a triangle list and the per-mesh pixel bounds both C calls take as a contract.  Loads no library."""
from __future__ import annotations

import math

import numpy as np
import torch


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
