"""``PredictionResult.draw`` of the reference (head_detector/detection_result.py:12-18,45-51 and head_detector/draw_utils.py) on the GPU:

  draw_plan(image_shape, heads, method, ...)    the host half: which classes a method paints, the int32 points (truncation toward zero), the
                                                boxes, the dot radius and its half-width table -- a few array operations, no per-primitive work
  draw_heads(image, heads, method, ...)         the pixels: csrc/draw.hip (libvghview.so) expands every box, triangle edge and dot on the device

Methods and what they paint per head, in this order (a later class over an earlier one, a later head over an earlier head):

  "bbox"       box                               cv2.rectangle(image, (x, y), (x + w, y + h), (255, 0, 0), 2)
  "landmarks"  wire, dots(head_indices)          cv2.polylines(closed, (0, 0, 255), thickness 1) per row of ``triangles``; cv2.circle(..., R, (255, 255, 255), -1)
  "points"     dots(face_indices)
  "full"       box, wire, dots(head_indices)

with ``R = max(1, int(min(H, W) * 0.001))``.  The reference draws the "full" view with 4 816 polylines and 2 470 circle calls per head from a
Python loop; here the number of kernel launches does not depend on the number of heads.  The pixel rules are OpenCV 4.x's as restated in
tests/draw_ref.py: PARITY UNPINNED against cv2 itself (bit-exact against that restatement; ``tools/first_contact.py --cv2`` and a host test
pin it wherever cv2 is installed).  There is no CPU path for the pixels.

``"pose"`` is not implemented: its arrows are oblique lines of thickness ``int(sqrt(area) * 0.03)``, which OpenCV draws from thickness 2 on with
its 16.16 fixed-point polygon filler; that rule has not been restated byte-exactly, and an approximate picture under the reference's name would
be worse than an error.  The class list and the colour table of csrc/draw.hip leave room for it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib_view
from .aligned import _device_image

# method -> (paints boxes, paints the wire, which index list the dots use); the reference's DRAW_MAPPING without "pose"
METHODS = {"bbox": (True, False, None), "landmarks": (False, True, "head_indices"), "points": (False, False, "face_indices"), "full": (True, True, "head_indices")}
ASSET_FILES = {"triangles": "triangles.txt", "head_indices": "flame_indices/head_indices.npy", "face_indices": "flame_indices/face.npy"}


class DrawAssetsMissing(NotImplementedError, FileNotFoundError):
    """A draw method needs a mesh asset that was not supplied.  Both what this package raises for a missing asset (FileNotFoundError naming the
    file) and what ``draw`` raised before it existed (NotImplementedError), so that callers written against either keep working."""


@dataclass
class DrawPlan:
    """Everything csrc/draw.hip needs besides the image; ``None`` = the class is not painted."""
    points: np.ndarray  # int32 [n, V, 2]
    boxes: Optional[np.ndarray]  # int32 [n, 4]: x, y, w, h
    triangles: Optional[np.ndarray]  # int32 [T, 3]
    indices: Optional[np.ndarray]  # int32 [K]
    radius: int
    half_widths: np.ndarray  # int32 [radius + 1]


def half_widths(radius: int) -> np.ndarray:
    """Half the width of the filled circle's row at distance 0 .. R from its centre row (OpenCV's midpoint loop): R = 1 -> [1, 0], a plus."""
    hw = [0] * (radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return np.array(hw, dtype=np.int32)


def _classes(method: str):
    if method == "pose":
        raise NotImplementedError('PredictionResult.draw("pose") is not implemented: its thick oblique arrows follow OpenCV\'s fixed-point polygon filler, which has not been '
                                  'restated byte-exactly; "full", "bbox", "landmarks" and "points" are')
    return METHODS[method]  # KeyError(method) like the reference's dictionary lookup


def _require_assets(method: str, triangles, head_indices, face_indices) -> None:
    box, wire, dots = _classes(method)
    have = {"triangles": triangles, "head_indices": head_indices, "face_indices": face_indices}
    missing = [k for k in (["triangles"] if wire else []) + ([dots] if dots else []) if have[k] is None]
    if missing:
        files = ", ".join(ASSET_FILES[k] for k in missing)
        raise DrawAssetsMissing(f'draw("{method}") needs the reference\'s mesh asset(s) {files}: construct HeadDetector(..., assets_dir=<reference>/head_detector/assets) '
                                f"or pass {', '.join(k + '=' for k in missing)} to PredictionResult")


def draw_plan(image_shape: Sequence[int], heads, method: str = "full", *, triangles=None, head_indices=None, face_indices=None) -> DrawPlan:
    """The host half of ``draw``.  Points are ``(int(v[0]), int(v[1]))`` of the float32 vertices: truncation toward zero, -0.7 -> 0; a non-finite
    coordinate or one with ``|v| >= 2**24`` raises ValueError naming the head (the reference raises or overflows there)."""
    box, wire, dots = _classes(method)
    _require_assets(method, triangles, head_indices, face_indices)
    H, W = int(image_shape[0]), int(image_shape[1])
    n = len(heads)
    xy = np.stack([np.asarray(h.vertices_3d, dtype=np.float32)[:, :2] for h in heads]) if n else np.zeros((0, 1, 2), dtype=np.float32)
    bad = ~(np.abs(xy) < _lib_view.MAX_COORD)  # NaN and inf compare false
    if bad.any():
        i = int(np.argmax(bad.reshape(n, -1).any(axis=1)))
        raise ValueError(f"draw: head {i}: a vertex is not finite or outside +-2**24 pixels")
    boxes = None
    if box:
        boxes = np.zeros((n, 4), dtype=np.int32)
        for i, h in enumerate(heads):
            x, y, w, hh = (int(v) for v in h.bbox)
            if w < 0 or hh < 0 or max(abs(x), abs(y), w, hh) >= _lib_view.MAX_COORD:
                raise ValueError(f"draw: head {i}: bbox {tuple(h.bbox)} needs w, h >= 0 and values below 2**24")
            boxes[i] = (x, y, w, hh)
    V = xy.shape[1]
    tri = idx = None
    if wire:
        tri = np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3), dtype=np.int32)
    if dots:
        idx = np.ascontiguousarray(np.array({"head_indices": head_indices, "face_indices": face_indices}[dots]).reshape(-1), dtype=np.int32)
    for name, a in (("triangles", tri), (dots, idx)):
        if a is not None and n and a.size and (int(a.min()) < 0 or int(a.max()) >= V):
            raise ValueError(f"draw: {name} index outside the {V} vertices of a head")
    radius = max(1, int(min(H, W) * 0.001))
    return DrawPlan(np.ascontiguousarray(np.trunc(xy).astype(np.int32)), boxes, tri, idx, radius, half_widths(radius))


def draw_heads(image, heads, method: str = "full", *, triangles=None, head_indices=None, face_indices=None, to_host: bool = True):
    """A NEW uint8 [H, W, 3] image: ``image`` with every head drawn in the reference's order.  ``image`` is a NumPy array (uploaded once) or a GPU
    uint8 tensor with pixels 3 bytes apart (rows may be pitched); it is never modified.  ``to_host=False`` returns a GPU tensor.  Errors that need
    no GPU come first: the method, a missing asset (``DrawAssetsMissing``), bad vertices or boxes (ValueError); then a missing GPU (``VghError``)."""
    plan = draw_plan(image.shape, heads, method, triangles=triangles, head_indices=head_indices, face_indices=face_indices)
    lib = _lib_view.load()
    src = _device_image(image, "drawn images")
    H, W = int(src.shape[0]), int(src.shape[1])
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=src.device)
    n = len(heads)
    job = _lib_view.DrawJob()
    job.src_dev, job.src_pitch_bytes, job.dst_dev = src.data_ptr(), (src.stride(0) if H > 1 else 3 * W), out.data_ptr()
    job.height, job.width, job.channels, job.n_heads, job.n_vertices, job.radius = H, W, 3, n, plan.points.shape[1], plan.radius
    job.points, job.half_widths = plan.points.ctypes.data, plan.half_widths.ctypes.data
    if n and plan.boxes is not None:
        job.boxes = plan.boxes.ctypes.data
    if n and plan.triangles is not None:
        job.triangles, job.n_triangles = plan.triangles.ctypes.data, plan.triangles.shape[0]
    if n and plan.indices is not None:
        job.indices, job.n_indices = plan.indices.ctypes.data, plan.indices.shape[0]
    with torch.cuda.device(src.device):
        _lib_view.check(lib.vghv_draw_heads(job, torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy() if to_host else out
