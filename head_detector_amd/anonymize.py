"""Head anonymisation on the GPU: a copy of the image in which every head is pixelated, blurred or filled (csrc/anonymize.hip, libvghanon.so).

  gaussian_taps(sigma, radius)                                      the integer Gaussian of one blur strength: int32 [radius + 1], centre first
  anonymize_plan(image_shape, heads, method, region, ...)           the host half: per head the geometry box, the cell side, the blur radius and its taps
  anonymize_heads(image, heads, method="pixelate", region="ellipse", ...)   the pixels

Every output byte is defined by the integer arithmetic include/vgh_anon.h states (restated in tests/anonymize_ref.py); the GPU result equals that
restatement bit for bit.  In short:

  regions   "box": the head's ``bbox`` grown by ``int(w * margin)`` and ``int(h * margin)`` on either side, half-open, not clipped;  "ellipse": the ellipse
            inscribed in that box;  "mesh": the head's own silhouette, the ``head_index`` buffer of ``visibility.head_visibility(occlusion="order")``, inside
            the mesh's pixel bounds.  ``owner=`` takes a caller's int32 [H, W] map instead (a segmentation mask from elsewhere): values outside [-1, n) count
            as -1, and a pixel outside its owner's box is left unchanged.  Where heads overlap, the later head owns the pixel, as in ``draw`` and ``render_mesh``.
  methods   "fill": ``color``;  "pixelate": a grid of ``cells`` cells along the box's longer side, anchored at the box's unclipped corner, every cell the
            rounded mean of ALL its in-image pixels;  "blur": a separable integer Gaussian, sigma = ``strength * max(box sides)``, radius = ceil(3 sigma),
            replicate border.  Every effect reads the source image only.

The number of kernel launches does not depend on the number of heads.  There is no CPU path for the pixels.  A blur radius above 1024 raises instead of
blurring less: a silently weaker blur on a large head would be the wrong failure for a privacy function ("pixelate" has no such limit).

A ``video.YUV420Frame`` is anonymised in its own luma and chroma planes, in place if wanted, by ``video.anonymize_frame`` (``PredictionResult.anonymize_frame``);
this module works on RGB images.  Out of scope: dilating a mesh or mask region, and hair outside the FLAME mesh -- ``margin`` with "box" or "ellipse" is the lever for that."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib_anon
from .aligned import _device_image
from .mesh_geometry import check_triangles, head_vertices, pixel_bounds, require_faces

METHODS = ("pixelate", "blur", "fill")
REGIONS = ("box", "ellipse", "mesh")


@dataclass
class AnonymizePlan:
    """Everything csrc/anonymize.hip needs besides the images and the owner map."""
    heads: np.ndarray  # _lib_anon.HEAD_DTYPE [n]: x0, y0, x1, y1 (half-open, unclipped), cell, radius, tap_offset, reserved
    taps: np.ndarray  # int32: the blur tables, one per distinct (sigma, radius), end to end
    method: int  # VGHAN_METHOD_*
    sigmas: np.ndarray  # float64 [n]: the blur's sigma per head (0 for the other methods)


def gaussian_taps(sigma: float, radius: int) -> np.ndarray:
    """int32 [radius + 1], tap 0 the centre, ``taps[0] + 2 * taps[1:].sum() == 65536`` exactly: ``q_k = floor(65536 * g_k / G + 0.5)`` for k >= 1 in float64
    with ``g_k = exp(-k^2 / (2 sigma^2))`` and ``G = g_0 + 2 (g_1 + ... + g_r)``; the centre takes the remainder.  ``radius = 0`` is the identity [65536]."""
    radius, sigma = int(radius), float(sigma)
    if not 0 <= radius <= _lib_anon.MAX_RADIUS:
        raise ValueError(f"gaussian_taps: radius {radius} outside 0 .. {_lib_anon.MAX_RADIUS}")
    if radius == 0:
        return np.array([_lib_anon.TAP_SUM], dtype=np.int32)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"gaussian_taps: sigma must be finite and positive for radius {radius}, got {sigma}")
    k = np.arange(radius + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    total = g[0] + 2.0 * g[1:].sum()
    taps = np.floor(_lib_anon.TAP_SUM * g / total + 0.5).astype(np.int64)
    taps[0] = _lib_anon.TAP_SUM - 2 * int(taps[1:].sum())
    return taps.astype(np.int32)


def _check_choice(method: str, region: str) -> None:
    if method not in METHODS:
        raise ValueError(f"anonymize: method must be one of {METHODS}, got {method!r}")
    if region not in REGIONS:
        raise ValueError(f"anonymize: region must be one of {REGIONS}, got {region!r}")


def anonymize_plan(image_shape: Sequence[int], heads, method: str, region: str, margin: float = 0.1, cells: int = 8, strength: float = 0.1, bounds=None, tables=None) -> AnonymizePlan:
    """The host half of ``anonymize_heads``; no GPU.  ``bounds``: for ``region="mesh"`` the int32 [n, 4] of ``mesh_geometry.pixel_bounds`` (inclusive, clipped).
    ``tables``: an empty ``TapTables`` to put the blur tables into, for a caller that appends rows of its own (``video.anonymize_frame``: the chroma rows).
    Raises ValueError naming the head for a bad box, a side above 32767 or a blur radius above 1024."""
    _check_choice(method, region)
    H, W = int(image_shape[0]), int(image_shape[1])
    if not (1 <= H <= _lib_anon.MAX_SIDE and 1 <= W <= _lib_anon.MAX_SIDE):
        raise ValueError(f"anonymize: the image must have 1 .. {_lib_anon.MAX_SIDE} pixels a side, got {H} x {W}")
    n = len(heads)
    if n > _lib_anon.MAX_HEADS:
        raise ValueError(f"anonymize: {n} heads exceed {_lib_anon.MAX_HEADS}")
    margin, strength = float(margin), float(strength)
    if not (math.isfinite(margin) and margin >= 0):
        raise ValueError(f"anonymize: margin must be finite and >= 0, got {margin}")
    if not (math.isfinite(strength) and strength >= 0):
        raise ValueError(f"anonymize: strength must be finite and >= 0, got {strength}")
    if int(cells) != cells or not 1 <= int(cells) <= _lib_anon.MAX_CELLS:
        raise ValueError(f"anonymize: cells must be an integer in 1 .. {_lib_anon.MAX_CELLS}, got {cells}")
    cells = int(cells)
    if region == "mesh":
        if bounds is None:
            raise ValueError('anonymize: region="mesh" needs the meshes\' pixel bounds')
        bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 4)
        if bounds.shape[0] != n:
            raise ValueError(f"anonymize: {bounds.shape[0]} rows of bounds for {n} heads")
    boxes = []
    for i, head in enumerate(heads):
        if region == "mesh":
            x0, y0, x1, y1 = (int(v) for v in bounds[i])
            x1, y1 = x1 + 1, y1 + 1  # inclusive -> half-open
            if x1 <= x0 or y1 <= y0:  # a mesh that paints nothing
                x1, y1 = x0, y0
        else:
            x, y, w, h = (int(v) for v in head.bbox)
            if w < 0 or h < 0:
                raise ValueError(f"anonymize: head {i}: bbox {tuple(head.bbox)} has a negative side")
            mx, my = int(w * margin), int(h * margin)
            x0, y0, x1, y1 = x - mx, y - my, x + w + mx, y + h + my
        boxes.append((x0, y0, x1, y1))
    tables = TapTables() if tables is None else tables
    rows, sigmas = plan_rows(boxes, method, cells, strength, tables)
    return AnonymizePlan(rows, tables.taps(), _lib_anon.METHODS[method], sigmas)


class TapTables:
    """The blur tables of one call, one per distinct (sigma, radius), end to end: several ``plan_rows`` (the luma and the chroma rows of a frame) may share one."""

    def __init__(self):
        self._tables, self._offsets, self._n = [], {}, 0

    def offset(self, sigma: float, radius: int) -> int:
        if (sigma, radius) not in self._offsets:
            self._offsets[(sigma, radius)] = self._n
            self._tables.append(gaussian_taps(sigma, radius))
            self._n += radius + 1
        return self._offsets[(sigma, radius)]

    def taps(self) -> np.ndarray:
        return np.concatenate(self._tables).astype(np.int32) if self._tables else np.zeros(0, dtype=np.int32)


def plan_rows(boxes, method: str, cells: int, strength: float, tables: TapTables):
    """The plan from explicit geometry boxes (x0, y0, x1, y1), half-open and unclipped: -> (rows [n] of ``_lib_anon.HEAD_DTYPE``, sigmas float64 [n]).  Per head
    the cell side ``max(1, ceil(max side / cells))`` (pixelate), or ``sigma = strength * max side``, ``radius = ceil(3 sigma)`` and the offset of its table in
    ``tables`` (blur).  Raises ValueError naming the head for a side above 32767, a corner beyond 2^24 or a radius above 1024."""
    n = len(boxes)
    rows = np.zeros(n, dtype=_lib_anon.HEAD_DTYPE)
    sigmas = np.zeros(n, dtype=np.float64)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        wb, hb = x1 - x0, y1 - y0
        if max(wb, hb) > _lib_anon.MAX_SIDE:
            raise ValueError(f"anonymize: head {i}: box sides {wb} x {hb} exceed {_lib_anon.MAX_SIDE}")
        if max(abs(x0), abs(y0)) >= _lib_anon.MAX_COORD:
            raise ValueError(f"anonymize: head {i}: box corner ({x0}, {y0}) outside +-2**24 pixels")
        cell = radius = at = 0
        if method == "pixelate":
            cell = max(1, -(-max(wb, hb) // cells))
        elif method == "blur":
            sigma = strength * max(wb, hb)
            radius = math.ceil(3.0 * sigma)
            if radius > _lib_anon.MAX_RADIUS:
                raise ValueError(f'anonymize: head {i}: a blur of strength {strength} on a box of {wb} x {hb} pixels needs radius {radius} > {_lib_anon.MAX_RADIUS}; '
                                 'use method="pixelate", which has no such limit, or a smaller strength')
            sigmas[i] = sigma
            at = tables.offset(sigma, radius)
        rows[i] = (x0, y0, x1, y1, cell, radius, at, 0)
    return rows, sigmas


def _check_color(color) -> int:
    c = [int(v) for v in color]
    if len(c) != 3 or any(not 0 <= v <= 255 or v != w for v, w in zip(c, color)):
        raise ValueError(f"anonymize: color must be three integers in 0 .. 255, got {tuple(color)}")
    return c[0] | c[1] << 8 | c[2] << 16


def _byte_range(t: torch.Tensor):
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) * t.element_size()
    return t.data_ptr(), t.data_ptr() + last + t.element_size()


def _plan_on_host(shape, heads, method: str, region: str, margin, cells, strength, owner, tables=None) -> Optional[AnonymizePlan]:
    """The front half that ``anonymize_heads`` and ``video.anonymize_frame`` share, without a GPU: the checks of ``owner`` against the (H, W) of ``shape``, and the
    plan -- or, for ``region="mesh"`` with heads, None after the argument checks alone: their boxes are the meshes' pixel bounds, which ``_plan_on_device`` finds."""
    n = len(heads)
    if owner is not None and tuple(owner.shape) != tuple(shape[:2]):
        raise ValueError(f"anonymize: owner must be int32 {tuple(shape[:2])}, got {tuple(owner.shape)}")
    if owner is not None and str(owner.dtype).replace("torch.", "") != "int32":
        raise ValueError(f"anonymize: owner must be int32, got {owner.dtype}")
    if region != "mesh" or n == 0:
        return anonymize_plan(shape, heads, method, "box" if n == 0 else region, margin, cells, strength, tables=tables)
    anonymize_plan(shape, [], method, region, margin, cells, strength, bounds=np.zeros((0, 4)))  # the argument checks that need neither heads nor a GPU
    return None


def _plan_on_device(plan: Optional[AnonymizePlan], dev, shape, heads, method: str, region: str, margin, cells, strength, faces, owner, tables=None):
    """The back half, on GPU ``dev``: -> (plan, owner_dev).  A plan that ``_plan_on_host`` left open is made from the meshes' pixel bounds, and the mesh silhouettes
    are the owner map unless the caller brought one (libvghvis.so paints them, Python hands the buffer over); ``owner_dev`` is a contiguous int32 [H, W] tensor on
    ``dev``, or None where the library paints the owner map from the boxes."""
    H, W = int(shape[0]), int(shape[1])
    owner_dev = None
    if plan is None:
        from .visibility import head_visibility

        verts = torch.from_numpy(head_vertices(heads)).to(dev)
        tri = check_triangles(faces, verts.shape[1], "anonymize")
        plan = anonymize_plan(shape, heads, method, region, margin, cells, strength, bounds=pixel_bounds(verts, tri, H, W), tables=tables)
        if owner is None:
            owner_dev = head_visibility(heads, faces, H, W, occlusion="order", barycentric=False, to_host=False).head_index
    if owner is not None:
        owner_dev = owner.to(dev) if isinstance(owner, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(owner)).to(dev)
    if owner_dev is not None:
        owner_dev = owner_dev.contiguous()
    return plan, owner_dev


def anonymize_heads(image, heads, method: str = "pixelate", region: str = "ellipse", *, margin: float = 0.1, cells: int = 8, strength: float = 0.1, color=(0, 0, 0),
                    faces=None, owner=None, out=None, to_host: bool = True):
    """A NEW uint8 [H, W, 3] image: ``image`` with every head anonymised (the module text states the rules).  ``image`` is a NumPy array (uploaded once) or a
    GPU uint8 tensor with pixels 3 bytes apart (rows may be pitched); it is never modified.  ``owner``: an int32 [H, W] map to use instead of the region's own
    (NumPy or a GPU tensor); ``region`` then only chooses the geometry boxes.  ``out``: a contiguous GPU uint8 [H, W, 3] tensor to write into (video loops); it
    must not overlap the source.  ``to_host=False`` returns a GPU tensor.  Errors that need no GPU come first: the method, the region, missing ``faces`` for
    "mesh", the colour, bad boxes and exceeded caps (ValueError naming the head); then a missing GPU (``VghError``)."""
    _check_choice(method, region)
    if region == "mesh":
        require_faces(faces)
    colour = _check_color(color)
    shape = tuple(image.shape)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"anonymised images need a uint8 image [H,W,3]; got {shape}")
    n = len(heads)
    plan = _plan_on_host(shape, heads, method, region, margin, cells, strength, owner)
    lib = _lib_anon.load()
    src = _device_image(image, "anonymised images")
    H, W = int(src.shape[0]), int(src.shape[1])
    dev = src.device
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3) and out.is_contiguous()):
            raise ValueError(f"anonymize: out must be a contiguous GPU uint8 tensor {(H, W, 3)} on {dev}")
        (s0, s1), (d0, d1) = _byte_range(src), _byte_range(out)
        if s0 < d1 and d0 < s1:
            raise ValueError("anonymize: out overlaps the source image (the source is never modified)")
    plan, owner_dev = _plan_on_device(plan, dev, shape, heads, method, region, margin, cells, strength, faces, owner)
    job = _lib_anon.Job()
    job.src_dev, job.src_pitch_bytes, job.dst_dev = src.data_ptr(), (src.stride(0) if H > 1 else 3 * W), out.data_ptr()
    job.height, job.width, job.n_heads, job.method, job.color = H, W, n, plan.method, colour
    job.region = _lib_anon.REGION_MAP if owner_dev is not None else _lib_anon.REGION_ELLIPSE if region == "ellipse" else _lib_anon.REGION_BOX
    if n:
        job.heads = plan.heads.ctypes.data
    if plan.taps.size:
        job.taps, job.n_taps = plan.taps.ctypes.data, plan.taps.size
    if owner_dev is not None:
        job.owner_dev = owner_dev.data_ptr()
    need = int(lib.vghan_workspace_bytes(job))
    if need <= 0:
        _lib_anon.check(-1)  # raises with the library's own message
    with torch.cuda.device(dev):
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)  # allocated, used and (by the caching allocator) reused in the order of this stream
        _lib_anon.check(lib.vghan_anonymize(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy() if to_host else out
