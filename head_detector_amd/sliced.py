"""Sliced detection for large photographs: the tile plan (host), the cross-tile merge on the device (libvghmerge.so, include/vgh_merge.h) and the conversion of a
tile's FLAME parameters to the convention of a whole-image detection.  ``HeadDetector.detect_sliced`` puts them together.

The photograph is cut into overlapping tiles, the network runs on the tiles as batches (each tile a pitched sub-view of the photograph on the device, letterboxed
by VGH_IMG_U8_RAW: an S x S tile reaches the network as the photograph's own bytes), a low-resolution pass over the whole image picks up the heads larger than a
tile overlap, and the per-tile detections are merged into one list in image coordinates.  The merge rule is stated once, in include/vgh_merge.h; DESIGN.md 3.6
repeats it and tests/slice_merge_ref.py restates it in NumPy.  ``border`` (2 source pixels) and ``overlap`` (25 %) are API defaults, NOT tuned values: no real
weights exist in this tree to tune them on."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .letterbox import geometry

# columns of SlicePlan.tiles
OFF_X, OFF_Y, TILE_W, TILE_H, PAD_X, PAD_Y, NEW_W, NEW_H = range(8)
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8  # bits of SlicePlan.interior


@dataclass
class SlicePlan:
    """The tiles of one photograph.  Row t of ``tiles`` = (off_x, off_y, w, h, pad_x, pad_y, new_w, new_h): the tile's rectangle in the image and its letterbox
    geometry for the S x S network input (letterbox.geometry)."""

    height: int
    width: int
    image_size: int
    tiles: np.ndarray  # int32 [T, 8]
    scale: np.ndarray  # float32 [T]: S / max(h, w) of the tile
    interior: np.ndarray  # uint8 [T]: bit 0 left (off_x > 0), bit 1 top, bit 2 right (off_x + w < width), bit 3 bottom; 0 for the whole image
    unpad: np.ndarray  # float32 [T, 3] = (pad_x - off_x * scale, pad_y - off_y * scale, scale): un-pads a tile's vertices straight into image coordinates

    @property
    def n_tiles(self) -> int:
        return int(self.tiles.shape[0])


def axis_offsets(length: int, tile: int, overlap: float) -> list:
    """Offsets of the tiles of size ``tile`` along an axis of ``length`` pixels: one tile [0, length) if it fits, else a stride of
    max(1, int(tile * (1 - overlap))) with the last tile shifted back to end at ``length`` (never ragged)."""
    if length <= tile:
        return [0]
    stride = max(1, int(tile * (1 - overlap)))
    n = -(-(length - tile) // stride) + 1
    return [min(k * stride, length - tile) for k in range(n)]


def plan_slices(height: int, width: int, image_size: int, tile_sizes: Optional[Sequence[int]] = None, overlap: float = 0.25, include_full: bool = True) -> SlicePlan:
    """The tile plan of a ``height`` x ``width`` photograph for a detector of input size ``image_size``.  ``tile_sizes`` (default: one entry, ``image_size``): the tiles
    of every size are the Cartesian product of the axis offsets, row-major; with ``include_full`` tile 0 is the whole image; a tile with the offset and size of an
    earlier one is dropped (an image no larger than a tile).  Raises ValueError for ``overlap`` outside [0, 0.9], a non-positive size, and a tile too elongated for
    the letterbox (the condition the raw-image path rejects: a letterboxed side below one pixel)."""
    height, width, S = int(height), int(width), int(image_size)
    if height < 1 or width < 1 or S < 1:
        raise ValueError(f"plan_slices: height x width {height} x {width} and image_size {S} must be positive")
    if not (isinstance(overlap, (int, float)) and 0.0 <= overlap <= 0.9):
        raise ValueError(f"plan_slices: overlap {overlap!r} outside [0, 0.9]")
    sizes = (S,) if tile_sizes is None else tuple(tile_sizes)
    rects = [(0, 0, width, height)] if include_full else []
    for t in sizes:
        if int(t) != t or t < 1:
            raise ValueError(f"plan_slices: tile size {t!r} is not a positive integer")
        t = int(t)
        ys, xs = axis_offsets(height, t, overlap), axis_offsets(width, t, overlap)
        rects += [(x, y, min(t, width), min(t, height)) for y in ys for x in xs]
    seen, rows = set(), []
    for r in rects:
        if r in seen:
            continue
        seen.add(r)
        x, y, w, h = r
        new_h, new_w, pad_x, pad_y, scale = geometry(h, w, S)
        if new_h < 1 or new_w < 1:
            raise ValueError(f"plan_slices: tile {len(rows)} ({h} x {w} at ({x}, {y})) is too elongated for a {S}x{S} letterbox")
        interior = (LEFT if x > 0 else 0) | (TOP if y > 0 else 0) | (RIGHT if x + w < width else 0) | (BOTTOM if y + h < height else 0)
        rows.append(((x, y, w, h, pad_x, pad_y, new_w, new_h), scale, interior))
    if not rows:
        raise ValueError("plan_slices: no tile (tile_sizes is empty and include_full is False)")
    tiles = np.array([r[0] for r in rows], dtype=np.int32).reshape(-1, 8)
    scale = np.array([r[1] for r in rows], dtype=np.float64)
    unpad = np.stack([tiles[:, PAD_X] - tiles[:, OFF_X] * scale, tiles[:, PAD_Y] - tiles[:, OFF_Y] * scale, scale], axis=1)  # float64, rounded once
    return SlicePlan(height, width, S, tiles, scale.astype(np.float32), np.array([r[2] for r in rows], dtype=np.uint8), unpad.astype(np.float32))


def to_whole_image_params(translation, scale_net, tile: Sequence[int], height: int, width: int, image_size: int):
    """A tile head's network translation [3] (padded S-space of the TILE) and scale -> (translation', scale') in the convention ``HeadDetector.__call__`` leaves a
    whole-image detection in: translation in the padded S-space of the WHOLE image, scale divided by the letterbox scale -- so that everything downstream
    (get_aligned_heads' skull centre with the reference's padding quirk included) treats a sliced head like any other.  With s_f, pad_f the whole image's
    letterbox geometry and s_t, pad_t, off the tile's:  scale' = scale_net / s_t;  translation'[:2] = (t - pad_t) * (s_f / s_t) + off * s_f + pad_f;
    translation'[2] = t_z * (s_f / s_t).  A tile whose geometry IS the whole image's passes the translation through untouched.  Works on NumPy arrays of any
    float type (and on torch tensors)."""
    off_x, off_y, w, h, pad_x, pad_y = (int(v) for v in tile[:6])
    _, _, fpx, fpy, s_f = geometry(height, width, image_size)
    s_t = geometry(h, w, image_size)[4]  # the Python float __call__ divides by
    new_scale = scale_net / s_t
    if (off_x, off_y, w, h) == (0, 0, int(width), int(height)):
        return translation, new_scale
    k = s_f / s_t
    out = translation * k  # a copy; z is done
    out[..., 0] = (translation[..., 0] - pad_x) * k + (off_x * s_f + fpx)
    out[..., 1] = (translation[..., 1] - pad_y) * k + (off_y * s_f + fpy)
    return out, new_scale


def image_boxes(boxes_full: np.ndarray, head_tile: np.ndarray, plan: SlicePlan) -> np.ndarray:
    """The integer boxes of the merged heads: rint(boxes_full) clipped to the image -- except for the heads of a tile that IS the whole image, which keep
    exactly what ``HeadDetector.__call__`` reports for them: its boxes are clipped to the padded S x S canvas only and may reach into the letterbox border,
    i.e. past the image, and a plan with only the whole-image tile reproduces ``__call__`` head for head."""
    bb = np.rint(np.asarray(boxes_full, dtype=np.float32).reshape(-1, 4)).astype(int)
    part = ~(plan.tiles[:, :4] == [0, 0, plan.width, plan.height]).all(axis=1)[np.asarray(head_tile, dtype=np.int64)]
    bb[np.ix_(part, [0, 2])] = bb[np.ix_(part, [0, 2])].clip(0, plan.width)
    bb[np.ix_(part, [1, 3])] = bb[np.ix_(part, [1, 3])].clip(0, plan.height)
    return bb


@dataclass
class MergedHeads:
    """What ``merge_tiles`` returns: capacity-sized tensors on the GPU; rows [0, n_heads) are heads, the rows behind hold -1 / zeros."""

    head_row: "torch.Tensor"  # int32 [max_heads] = t * keep_k + r
    head_tile: "torch.Tensor"  # int32 [max_heads]
    boxes_full: "torch.Tensor"  # float32 [max_heads, 4] xyxy in image coordinates
    scores: "torch.Tensor"  # float32 [max_heads]
    n_heads: "torch.Tensor"  # int32 [1]
    n_kept_uncapped: "torch.Tensor"  # int32 [1]: kept candidates before the max_heads cap
    status: Optional["torch.Tensor"] = None  # uint8 [T * keep_k]: 0 absent, 1 kept, 2 truncated, 3 suppressed, 4 over the cap


@dataclass
class SliceInfo:
    """``detect_sliced(return_info=True)``: the plan, the source tile of every head and how many candidates ended in each status."""

    plan: SlicePlan
    head_tile: np.ndarray  # int32 [n]
    status_counts: Dict[str, int]  # absent / kept / truncated / suppressed / over_cap
    n_kept_uncapped: int


STATUS_NAMES = ("absent", "kept", "truncated", "suppressed", "over_cap")


def merge_tiles(boxes, scores, counts, plan: SlicePlan, *, border: float = 2.0, match_thr: float = 0.5, metric: str = "iou", max_heads: int = 1000,
                want_status: bool = False) -> MergedHeads:
    """The cross-tile merge (vghm_merge_tiles) of per-tile slabs exactly as ``VGHeadsEngine.detect`` leaves them: ``boxes`` [T, keep_k, 4] xyxy in the padded S-space
    of each tile, ``scores`` [T, keep_k], ``counts`` [T] int32, all contiguous on one GPU, T = ``plan.n_tiles``.  Queued on the current stream; nothing is read
    back.  ``border``: a detection that comes within this many SOURCE pixels of an edge of its tile that lies inside the image is taken for a truncated head and
    dropped (an API default, not a tuned value); ``metric`` "iou" or "ios" (intersection over the smaller box) against ``match_thr``."""
    import torch

    from . import _lib_merge

    if metric not in _lib_merge.METRICS:
        raise ValueError(f"merge_tiles: metric {metric!r} is neither 'iou' nor 'ios'")
    if int(max_heads) != max_heads or not 1 <= max_heads <= _lib_merge.MAX_HEADS:
        raise ValueError(f"merge_tiles: max_heads {max_heads!r} outside 1 .. {_lib_merge.MAX_HEADS}")
    if not (math.isfinite(border) and border >= 0):
        raise ValueError(f"merge_tiles: border {border!r} is not a finite non-negative number")
    if math.isnan(match_thr):
        raise ValueError("merge_tiles: match_thr is NaN")
    for name, t, dtype in (("boxes", boxes, torch.float32), ("scores", scores, torch.float32), ("counts", counts, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"merge_tiles: {name} must be a {dtype} tensor; got {getattr(t, 'dtype', type(t))}")
    T = plan.n_tiles
    if boxes.dim() != 3 or boxes.shape[0] != T or boxes.shape[1] < 1 or boxes.shape[2] != 4:
        raise ValueError(f"merge_tiles: boxes must be [T = {T}, keep_k >= 1, 4]; got {tuple(boxes.shape)}")
    keep_k = int(boxes.shape[1])
    if tuple(scores.shape) != (T, keep_k) or tuple(counts.shape) != (T,):
        raise ValueError(f"merge_tiles: scores must be [{T}, {keep_k}] and counts [{T}]; got {tuple(scores.shape)} and {tuple(counts.shape)}")
    for name, t in (("boxes", boxes), ("scores", scores), ("counts", counts)):
        if not t.is_cuda or t.device != boxes.device or not t.is_contiguous():
            raise ValueError(f"merge_tiles: {name} must be a contiguous tensor on the GPU of boxes (there is no CPU path)")
    lib = _lib_merge.load()
    dev = boxes.device
    tiles = np.ascontiguousarray(plan.tiles, dtype=np.int32)
    scale = np.ascontiguousarray(plan.scale, dtype=np.float32)
    interior = np.ascontiguousarray(plan.interior, dtype=np.uint8)
    with torch.cuda.device(dev):
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        out = MergedHeads(torch.empty(max_heads, **i32), torch.empty(max_heads, **i32), torch.empty(max_heads, 4, **f32), torch.empty(max_heads, **f32),
                          torch.empty(1, **i32), torch.empty(1, **i32), torch.empty(T * keep_k, dtype=torch.uint8, device=dev) if want_status else None)
        ws = torch.empty(max(16, int(lib.vghm_merge_workspace_bytes(T, keep_k))), dtype=torch.uint8, device=dev)  # 0 bytes = sizes the call itself rejects
        job = _lib_merge.MergeJob(T, keep_k, int(plan.image_size), int(max_heads), _lib_merge.METRICS[metric], float(border), float(match_thr), 0, boxes.data_ptr(),
                                  scores.data_ptr(), counts.data_ptr(), tiles.ctypes.data, scale.ctypes.data, interior.ctypes.data, out.head_row.data_ptr(),
                                  out.head_tile.data_ptr(), out.boxes_full.data_ptr(), out.scores.data_ptr(), out.n_heads.data_ptr(), out.n_kept_uncapped.data_ptr(),
                                  out.status.data_ptr() if want_status else None)
        _lib_merge.check(lib.vghm_merge_tiles(_lib_merge.C.byref(job), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out
