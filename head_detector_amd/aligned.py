"""Aligned head crops: ``PredictionResult.get_aligned_heads`` of the reference (head_detector/detection_result.py:56-70) with its helpers
under their own names (head_detector/utils.py:26-117):

  extend_bbox, extend_to_rect, flame_params_skull_center, get_rotation_mat, vertically_align, refined_head_bbox (host, float64)
  aligned_head_plan(image_shape, heads, head_indices)   the per-head geometry: a few dozen float64 operations, on the host
  warp_crops(image, jobs)                                the pixels: ONE launch of csrc/aligned.hip (libvghview.so) for all crops

The reference copies the whole photograph and warps all of it into a larger canvas for every head, then keeps a head-sized crop; here the
geometry is planned on the host in the reference's operation order (its ``int()`` truncations decide shapes, so the order is part of the
contract) and the device computes only the pixels that are kept.  The warp is OpenCV's 8-bit ``warpAffine(..., INTER_LINEAR)`` with the
constant-0 border; its fixed-point tables are built here in float64, the kernel is integer arithmetic only (PARITY UNPINNED against cv2 itself,
bit-exact against tests/warp_affine_ref.py).  There is no CPU path for the pixels.

Quirks of the reference that are kept: ``IMAGE_SIZE`` is the constant 640 whatever the detector's ``image_size``; the skull centre subtracts the
WHOLE padding, not half; the translation is a float32 tensor divided by a Python float; ``extend_bbox`` truncates toward zero; the crop is
``image[y:y+h, x:x+w]`` with Python slice semantics (a negative start counts from the far edge, which usually leaves an EMPTY crop: it is returned
as such, so there is one crop per head)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib_view
from ._lib import VghError
from .head_info import Bbox

IMAGE_SIZE = 640
MAX_YAW = 60
AB_SCALE = 1024  # OpenCV's AB_BITS = 10
ROUND_DELTA = 16  # AB_SCALE / INTER_TAB_SIZE / 2


def refined_head_bbox(vertices: np.ndarray, head_indices: np.ndarray) -> Bbox:
    """utils.py:26-35 on the host, in the dtype of ``vertices`` (float64 for rotated landmarks): int() of min / max over the ``head_indices`` rows.
    (``pncc.refined_head_bbox`` is the batched float32 device version.)"""
    points = np.take(vertices, np.array(head_indices), axis=0)
    x, y, x1, y1 = (int(v) for v in (points[:, 0].min(), points[:, 1].min(), points[:, 0].max(), points[:, 1].max()))
    return Bbox(x=x, y=y, w=x1 - x, h=y1 - y)


def extend_bbox(bbox, offset: Union[Tuple[float, ...], float] = 0.1) -> np.ndarray:
    """utils.py:38-66: [x, y, w, h] grown by ``offset`` (a fraction of w / h; one value, (w, h) or (left, right, top, bottom)), truncated toward zero."""
    x, y, w, h = bbox
    if isinstance(offset, tuple):
        if len(offset) == 4:
            left, right, top, bottom = offset
        elif len(offset) == 2:
            left = right = offset[0]
            top = bottom = offset[1]
    else:
        left = right = top = bottom = offset
    return np.array([x - w * left, y - h * top, w * (1.0 + right + left), h * (1.0 + top + bottom)]).astype("int32")


def extend_to_rect(bbox) -> np.ndarray:
    """utils.py:69-76: the longer side wins, the shorter one is centred with floor division."""
    x, y, w, h = bbox
    if w > h:
        return np.array([x, y - (w - h) // 2, w, w])
    return np.array([x - (h - w) // 2, y, h, h])


def _skull_center(translation, height: int, width: int) -> Tuple[int, int]:
    scale = IMAGE_SIZE / max(height, width)
    if height > width:
        new_h, new_w = IMAGE_SIZE, int(width * IMAGE_SIZE / height)
    else:
        new_h, new_w = int(height * IMAGE_SIZE / width), IMAGE_SIZE
    pad_w, pad_h = IMAGE_SIZE - new_w, IMAGE_SIZE - new_h
    centre = (torch.as_tensor(translation, dtype=torch.float32).cpu() / scale)[0].numpy()  # float32 tensor / Python float, like the reference
    return int(centre[0] - pad_w), int(centre[1] - pad_h)


def flame_params_skull_center(flame_params, image) -> Tuple[int, int]:
    """utils.py:79-90: the head's translation (padded-640 space) brought to image pixels."""
    return _skull_center(flame_params.translation, int(image.shape[0]), int(image.shape[1]))


def get_rotation_matrix_2d(center, angle: float, scale: float = 1.0) -> np.ndarray:
    """cv2.getRotationMatrix2D: [2, 3] float64; the centre is a float32 point, the angle in degrees."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    a = float(angle) * (math.pi / 180.0)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def _rotation_mat(height: int, width: int, center, angle) -> Tuple[np.ndarray, Tuple[int, int]]:
    m = get_rotation_matrix_2d(center, angle, 1.0)
    abs_cos, abs_sin = abs(m[0, 0]), abs(m[0, 1])
    bound_w = int(height * abs_sin + width * abs_cos)
    bound_h = int(height * abs_cos + width * abs_sin)
    m[0, 2] += bound_w / 2 - center[0]
    m[1, 2] += bound_h / 2 - center[1]
    return m, (bound_w, bound_h)


def get_rotation_mat(img, img_center, angle) -> Tuple[np.ndarray, Tuple[int, int]]:
    """utils.py:93-106: rotation about ``img_center`` that moves it to the middle of a canvas large enough for the rotated image -> (matrix, (bound_w, bound_h))."""
    return _rotation_mat(int(img.shape[0]), int(img.shape[1]), img_center, angle)


@dataclass
class HeadPlan:
    """Geometry of one head's crop.  ``matrix`` / ``bounds`` of an un-rotated head are the identity and the image's own (width, height)."""
    rotated: bool
    matrix: np.ndarray  # [2, 3] float64
    bounds: Tuple[int, int]  # (bound_w, bound_h) of the warped canvas
    rect: Tuple[int, int, int, int]  # (x, y, w, h) as the reference computes it, possibly outside the canvas
    region: Tuple[int, int, int, int]  # (x0, y0, x1, y1): canvas[y:y+h, x:x+w] resolved with Python slice semantics (x1 < x0 or y1 < y0: empty)

    @property
    def shape(self) -> Tuple[int, int, int]:
        x0, y0, x1, y1 = self.region
        return (max(0, y1 - y0), max(0, x1 - x0), 3)


def aligned_head_plan(image_shape: Sequence[int], heads, head_indices: np.ndarray, offset=0.1) -> List[HeadPlan]:
    """detection_result.py:56-70 without the pixels: for every head whether it is rotated (``abs(yaw) < 60``), the matrix, the canvas bounds, the
    rect and the final slice.  ``offset``: the margin of ``extend_bbox`` (the reference's 0.1)."""
    H, W = int(image_shape[0]), int(image_shape[1])
    plans = []
    for head in heads:
        vertices = head.vertices_3d
        rotated = bool(np.abs(head.head_pose.yaw) < MAX_YAW)
        if rotated:
            matrix, bounds = _rotation_mat(H, W, _skull_center(head.flame_params.translation, H, W), head.head_pose.roll)
            vertices = np.hstack([vertices[:, :2], np.ones((vertices.shape[0], 1))]) @ matrix.T  # float64, on every vertex
        else:
            matrix, bounds = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (W, H)
        box = refined_head_bbox(vertices, head_indices)
        x, y, w, h = (int(v) for v in extend_to_rect(extend_bbox([box.x, box.y, box.w, box.h], offset=offset)))
        y0, y1, _ = slice(y, y + h).indices(bounds[1])
        x0, x1, _ = slice(x, x + w).indices(bounds[0])
        plans.append(HeadPlan(rotated, matrix, bounds, (x, y, w, h), (x0, y0, x1, y1)))
    return plans


# ---- the pixels ----------------------------------------------------------------------------------------------------------------------
def invert_affine(matrix: np.ndarray) -> Tuple[float, float, float, float, float, float]:
    """warpAffine's inversion of the forward matrix, in its operation order -> (A00, A01, b0, A10, A11, b1)."""
    m = [float(v) for v in np.asarray(matrix, dtype=np.float64).reshape(6)]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11
    m[1] *= -d
    m[3] *= -d
    m[4] = a22
    return m[0], m[1], -m[0] * m[2] - m[1] * m[5], m[3], m[4], -m[3] * m[2] - m[4] * m[5]


def warp_tables(matrix: np.ndarray, region: Tuple[int, int, int, int]) -> np.ndarray:
    """int32 [adelta(w) | bdelta(w) | X0(h) | Y0(h)] of the canvas columns x0 .. x1 - 1 and rows y0 .. y1 - 1 (include/vgh_view.h): every product and
    sum a float64 operation of its own, ``np.rint`` = round half to even, saturated to int32."""
    x0, y0, x1, y1 = region
    a00, a01, b0, a10, a11, b1 = invert_affine(matrix)
    xs = np.arange(x0, x1, dtype=np.float64)
    ys = np.arange(y0, y1, dtype=np.float64)
    t = np.concatenate([a00 * xs * AB_SCALE, a10 * xs * AB_SCALE, (a01 * ys + b0) * AB_SCALE, (a11 * ys + b1) * AB_SCALE])
    t = np.clip(np.rint(t), -2147483648, 2147483647).astype(np.int64)
    t[2 * (x1 - x0):] += ROUND_DELTA
    return np.clip(t, -2147483648, 2147483647).astype(np.int32)


def _device_image(image, what: str = "aligned crops") -> torch.Tensor:
    """uint8 [H, W, 3] as a GPU tensor whose pixels are 3 bytes apart (rows may be further apart: strided views are used as they are)."""
    t = image if isinstance(image, torch.Tensor) else np.asarray(image)
    if str(t.dtype).replace("torch.", "") != "uint8" or len(t.shape) != 3 or t.shape[2] != 3:
        raise ValueError(f"{what} need a uint8 image [H,W,3]; got {t.dtype} {tuple(t.shape)}")
    if not (1 <= t.shape[0] <= _lib_view.MAX_SIDE and 1 <= t.shape[1] <= _lib_view.MAX_SIDE):
        raise ValueError(f"{what} need an image of 1 .. {_lib_view.MAX_SIDE} pixels a side; got {tuple(t.shape[:2])}")
    if not torch.cuda.is_available():
        raise VghError(f"{what} need a GPU: the HIP kernels of libvghview.so are the only implementation of the pixels")
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not t.is_cuda:
        return t.contiguous().to(torch.device("cuda", torch.cuda.current_device()))
    if t.stride(2) != 1 or t.stride(1) != 3 or (t.shape[0] > 1 and t.stride(0) < 3 * t.shape[1]):
        raise ValueError(f"{what} need pixels 3 bytes apart and rows at least 3 * W bytes apart; got strides {tuple(t.stride())}")
    return t


def warp_crops(image, jobs: Sequence[Tuple[np.ndarray, Tuple[int, int, int, int]]], to_host: bool = True) -> list:
    """``jobs`` = (matrix [2, 3], region (x0, y0, x1, y1) of the warped canvas) per crop -> per crop the uint8 [h, w, 3] bytes
    ``cv2.warpAffine(image, matrix, canvas, INTER_LINEAR)[y0:y1, x0:x1]`` would hold (empty sides stay empty).  ``image``: uint8 [H, W, 3], a NumPy
    array (uploaded once) or a GPU tensor (rows may be pitched).  One upload of descriptors + tables, one launch, one packed result buffer:
    NumPy arrays for ``to_host=True``, otherwise GPU tensors that are views into that buffer."""
    lib = _lib_view.load()
    src = _device_image(image)
    H, W = int(src.shape[0]), int(src.shape[1])
    pitch = src.stride(0) if H > 1 else 3 * W
    crops = (_lib_view.Crop * max(1, len(jobs)))()
    tables, n_tab, n_dst, shapes = [], 0, 0, []
    for c, (matrix, (x0, y0, x1, y1)) in zip(crops, jobs):
        w, h = max(0, x1 - x0), max(0, y1 - y0)
        c.src_dev, c.src_pitch_bytes, c.src_h, c.src_w, c.src_channels = src.data_ptr(), pitch, H, W, 3
        c.crop_w, c.crop_h, c.table_offset, c.dst_offset = w, h, n_tab, n_dst
        shapes.append((n_dst, h, w))
        if w and h:
            tables.append(warp_tables(matrix, (x0, y0, x1, y1)))
            n_tab += 2 * (w + h)
            n_dst += 3 * w * h
    out = torch.empty(n_dst, dtype=torch.uint8, device=src.device)
    if n_dst:
        tab = np.concatenate(tables)
        with torch.cuda.device(src.device):
            _lib_view.check(lib.vghv_warp_crops(crops, len(jobs), tab.ctypes.data, n_tab, out.data_ptr(), n_dst, torch.cuda.current_stream().cuda_stream))
    if to_host:
        host = out.cpu().numpy()
        return [host[at:at + 3 * h * w].reshape(h, w, 3) for at, h, w in shapes]
    return [out[at:at + 3 * h * w].view(h, w, 3) for at, h, w in shapes]


def vertically_align(img, vertices: np.ndarray, flame_params, roll: float):
    """utils.py:109-117: the whole image rotated by ``roll`` about the head's skull centre (uint8 [bound_h, bound_w, 3]) and the landmarks [V, 2] in
    that canvas.  Same kernel as the crops, the crop being the whole canvas."""
    matrix, bounds = get_rotation_mat(img, flame_params_skull_center(flame_params, img), roll)
    vertical_img = warp_crops(img, [(matrix, (0, 0, bounds[0], bounds[1]))])[0]
    vertices = np.hstack([vertices[:, :2], np.ones((vertices.shape[0], 1))])
    return vertical_img, vertices @ matrix.T


def get_aligned_heads(image, heads, head_indices: np.ndarray, to_host: bool = True) -> list:
    """One upright square crop per head (detection_result.py:56-70); see ``warp_crops`` for ``image`` and ``to_host``."""
    plans = aligned_head_plan(image.shape, heads, head_indices)
    if not plans:
        return []
    return warp_crops(image, [(p.matrix, p.region) for p in plans], to_host=to_host)
