"""Head tensors: the heads of one image, one video frame or a whole batch as ONE dense, normalised tensor for the next network (face recognition, attributes,
gaze, liveness, a quality filter), with the map back to image coordinates.

    t = result.get_head_tensors(112, dtype=torch.float16)              # t.tensor [n, 3, 112, 112] on the GPU, t.matrices [n, 2, 3], t.to_image(points, i)
    t = head_tensors_batch(detector.detect_batch(frames, rgb="none"))  # video frames: cut out of their own YUV planes, t.image_index [sum n]

  head_tensor_plan(image_shape, heads, size, ...)   the host half, float64: per head six Q32 coefficients, the supersampling factor and the crop-to-image matrix
  head_tensors(source, heads, size, ...)            the pixels: ONE staging upload and ONE launch of csrc/head_tensors.hip (libvghcrop.so) for all heads
  head_tensors_batch(results, size, ...)            the same single call over the heads of many results

The rule of the pixels is stated once, in include/vgh_crop.h, restated in tests/head_tensors_ref.py and equal to it bit for bit: every output pixel is the mean of
K x K bilinear sub-samples (5-bit fractions, integer arithmetic), K = min(8, ceil(side / size)) unless ``supersample`` says otherwise, so a large head is
box-filtered down instead of aliased -- up to a point: a head larger than 8 * size pixels a side is sampled sparsely.  uint8 output is the rounded mean; float
output is ``fl32(fl32(sum * a_c) + b_c)`` with ``a_c = scale / (1024 K^2 std_c)`` and ``b_c = -mean_c / std_c`` formed here in float64 and rounded once; float16
and bfloat16 are the round-to-nearest-even conversions of that.  A YUV tap is converted to RGB bytes by the integer rule of ``video.YUV420Frame.to_rgb`` before
the weights are applied, so a frame gives exactly what ``to_rgb()`` gives; no RGB copy is written.

Geometry.  ``aligned=True`` is that of ``get_aligned_heads``: the head rotated upright about its skull centre (``aligned.aligned_head_plan``, needs
``head_indices``) and the square rect around its refined box.  ``aligned=False`` needs no asset: the square around ``bbox`` grown by ``margin``, un-rotated.  The
rect is never sliced: a head that leaves the image gets a full crop with ``fill`` where there is no image, so there is one tensor per head, always.
There is no CPU path for the pixels."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib_crop
from ._lib import VghError
from .aligned import aligned_head_plan, extend_bbox, extend_to_rect, invert_affine
from .video import YUV420Frame

Q32 = 4294967296.0  # 2^32
ROUND_FRACTION = 1 << 26  # half of a 1/32 pixel in Q32: rounds the 5-bit fraction to nearest
DTYPES = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16", torch.uint8: "uint8"}


@dataclass
class HeadTensorPlan:
    """The host half of a call.  ``coefficients`` [n, 6] int64: (X0, XP, XQ, Y0, YP, YQ) of include/vgh_crop.h; ``supersample`` [n] int32: K; ``matrices`` [n, 2, 3]
    float64: crop pixel centre (column, row, 1) -> image pixel (x, y); ``sides`` [n]: the side of the square rect each crop shows."""
    size: int
    coefficients: np.ndarray
    supersample: np.ndarray
    matrices: np.ndarray
    sides: np.ndarray

    def __len__(self) -> int:
        return int(self.supersample.shape[0])


@dataclass
class HeadTensors:
    """``tensor``: [n, 3, S, S] or [n, S, S, 3] on the GPU; ``matrices`` [n, 2, 3] float64 and ``supersample`` [n] as in the plan; ``image_index`` [n]: the
    result (of ``head_tensors_batch``) each head came from, zeros for a single source."""
    tensor: torch.Tensor
    matrices: np.ndarray
    supersample: np.ndarray
    image_index: np.ndarray

    def to_image(self, points, i: int) -> np.ndarray:
        """``points`` [m, 2] (column, row) in pixels of crop ``i`` (integer = pixel centre) -> [m, 2] float64 image coordinates (x, y)."""
        p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        m = self.matrices[i]
        return p @ m[:, :2].T + m[:, 2]


# ---- argument checks: ValueError, the argument named, nothing here needs a GPU ----------------------------------------------------------------------
def _check_size(size) -> int:
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= int(size) <= _lib_crop.MAX_SIZE:
        raise ValueError(f"size must be an integer in 1 .. {_lib_crop.MAX_SIZE}, got {size!r}")
    return int(size)


def _check_supersample(supersample):
    if isinstance(supersample, str):
        if supersample != "auto":
            raise ValueError(f'supersample must be "auto" or an integer in 1 .. {_lib_crop.MAX_SUPERSAMPLE}, got {supersample!r}')
        return None
    if isinstance(supersample, bool) or not isinstance(supersample, (int, np.integer)) or not 1 <= int(supersample) <= _lib_crop.MAX_SUPERSAMPLE:
        raise ValueError(f'supersample must be "auto" or an integer in 1 .. {_lib_crop.MAX_SUPERSAMPLE}, got {supersample!r}')
    return int(supersample)


def _check_margin(margin) -> float:
    if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) or not math.isfinite(margin) or margin < 0:
        raise ValueError(f"margin must be a finite number >= 0, got {margin!r}")
    return float(margin)


def _check_shape(image_shape) -> tuple:
    shape = tuple(int(v) for v in image_shape)
    if len(shape) < 2 or not (1 <= shape[0] <= _lib_crop.MAX_SIDE and 1 <= shape[1] <= _lib_crop.MAX_SIDE):
        raise ValueError(f"image_shape must be (H, W, ...) with sides in 1 .. {_lib_crop.MAX_SIDE}, got {shape}")
    return shape


def _triple(value, name: str) -> List[float]:
    try:
        v = [float(x) for x in value]
    except TypeError:
        v = []
    if len(v) != 3 or not all(math.isfinite(x) for x in v):
        raise ValueError(f"{name} must be three finite numbers (in the output's channel order), got {value!r}")
    return v


def _missing_head_indices() -> FileNotFoundError:
    return FileNotFoundError("get_head_tensors(aligned=True) needs the reference's mesh asset flame_indices/head_indices.npy: "
                             "construct HeadDetector(..., assets_dir=<reference>/head_detector/assets) or pass head_indices= (aligned=False needs no asset)")


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------------
def head_tensor_plan(image_shape: Sequence[int], heads, size: int, *, aligned: bool = True, margin: float = 0.1, supersample="auto", head_indices=None) -> HeadTensorPlan:
    """Per head, in float64: the square rect (x, y, side, side) on the (warped) canvas and the forward matrix -- ``aligned.aligned_head_plan`` as it is for
    ``aligned=True`` (``margin`` is its ``offset``; needs ``head_indices``), the identity and ``extend_to_rect(extend_bbox(head.bbox, margin))`` otherwise --
    then ``side = max(side, 1)``, ``K = min(8, max(1, ceil(side / size)))`` unless ``supersample`` is an integer, and the six coefficients: sub-sample p along a
    row lies at canvas coordinate ``x + (p + 0.5) side / (size K) - 0.5`` (likewise along a column), its image position is ``invert_affine(matrix)`` of that
    point, and each coefficient is ``rint(. * 2^32)`` with 2^26 added to X0 and Y0 (the 5-bit fraction rounds to nearest).  The rect is NOT sliced."""
    S = _check_size(size)
    forced = _check_supersample(supersample)
    margin = _check_margin(margin)
    shape = _check_shape(image_shape)
    if aligned:
        if head_indices is None:
            raise _missing_head_indices()
        geometry = [(p.matrix, p.rect) for p in aligned_head_plan(shape, heads, head_indices, offset=margin)]
    else:
        identity = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        geometry = [(identity, tuple(int(v) for v in extend_to_rect(extend_bbox(list(head.bbox), margin)))) for head in heads]
    n = len(geometry)
    if n > _lib_crop.MAX_HEADS:
        raise ValueError(f"{n} heads exceed the {_lib_crop.MAX_HEADS} of one call")
    coefficients, ks = np.zeros((n, 6), np.int64), np.zeros(n, np.int32)
    matrices, sides = np.zeros((n, 2, 3), np.float64), np.zeros(n, np.int64)
    for i, (matrix, (x, y, w, h)) in enumerate(geometry):
        side = max(int(w), 1)
        K = forced if forced is not None else min(_lib_crop.MAX_SUPERSAMPLE, max(1, -(-side // S)))
        a00, a01, b0, a10, a11, b1 = invert_affine(matrix)
        step = side / (S * K)  # canvas pixels between sub-samples
        cx, cy = x + 0.5 * step - 0.5, y + 0.5 * step - 0.5  # sub-sample (0, 0)
        values = (a00 * cx + a01 * cy + b0, a00 * step, a01 * step, a10 * cx + a11 * cy + b1, a10 * step, a11 * step)
        reach = max(abs(values[0]), abs(values[3])) + S * K * max(abs(values[1]) + abs(values[2]), abs(values[4]) + abs(values[5]))
        if not reach < 2.0 ** 29:  # (a NaN fails this too) in Q32 every position then stays below 2^61 + 2^26 < 2^62, the library's bound
            raise ValueError(f"head {i}: its crop reaches more than 2^29 pixels from the image's origin (rect {(x, y, side, side)})")
        q = [int(np.rint(v * Q32)) for v in values]
        q[0] += ROUND_FRACTION
        q[3] += ROUND_FRACTION
        coefficients[i], ks[i], sides[i] = q, K, side
        pitch = side / S  # canvas pixels between crop pixel centres
        px, py = x + 0.5 * pitch - 0.5, y + 0.5 * pitch - 0.5
        matrices[i] = [[a00 * pitch, a01 * pitch, a00 * px + a01 * py + b0], [a10 * pitch, a11 * pitch, a10 * px + a11 * py + b1]]
    return HeadTensorPlan(S, coefficients, ks, matrices, sides)


# ---- sources ------------------------------------------------------------------------------------------------------------------------------------------
def _source_shape(source, what: str = "source") -> tuple:
    """(H, W, 3) of a source, with every check that needs no GPU."""
    if isinstance(source, YUV420Frame):
        shape = source.shape
        if not source.y.is_cuda:
            raise ValueError(f"{what}: the planes of a video.YUV420Frame must lie on the GPU (they are used where they are); got {source.device}")
    elif isinstance(source, (np.ndarray, torch.Tensor)):
        shape = tuple(int(v) for v in source.shape)
        if str(source.dtype).replace("torch.", "") != "uint8" or len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"{what} must be a uint8 image [H, W, 3] or a video.YUV420Frame; got {source.dtype} {shape}")
        if isinstance(source, torch.Tensor) and source.is_cuda and (source.stride(2) != 1 or source.stride(1) != 3 or (shape[0] > 1 and source.stride(0) < 3 * shape[1])):
            raise ValueError(f"{what} needs pixels 3 bytes apart and rows at least 3 * W bytes apart; got strides {tuple(source.stride())}")
    else:
        raise ValueError(f"{what} must be a uint8 image [H, W, 3] (NumPy or GPU tensor) or a video.YUV420Frame; got {type(source).__name__}")
    if not (1 <= shape[0] <= _lib_crop.MAX_SIDE and 1 <= shape[1] <= _lib_crop.MAX_SIDE):
        raise ValueError(f"{what} must have sides in 1 .. {_lib_crop.MAX_SIDE}; got {shape[:2]}")
    return shape


def _describe(source, row: "_lib_crop.Source", device: torch.device):
    """Fill ``row`` for a source on ``device`` -> what must stay alive while the call's work is queued."""
    if isinstance(source, YUV420Frame):
        h, w, _ = source.shape
        row.kind, row.h, row.w, row.chroma_step = _lib_crop.SOURCE_YUV420, h, w, source.chroma_step
        row.y_dev, row.u_dev, row.v_dev = source.y.data_ptr(), source.u.data_ptr(), source.v.data_ptr()
        row.y_pitch_bytes, row.uv_pitch_bytes = source.y_pitch, source.uv_pitch
        row.y_offset, row.cy, row.crv, row.cgu, row.cgv, row.cbu = source.coefficients
        return source
    t = source if isinstance(source, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(source))
    if not t.is_cuda:
        t = t.contiguous().to(device)
    h, w = int(t.shape[0]), int(t.shape[1])
    row.kind, row.h, row.w, row.rgb_dev, row.rgb_pitch_bytes = _lib_crop.SOURCE_RGB, h, w, t.data_ptr(), (t.stride(0) if h > 1 else 3 * w)
    return t


# ---- the pixels ---------------------------------------------------------------------------------------------------------------------------------------
def _head_tensors(items, size, *, aligned, margin, mean, std, scale, dtype, layout, channel_order, fill, supersample, out) -> HeadTensors:
    """``items``: (source, heads, head_indices) per result.  Errors in this order: ValueError (arguments), FileNotFoundError (head_indices), VghError (GPU)."""
    S = _check_size(size)
    _check_supersample(supersample)
    _check_margin(margin)
    if not isinstance(dtype, torch.dtype) or dtype not in DTYPES:
        raise ValueError(f"dtype must be one of torch.float32, torch.float16, torch.bfloat16, torch.uint8; got {dtype!r}")
    if layout not in _lib_crop.LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(_lib_crop.LAYOUTS)}, got {layout!r}")
    if channel_order not in _lib_crop.ORDERS:
        raise ValueError(f"channel_order must be one of {sorted(_lib_crop.ORDERS)}, got {channel_order!r}")
    mean, std = _triple(mean, "mean"), _triple(std, "std")
    if any(s == 0.0 for s in std):
        raise ValueError(f"std must not hold a zero, got {tuple(std)}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not math.isfinite(scale):
        raise ValueError(f"scale must be a finite number, got {scale!r}")
    fill_bytes = _triple(fill, "fill")
    if any(v != int(v) or not 0 <= v <= 255 for v in fill_bytes):
        raise ValueError(f"fill must be three integers in 0 .. 255 (in the output's channel order), got {fill!r}")
    shapes = [_source_shape(source, "source" if len(items) == 1 else f"the source of result {k}") for k, (source, _, _) in enumerate(items)]
    n = sum(len(heads) for _, heads, _ in items)
    if n > _lib_crop.MAX_HEADS:
        raise ValueError(f"{n} heads exceed the {_lib_crop.MAX_HEADS} of one call")
    result_shape = (n, 3, S, S) if layout == "nchw" else (n, S, S, 3)
    if out is not None and not (isinstance(out, torch.Tensor) and tuple(out.shape) == result_shape and out.dtype == dtype and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {result_shape}; got {getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")
    if aligned and any(head_indices is None for _, _, head_indices in items):
        raise _missing_head_indices()
    plans = [head_tensor_plan(shape, heads, S, aligned=aligned, margin=margin, supersample=supersample, head_indices=head_indices)
             for shape, (_, heads, head_indices) in zip(shapes, items)]
    if not torch.cuda.is_available():
        raise VghError("head tensors need a GPU: the HIP kernel of libvghcrop.so is the only implementation of the pixels")
    lib = _lib_crop.load()
    on_device = [d for d in (s.device if isinstance(s, YUV420Frame) else s.device if isinstance(s, torch.Tensor) and s.is_cuda else None for s, _, _ in items) if d is not None]
    device = on_device[0] if on_device else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda" or any(d != device for d in on_device):
        raise ValueError(f"every source must lie on one GPU; got {sorted({str(d) for d in on_device})}")
    if out is not None and out.device != device:
        raise ValueError(f"out must lie on {device}, the device of the source; got {out.device}")
    matrices = np.concatenate([p.matrices for p in plans]) if plans else np.zeros((0, 2, 3))
    ks = np.concatenate([p.supersample for p in plans]) if plans else np.zeros(0, np.int32)
    image_index = np.concatenate([np.full(len(p), k, np.int64) for k, p in enumerate(plans)]) if plans else np.zeros(0, np.int64)
    with torch.cuda.device(device):
        tensor = out if out is not None else torch.empty(result_shape, dtype=dtype, device=device)
        if n == 0:
            return HeadTensors(tensor, matrices, ks, image_index)
        sources = (_lib_crop.Source * len(items))()
        keep = [_describe(source, row, device) for row, (source, _, _) in zip(sources, items)]
        rows = np.zeros(n, _lib_crop.HEAD_DTYPE)
        coefficients = np.concatenate([p.coefficients for p in plans])
        for k, name in enumerate(("x0", "xp", "xq", "y0", "yp", "yq")):
            rows[name] = coefficients[:, k]
        rows["source"], rows["supersample"] = image_index, ks
        job = _lib_crop.Job()
        if dtype != torch.uint8:  # float64, rounded once
            d = 1024.0 * ks.astype(np.float64) ** 2
            rows["a"] = (float(scale) / (d[:, None] * np.array(std, np.float64)[None, :])).astype(np.float32)
            job.b[:] = [float(np.float32(-m / s)) for m, s in zip(mean, std)]
        job.sources, job.heads, job.n_sources, job.n_heads, job.size = _lib_crop.C.addressof(sources), rows.ctypes.data, len(items), n, S
        job.dtype, job.layout, job.channel_order = _lib_crop.DTYPES[DTYPES[dtype]], _lib_crop.LAYOUTS[layout], _lib_crop.ORDERS[channel_order]
        job.fill = int(fill_bytes[0]) | int(fill_bytes[1]) << 8 | int(fill_bytes[2]) << 16
        job.dst_dev, job.dst_bytes = tensor.data_ptr(), tensor.numel() * tensor.element_size()
        _lib_crop.check(lib.vghc_head_tensors(job, torch.cuda.current_stream().cuda_stream))
        del keep  # (an upload made here is freed, and its memory reused, in the order of this stream)
    return HeadTensors(tensor, matrices, ks, image_index)


def head_tensors(source, heads, size: int = 224, *, aligned: bool = True, margin: float = 0.1, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), scale: float = 1 / 255,
                 dtype=torch.float32, layout: str = "nchw", channel_order: str = "rgb", fill=(0, 0, 0), supersample="auto", head_indices=None,
                 out: Optional[torch.Tensor] = None) -> HeadTensors:
    """Every head of ``source`` as one ``size`` x ``size`` crop in one tensor: ``(pixel * scale - mean) / std`` per channel in ``dtype`` (float32, float16,
    bfloat16), or the bytes themselves (uint8: ``mean``, ``std`` and ``scale`` are ignored).  ``source``: a NumPy uint8 image [H, W, 3] (uploaded once), a GPU
    uint8 image (rows may be pitched) or a ``video.YUV420Frame`` (its planes are used where they are).  ``layout``: "nchw" or "nhwc"; ``channel_order``: "rgb"
    or "bgr"; ``mean``, ``std`` and ``fill`` are given in the OUTPUT's channel order.  ``fill``: the bytes where a crop shows no image.  ``supersample``: "auto"
    (K = min(8, ceil(side / size)): a head larger than 8 * size pixels is sampled sparsely) or K itself.  ``aligned`` / ``margin`` / ``head_indices``: see
    ``head_tensor_plan``.  ``out``: a preallocated contiguous tensor of exactly the result's shape, dtype and device.  No heads: an empty tensor, nothing is
    queued.  Errors: ValueError for the arguments, then FileNotFoundError for missing ``head_indices``, then VghError for a missing GPU or library."""
    return _head_tensors([(source, heads, head_indices)], size, aligned=aligned, margin=margin, mean=mean, std=std, scale=scale, dtype=dtype, layout=layout,
                         channel_order=channel_order, fill=fill, supersample=supersample, out=out)


def head_tensors_batch(results, size: int = 224, *, aligned: bool = True, margin: float = 0.1, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), scale: float = 1 / 255,
                       dtype=torch.float32, layout: str = "nchw", channel_order: str = "rgb", fill=(0, 0, 0), supersample="auto", head_indices=None,
                       out: Optional[torch.Tensor] = None) -> HeadTensors:
    """The heads of a list of ``PredictionResult`` in ONE call and one tensor [sum n, ...], in the results' order; ``image_index`` [sum n] names each head's
    result.  A result's source is its ``source_frame`` if it has one, otherwise its ``original_image``, so ``detect_batch(frames, rgb="none")`` followed by this
    gives one batch for the next model.  ``head_indices``: for every result; otherwise each result's own.  The other keywords are those of ``head_tensors``."""
    items = []
    for k, r in enumerate(results):
        source = r.source_frame if getattr(r, "source_frame", None) is not None else r.original_image
        if source is None:
            raise ValueError(f"result {k} has neither a source_frame nor an original_image")
        items.append((source, r.heads, head_indices if head_indices is not None else getattr(r, "head_indices", None)))
    return _head_tensors(items, size, aligned=aligned, margin=margin, mean=mean, std=std, scale=scale, dtype=dtype, layout=layout, channel_order=channel_order,
                         fill=fill, supersample=supersample, out=out)
