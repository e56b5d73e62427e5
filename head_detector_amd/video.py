"""Video frames as decoders deliver them: 8-bit YUV 4:2:0 (NV12 / NV21 surfaces of a hardware decoder, planar I420 of a software one) straight into the detector.

    frame = YUV420Frame.from_nv12(surface, height, width, pitch=surface_pitch, uv_offset=aligned_height * surface_pitch)   # views of the surface, no copy
    predictions = detector(frame)                 # or detector.detect_batch(frames), tracker.update(frame), engine.detect(frames)

The library converts every tap to RGB while it letterboxes (VGH_IMG_YUV420_RAW, csrc/letterbox.hip): no RGB copy of the frame is written.  The conversion is the
integer rule stated in include/vgh.h (vgh_yuv420_image) -- nearest chroma sample, 16.16 fixed-point coefficients, every pixel clamped to bytes:

    c = Y - y_offset, d = U - 128, e = V - 128
    R = clamp8((cy*c + crv*e + 32768) >> 16),  G = clamp8((cy*c + cgu*d + cgv*e + 32768) >> 16),  B = clamp8((cy*c + cbu*d + 32768) >> 16)

``YUV420Frame.to_rgb()`` is that rule in torch integer ops (CPU or GPU tensors); the detector's result is defined as "``to_rgb()``, then what an RGB image gets".
PARITY UNPINNED against cv2.cvtColor (cv2 rounds its coefficients to another fixed-point precision): ``tools/first_contact.py --cv2`` reports the difference.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np
import torch

# (Kr, Kb) of the luma equation Y = Kr R + Kg G + Kb B, Kg = 1 - Kr - Kb
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def yuv_coefficients(matrix: str = "bt709", full_range: bool = False) -> Tuple[int, int, int, int, int, int]:
    """-> (y_offset, cy, crv, cgu, cgv, cbu): the fixed-point coefficients (* 2^16) of vgh_yuv420_image, rounded (``round``: half to even; no value is a tie) from
    the float64 (Kr, Kb) definition of ``matrix``, Kg = 1 - Kr - Kb:

        limited range: y_offset = 16, sy = 255 / 219, sc = 255 / 224        full range: y_offset = 0, sy = sc = 1
        cy  = round(65536 * sy)
        crv = round(65536 * sc * 2 (1 - Kr))                  R = sy (Y - y_offset) + sc 2 (1 - Kr) (V - 128)
        cbu = round(65536 * sc * 2 (1 - Kb))                  B = sy (Y - y_offset) + sc 2 (1 - Kb) (U - 128)
        cgu = round(65536 * sc * -2 Kb (1 - Kb) / Kg)         G = (Y - Kr R - Kb B) / Kg
        cgv = round(65536 * sc * -2 Kr (1 - Kr) / Kg)"""
    if matrix not in MATRICES:
        raise ValueError(f"yuv_coefficients: matrix {matrix!r} is not one of {sorted(MATRICES)}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    q = lambda v: int(round(65536.0 * v))  # noqa: E731
    return (0 if full_range else 16, q(sy), q(sc * 2.0 * (1.0 - kr)), q(sc * -2.0 * kb * (1.0 - kb) / kg), q(sc * -2.0 * kr * (1.0 - kr) / kg), q(sc * 2.0 * (1.0 - kb)))


def _as_tensor(a, what: str) -> torch.Tensor:
    """A uint8 tensor as it is (CPU or GPU); a NumPy array uploaded once to the current GPU."""
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            raise ValueError(f"{what}: expected uint8; got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8:
        raise ValueError(f"{what}: expected a uint8 tensor or array; got {getattr(a, 'dtype', type(a))}")
    return a


def _pitch(t: torch.Tensor, dim: int, need: int) -> int:
    """Stride of ``dim`` in elements; a dimension of size 1 has no meaningful stride: the smallest valid one."""
    return int(t.stride(dim)) if t.shape[dim] > 1 else max(int(t.stride(dim)), need)


class YUV420Frame:
    """One 8-bit YUV 4:2:0 frame: ``y`` uint8 [h, w] (rows may be pitched: strides (pitch, 1)), ``u`` and ``v`` uint8 [(h+1)//2, (w+1)//2] with strides
    (uv_pitch, chroma_step) -- chroma_step 1 for planar planes, 2 for the two interleaved views of an NV12 / NV21 chroma plane.  The tensors are kept as given
    (views are not copied); all three on one device.  NumPy planes are uploaded once to the current GPU (planar only: an interleaved pair is one buffer, see
    ``from_nv12``).  ``matrix`` / ``full_range`` choose the coefficients (``yuv_coefficients``)."""

    def __init__(self, y, u, v, *, chroma_step: int, matrix: str = "bt709", full_range: bool = False):
        if chroma_step not in (1, 2):
            raise ValueError(f"YUV420Frame: chroma_step {chroma_step} (1 = planar, 2 = interleaved)")
        if chroma_step == 2 and any(isinstance(p, np.ndarray) for p in (u, v)):
            raise ValueError("YUV420Frame: interleaved NumPy chroma views would be uploaded as two buffers; use from_nv12 / from_nv21 with the whole surface")
        y, u, v = _as_tensor(y, "YUV420Frame: y"), _as_tensor(u, "YUV420Frame: u"), _as_tensor(v, "YUV420Frame: v")
        if y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1:
            raise ValueError(f"YUV420Frame: y must be [h, w] with h, w >= 1; got {tuple(y.shape)}")
        h, w = int(y.shape[0]), int(y.shape[1])
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if tuple(u.shape) != (ch, cw) or tuple(v.shape) != (ch, cw):
            raise ValueError(f"YUV420Frame: a {h} x {w} frame has chroma planes [{ch}, {cw}]; got u {tuple(u.shape)}, v {tuple(v.shape)}")
        if not (y.device == u.device == v.device):
            raise ValueError(f"YUV420Frame: planes on different devices: {y.device}, {u.device}, {v.device}")
        if w > 1 and y.stride(1) != 1:
            raise ValueError(f"YUV420Frame: the luma samples of a row must be dense (strides (pitch, 1)); got {y.stride()}")
        y_pitch = _pitch(y, 0, w)
        if y_pitch < w:
            raise ValueError(f"YUV420Frame: luma pitch {y_pitch} < width {w}")
        for name, p in (("u", u), ("v", v)):
            if cw > 1 and p.stride(1) != chroma_step:
                raise ValueError(f"YUV420Frame: {name} has samples {p.stride(1)} bytes apart, chroma_step says {chroma_step}")
        uv_pitch, v_pitch = _pitch(u, 0, chroma_step * cw), _pitch(v, 0, chroma_step * cw)
        if ch > 1 and uv_pitch != v_pitch:
            raise ValueError(f"YUV420Frame: u and v rows are {uv_pitch} and {v_pitch} bytes apart; the two chroma planes share one pitch")
        if uv_pitch < chroma_step * cw:
            raise ValueError(f"YUV420Frame: chroma pitch {uv_pitch} < chroma_step * ((w + 1) // 2) = {chroma_step * cw}")
        coef = yuv_coefficients(matrix, full_range)
        self.y, self.u, self.v = y, u, v
        self.chroma_step, self.matrix, self.full_range = int(chroma_step), matrix, bool(full_range)
        self.y_pitch, self.uv_pitch = y_pitch, uv_pitch
        self.coefficients = coef

    # ---- views of decoder output ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _surface(buffer, what: str) -> torch.Tensor:
        t = _as_tensor(buffer, what)
        if not t.is_contiguous():
            raise ValueError(f"{what}: the surface must be one contiguous buffer; got strides {t.stride()}")
        return t.reshape(-1)

    @staticmethod
    def _view(flat: torch.Tensor, what: str, shape, strides, offset: int) -> torch.Tensor:
        last = offset + sum((n - 1) * s for n, s in zip(shape, strides))
        if offset < 0 or last >= flat.numel():
            raise ValueError(f"{what}: bytes [{offset}, {last}] lie outside the surface of {flat.numel()} bytes")
        return torch.as_strided(flat, shape, strides, flat.storage_offset() + offset)

    @classmethod
    def _from_interleaved(cls, who: str, v_first: bool, buffer_or_planes, height: int, width: int, pitch, uv_offset, kw) -> "YUV420Frame":
        h, w = int(height), int(width)
        if h < 1 or w < 1:
            raise ValueError(f"{who}: frame of {h} x {w}")
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if isinstance(buffer_or_planes, (tuple, list)):  # (y [h, w], uv [ch, cw, 2]): two allocations, as some decoders export them
            if len(buffer_or_planes) != 2:
                raise ValueError(f"{who}: planes are (y, uv)")
            y, uv = _as_tensor(buffer_or_planes[0], f"{who}: y"), _as_tensor(buffer_or_planes[1], f"{who}: uv")
            if uv.dim() == 2 and uv.shape[1] == 2 * cw and uv.stride(1) == 1:
                uv = uv.unflatten(1, (cw, 2))
            if uv.dim() != 3 or tuple(uv.shape) != (ch, cw, 2):
                raise ValueError(f"{who}: the chroma plane of a {h} x {w} frame is [{ch}, {cw}, 2] (or [{ch}, {2 * cw}]); got {tuple(uv.shape)}")
            if tuple(y.shape) != (h, w):
                raise ValueError(f"{who}: y is {tuple(y.shape)}, not [{h}, {w}]")
            first, second = uv[..., 0], uv[..., 1]
        else:
            flat = cls._surface(buffer_or_planes, who)
            pitch = int(pitch) if pitch is not None else 2 * cw  # (an odd width needs w + 1 bytes per chroma row)
            if pitch < w or pitch < 2 * cw:
                raise ValueError(f"{who}: pitch {pitch} is too small for rows of {w} luma / {2 * cw} chroma bytes")
            uv_offset = int(uv_offset) if uv_offset is not None else pitch * h
            if uv_offset < pitch * (h - 1) + w:
                raise ValueError(f"{who}: uv_offset {uv_offset} lies inside the luma plane ({h} rows, {pitch} bytes apart)")
            y = cls._view(flat, who, (h, w), (pitch, 1), 0)
            first = cls._view(flat, who, (ch, cw), (pitch, 2), uv_offset)
            second = cls._view(flat, who, (ch, cw), (pitch, 2), uv_offset + 1)
        u, v = (second, first) if v_first else (first, second)
        return cls(y, u, v, chroma_step=2, **kw)

    @classmethod
    def from_nv12(cls, buffer_or_planes, height: int, width: int, pitch: Optional[int] = None, uv_offset: Optional[int] = None, **kw) -> "YUV420Frame":
        """NV12: a luma plane and ONE chroma plane of interleaved (U, V) pairs, as hardware decoders deliver it.  ``buffer_or_planes``: the whole surface as one
        contiguous uint8 buffer -- rows ``pitch`` bytes apart (default: the width, rounded up to even), the chroma plane at byte ``uv_offset`` (default
        ``pitch * height``; decoders that align the luma height put it at ``pitch * aligned_height``) -- or a pair (y [h, w], uv [ch, cw, 2]).  Views, no copy
        (NumPy: one upload of the surface).  ``**kw``: matrix, full_range."""
        return cls._from_interleaved("from_nv12", False, buffer_or_planes, height, width, pitch, uv_offset, kw)

    @classmethod
    def from_nv21(cls, buffer_or_planes, height: int, width: int, pitch: Optional[int] = None, uv_offset: Optional[int] = None, **kw) -> "YUV420Frame":
        """NV21: as ``from_nv12`` with (V, U) pairs."""
        return cls._from_interleaved("from_nv21", True, buffer_or_planes, height, width, pitch, uv_offset, kw)

    @classmethod
    def from_i420(cls, buffer_or_planes, height: int, width: int, pitch: Optional[int] = None, uv_offset: Optional[int] = None, **kw) -> "YUV420Frame":
        """Planar I420: luma, then the U plane, then the V plane.  ``buffer_or_planes``: one contiguous uint8 buffer -- luma rows ``pitch`` bytes apart (default: the
        width, rounded up to even), chroma rows ``pitch // 2``, the U plane at byte ``uv_offset`` (default ``pitch * height``) and the V plane right behind its
        ``(height + 1) // 2`` rows -- or a triple (y, u, v) of planes, named by meaning, not by their order in memory (YV12 stores V first: pass its
        second chroma plane as u).  Views, no copy."""
        who = "from_i420"
        h, w = int(height), int(width)
        if h < 1 or w < 1:
            raise ValueError(f"{who}: frame of {h} x {w}")
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if isinstance(buffer_or_planes, (tuple, list)):
            if len(buffer_or_planes) != 3:
                raise ValueError(f"{who}: planes are (y, u, v)")
            y, u, v = buffer_or_planes
            if tuple(getattr(y, "shape", ())) != (h, w):
                raise ValueError(f"{who}: y is {tuple(getattr(y, 'shape', ()))}, not [{h}, {w}]")
            return cls(y, u, v, chroma_step=1, **kw)
        flat = cls._surface(buffer_or_planes, who)
        pitch = int(pitch) if pitch is not None else 2 * cw
        if pitch < w or pitch // 2 < cw:
            raise ValueError(f"{who}: pitch {pitch} is too small for rows of {w} luma / {cw} chroma bytes at pitch // 2")
        uv_offset = int(uv_offset) if uv_offset is not None else pitch * h
        if uv_offset < pitch * (h - 1) + w:
            raise ValueError(f"{who}: uv_offset {uv_offset} lies inside the luma plane ({h} rows, {pitch} bytes apart)")
        cp = pitch // 2
        y = cls._view(flat, who, (h, w), (pitch, 1), 0)
        u = cls._view(flat, who, (ch, cw), (cp, 1), uv_offset)
        v = cls._view(flat, who, (ch, cw), (cp, 1), uv_offset + cp * ch)
        return cls(y, u, v, chroma_step=1, **kw)

    # ---------------------------------------------------------------------------------------------------------------------------------------
    @property
    def shape(self) -> Tuple[int, int, int]:
        """(h, w, 3): the shape of the RGB image this frame stands for."""
        return (int(self.y.shape[0]), int(self.y.shape[1]), 3)

    @property
    def device(self) -> torch.device:
        return self.y.device

    @property
    def planes(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.y, self.u, self.v

    def to_rgb(self) -> torch.Tensor:
        """uint8 [h, w, 3] on the frame's device: every pixel by the rule of include/vgh.h, in int32 torch ops (exactly what the library's letterbox fetches)."""
        h, w, _ = self.shape
        y_offset, cy, crv, cgu, cgv, cbu = self.coefficients
        c = self.y.to(torch.int32) - y_offset
        up = lambda p: (p.to(torch.int32) - 128).repeat_interleave(2, dim=0)[:h].repeat_interleave(2, dim=1)[:, :w]  # noqa: E731  (y >> 1, x >> 1)
        d, e = up(self.u), up(self.v)
        luma = cy * c + 32768
        rgb = torch.stack([luma + crv * e, luma + cgu * d + cgv * e, luma + cbu * d], dim=-1)
        return torch.bitwise_right_shift(rgb, 16).clamp_(0, 255).to(torch.uint8)

    def __repr__(self) -> str:
        h, w, _ = self.shape
        return f"YUV420Frame({h} x {w}, chroma_step={self.chroma_step}, {self.matrix}, {'full' if self.full_range else 'limited'} range, {self.device})"


def frame_rgb(frame: YUV420Frame, rgb: str = "host") -> Union[np.ndarray, torch.Tensor]:
    """The ``original_image`` of a result whose input was a frame: ``to_rgb()`` on the host (NumPy, the default, like any other call) or kept on the device."""
    if rgb not in ("host", "device"):
        raise ValueError(f"rgb={rgb!r}: 'host' (a NumPy original_image) or 'device' (a GPU tensor)")
    out = frame.to_rgb()
    return out if rgb == "device" else out.cpu().numpy()
