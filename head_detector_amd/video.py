"""Video frames as decoders deliver them: 8-bit YUV 4:2:0 (NV12 / NV21 surfaces of a hardware decoder, planar I420 of a software one) straight into the detector.

    frame = YUV420Frame.from_nv12(surface, height, width, pitch=surface_pitch, uv_offset=aligned_height * surface_pitch)   # views of the surface, no copy
    predictions = detector(frame)                 # or detector.detect_batch(frames), tracker.update(frame), engine.detect(frames)

The library converts every tap to RGB while it letterboxes (VGH_IMG_YUV420_RAW, csrc/letterbox.hip): no RGB copy of the frame is written.  The conversion is the
integer rule stated in include/vgh.h (vgh_yuv420_image) -- nearest chroma sample, 16.16 fixed-point coefficients, every pixel clamped to bytes:

    c = Y - y_offset, d = U - 128, e = V - 128
    R = clamp8((cy*c + crv*e + 32768) >> 16),  G = clamp8((cy*c + cgu*d + cgv*e + 32768) >> 16),  B = clamp8((cy*c + cbu*d + 32768) >> 16)

``YUV420Frame.to_rgb()`` is that rule in torch integer ops (CPU or GPU tensors); the detector's result is defined as "``to_rgb()``, then what an RGB image gets".
PARITY UNPINNED against cv2.cvtColor (cv2 rounds its coefficients to another fixed-point precision): ``tools/first_contact.py --cv2`` reports the difference.

10- and 12-bit frames (HEVC Main10, AV1 10-bit: P010 / P012 / P016 surfaces, yuv420p10le planes) go in the same way as a ``YUV420Frame16``:

    frame = YUV420Frame16.from_p010(surface, height, width, pitch=surface_pitch, uv_offset=aligned_height * surface_pitch)   # or from_i010; views, no copy
    predictions = detector(frame)                 # VGH_IMG_YUV420P16_RAW: sample = (word >> shift) & (2^D - 1), the same rule with 2^(D+8) coefficients, RGB BYTES out

Everything behind the fetch is the 8-bit path; ``to_8bit()`` narrows a deep frame for ``anonymize_frame``, the overlay and the head tensors, which work in 8-bit planes.

Out again, to an encoder (include/vgh_video.h, libvghvideo.so; restated in tests/yuv_anonymize_ref.py and equal to it bit for bit):

    anonymize_frame(frame, heads, out=frame)      # every head hidden in the frame's own luma and chroma planes, in place: no RGB image is made
    YUV420Frame.from_rgb(image, "nv12")           # what draw(), render_mesh() and anonymize() return, packed to YUV 4:2:0

Every plane is a one-channel image under the rule of ``anonymize``: the luma plane with the head's box, ellipse or mesh region; a chroma sample belongs to the
latest head that owns any of the (up to) four luma pixels it colours, and is changed inside the chroma box (x0 >> 1, y0 >> 1, (x1 + 1) >> 1, (y1 + 1) >> 1)
with the cell side and the blur radius worked out from that box by the same formulas.  Limits: 8-bit 4:2:0 only; the luma and the chroma grid of "pixelate" are
independent, so the edges of their cells may differ by a sample.  The packer, integer like ``to_rgb``:

    Y = clamp8(y_offset + ((kyr R + kyg G + kyb B + 32768) >> 16))
    U = clamp8(128 + ((kur Rm + kug Gm + kub Bm + 32768) >> 16)),  V likewise;  (Rm, Gm, Bm) the rounded mean (2 S + m) / (2 m) of the 2 x 2 block's in-image pixels

PARITY of the packer UNPINNED against cv2.cvtColor as well (``tools/first_contact.py --cv2``).
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np
import torch

# (Kr, Kb) of the luma equation Y = Kr R + Kg G + Kb B, Kg = 1 - Kr - Kb
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def yuv_coefficients(matrix: str = "bt709", full_range: bool = False, bit_depth: int = 8) -> Tuple[int, int, int, int, int, int]:
    """-> (y_offset, cy, crv, cgu, cgv, cbu): the fixed-point coefficients (* 2^16) of vgh_yuv420_image, rounded (``round``: half to even; no value is a tie) from
    the float64 (Kr, Kb) definition of ``matrix``, Kg = 1 - Kr - Kb:

        limited range: y_offset = 16, sy = 255 / 219, sc = 255 / 224        full range: y_offset = 0, sy = sc = 1
        cy  = round(65536 * sy)
        crv = round(65536 * sc * 2 (1 - Kr))                  R = sy (Y - y_offset) + sc 2 (1 - Kr) (V - 128)
        cbu = round(65536 * sc * 2 (1 - Kb))                  B = sy (Y - y_offset) + sc 2 (1 - Kb) (U - 128)
        cgu = round(65536 * sc * -2 Kb (1 - Kb) / Kg)         G = (Y - Kr R - Kb B) / Kg
        cgv = round(65536 * sc * -2 Kr (1 - Kr) / Kg)

    ``bit_depth`` D = 10 or 12: the coefficients (* 2^(D+8)) of vgh_yuv420p16_image, which take D-bit samples to 8-bit RGB -- the same expressions with
    65536 -> 2^(D+8), 128 -> 2^(D-1) and, with k = 2^(D-8):

        limited range: y_offset = 16 k, sy = 255 / (219 k), sc = 255 / (224 k)        full range: y_offset = 0, sy = sc = 255 / (2^D - 1)

    (a power of two scales a float64 exactly, so the limited-range integers are those of 8 bits; the full-range ones are not: 255 / 1023 is not 1 / 4)."""
    if matrix not in MATRICES:
        raise ValueError(f"yuv_coefficients: matrix {matrix!r} is not one of {sorted(MATRICES)}")
    if bit_depth not in (8, 10, 12):
        raise ValueError(f"yuv_coefficients: bit_depth {bit_depth!r} is not 8, 10 or 12")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    k = float(1 << (bit_depth - 8))
    sy, sc = (255.0 / ((1 << bit_depth) - 1),) * 2 if full_range else (255.0 / (219.0 * k), 255.0 / (224.0 * k))  # (8 bits, full range: 255 / 255 = 1.0)
    one = float(1 << (bit_depth + 8))
    q = lambda v: int(round(one * v))  # noqa: E731
    return (0 if full_range else 16 << (bit_depth - 8), q(sy), q(sc * 2.0 * (1.0 - kr)), q(sc * -2.0 * kb * (1.0 - kb) / kg), q(sc * -2.0 * kr * (1.0 - kr) / kg),
            q(sc * 2.0 * (1.0 - kb)))


def rgb_to_yuv_coefficients(matrix: str = "bt709", full_range: bool = False) -> Tuple[int, ...]:
    """-> (y_offset, kyr, kyg, kyb, kur, kug, kub, kvr, kvg, kvb): the fixed-point coefficients (* 2^16) of vghy_pack_rgb, from the same float64 (Kr, Kb) table as
    ``yuv_coefficients``; sy = 219 / 255 and sc = 224 / 255 for limited range, both 1 for full range:

        kyr = round(65536 sy Kr), kyb = round(65536 sy Kb), kyg = round(65536 sy) - kyr - kyb                  the luma row sums to round(65536 sy)
        kub = kvr = round(65536 sc / 2)
        kur = round(65536 sc * -Kr / (2 (1 - Kb))), kug = -(kur + kub)                                          the chroma rows sum to exactly 0:
        kvb = round(65536 sc * -Kb / (2 (1 - Kr))), kvg = -(kvr + kvb)                                          every grey gives U = V = 128"""
    if matrix not in MATRICES:
        raise ValueError(f"rgb_to_yuv_coefficients: matrix {matrix!r} is not one of {sorted(MATRICES)}")
    kr, kb = MATRICES[matrix]
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    q = lambda v: int(round(65536.0 * v))  # noqa: E731
    kyr, kyb = q(sy * kr), q(sy * kb)
    kyg = q(sy) - kyr - kyb
    kub = kvr = q(sc / 2.0)
    kur = q(sc * -kr / (2.0 * (1.0 - kb)))
    kvb = q(sc * -kb / (2.0 * (1.0 - kr)))
    return (0 if full_range else 16, kyr, kyg, kyb, kur, -(kur + kub), kub, kvr, -(kvr + kvb), kvb)


def rgb_to_yuv(color, matrix: str = "bt709", full_range: bool = False) -> Tuple[int, int, int]:
    """(Y, U, V) of one RGB colour (three integers in 0 .. 255) by the packer's rule for one pixel; on the host, in Python integers."""
    c = [int(v) for v in color]
    if len(c) != 3 or any(not 0 <= v <= 255 or v != w for v, w in zip(c, color)):
        raise ValueError(f"rgb_to_yuv: color must be three integers in 0 .. 255, got {tuple(color)}")
    y_offset, *k = rgb_to_yuv_coefficients(matrix, full_range)
    clamp8 = lambda v: min(max(v, 0), 255)  # noqa: E731
    dot = lambda at: (k[at] * c[0] + k[at + 1] * c[1] + k[at + 2] * c[2] + 32768) >> 16  # noqa: E731
    return clamp8(y_offset + dot(0)), clamp8(128 + dot(3)), clamp8(128 + dot(6))


LAYOUTS = ("nv12", "nv21", "i420")


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

    @classmethod
    def empty(cls, height: int, width: int, layout: str = "nv12", device=None, **kw) -> "YUV420Frame":
        """A new dense frame of uninitialised bytes: one surface with rows ``2 * ((width + 1) // 2)`` bytes apart, viewed as ``layout`` ("nv12", "nv21" or
        "i420").  ``device``: a GPU (default: the current one).  ``**kw``: matrix, full_range."""
        if layout not in LAYOUTS:
            raise ValueError(f"YUV420Frame.empty: layout must be one of {LAYOUTS}, got {layout!r}")
        h, w = int(height), int(width)
        if h < 1 or w < 1:
            raise ValueError(f"YUV420Frame.empty: frame of {h} x {w}")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        pitch = 2 * ((w + 1) // 2)
        surface = torch.empty(pitch * h + pitch * ((h + 1) // 2), dtype=torch.uint8, device=device)
        return {"nv12": cls.from_nv12, "nv21": cls.from_nv21, "i420": cls.from_i420}[layout](surface, h, w, **kw)

    @classmethod
    def from_rgb(cls, image, layout: str = "nv12", matrix: str = "bt709", full_range: bool = False, out: Optional["YUV420Frame"] = None) -> "YUV420Frame":
        """The frame of an RGB image (csrc/yuv_pack.hip, libvghvideo.so): what ``draw()``, ``render_mesh()`` and ``anonymize()`` return, ready for an encoder.
        ``image``: uint8 [H, W, 3], a NumPy array (uploaded once) or a GPU tensor with pixels 3 bytes apart (rows may be pitched); never modified.  Luma per
        pixel, chroma from the rounded mean of each 2 x 2 block's in-image pixels, by the integer rule the module text states with
        ``rgb_to_yuv_coefficients(matrix, full_range)``.  ``out``: a frame of the same size on the same device to write into (its own layout, matrix and range
        are used; it must not overlap the image); otherwise a new dense ``layout`` frame.  There is no CPU path."""
        from . import _lib_video
        from .aligned import _device_image

        if out is None and layout not in LAYOUTS:
            raise ValueError(f"from_rgb: layout must be one of {LAYOUTS}, got {layout!r}")
        if out is not None:
            if not isinstance(out, YUV420Frame):
                raise ValueError(f"from_rgb: out must be a YUV420Frame, got {type(out).__name__}")
            matrix, full_range = out.matrix, out.full_range
        coef = rgb_to_yuv_coefficients(matrix, full_range)
        lib = _lib_video.load()
        src = _device_image(image, "packed frames")
        H, W = int(src.shape[0]), int(src.shape[1])
        if out is None:
            out = cls.empty(H, W, layout, src.device, matrix=matrix, full_range=full_range)
        elif out.shape != (H, W, 3) or out.device != src.device:
            raise ValueError(f"from_rgb: out is {out!r}; the image is {H} x {W} on {src.device}")
        job = _lib_video.PackJob()
        job.src_dev, job.src_pitch_bytes, job.height, job.width = src.data_ptr(), (src.stride(0) if H > 1 else 3 * W), H, W
        for k, (plane, pitch, step) in enumerate(out._layout()):
            job.planes[k].dst_dev, job.planes[k].dst_pitch, job.planes[k].dst_step = plane.data_ptr(), pitch, step
        job.y_offset = coef[0]
        for k in range(9):
            job.coef[k] = coef[1 + k]
        with torch.cuda.device(src.device):
            _lib_video.check(lib.vghy_pack_rgb(job, torch.cuda.current_stream().cuda_stream))
        return out

    def _layout(self):
        """((plane, pitch in bytes, step in bytes) for y, u, v) as include/vgh_video.h describes a plane."""
        return ((self.y, self.y_pitch, 1), (self.u, self.uv_pitch, self.chroma_step), (self.v, self.uv_pitch, self.chroma_step))

    def _like(self) -> "YUV420Frame":
        """A new dense frame of this frame's size, layout, matrix and range."""
        h, w, _ = self.shape
        layout = "i420" if self.chroma_step == 1 else "nv12" if self.v.data_ptr() > self.u.data_ptr() else "nv21"
        return YUV420Frame.empty(h, w, layout, self.device, matrix=self.matrix, full_range=self.full_range)

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


_WORDS = tuple(getattr(torch, n) for n in ("int16", "uint16") if hasattr(torch, n))


def _as_words(a, what: str, surface: bool = False) -> torch.Tensor:
    """A tensor of 16-bit words as it is (CPU or GPU, int16 or uint16); a NumPy array of them uploaded once to the current GPU.  ``surface``: bytes will do as well."""
    ok = "uint8, int16 or uint16" if surface else "int16 or uint16"
    if isinstance(a, np.ndarray):
        if a.dtype not in ((np.int16, np.uint16, np.uint8) if surface else (np.int16, np.uint16)):
            raise ValueError(f"{what}: expected {ok}; got {a.dtype}")
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(a, torch.Tensor) or a.dtype not in (_WORDS + ((torch.uint8,) if surface else ())):
        raise ValueError(f"{what}: expected a tensor or array of {ok}; got {getattr(a, 'dtype', type(a))}")
    return a


class YUV420Frame16:
    """One 10- or 12-bit YUV 4:2:0 frame in 16-bit words, as HEVC Main10 / AV1 10-bit decoders deliver it (P010 / P012 / P016 surfaces, I010 = yuv420p10le planes):
    ``y`` [h, w] (rows may be pitched: strides (pitch, 1)), ``u`` and ``v`` [(h+1)//2, (w+1)//2] with strides (uv_pitch, chroma_step), all counted in ELEMENTS
    (16-bit words) -- chroma_step 1 for planar planes, 2 for the two interleaved views of a P010 chroma plane.  The planes are ``torch.int16`` or ``torch.uint16``
    tensors, kept as given (views are not copied) and read as unsigned little-endian words either way; all three on one device.  NumPy ``uint16`` planes are
    uploaded once to the current GPU (planar only, see ``from_p010``).  A sample is ``(word >> shift) & (2^bit_depth - 1)``: ``shift = 16 - bit_depth`` for the
    MSB-aligned words of a hardware decoder, 0 for LSB-aligned ones; whatever lies in a word's other bits is never looked at.  ``matrix`` / ``full_range`` choose
    the coefficients (``yuv_coefficients(matrix, full_range, bit_depth)``).

    The detector takes it wherever it takes a ``YUV420Frame`` (VGH_IMG_YUV420P16_RAW: every tap converted to RGB BYTES inside the device letterbox by the rule of
    include/vgh.h, vgh_yuv420p16_image; ``to_rgb()`` is that rule in torch integer ops).  It is deliberately not a ``YUV420Frame``: ``anonymize_frame``, the overlay
    and the head tensors work in 8-bit planes, and ``to_8bit()`` is the bridge to them.  Writing into deep planes, crops from them, 4:2:2 / 4:4:4, big-endian words,
    16 significant bits, chroma interpolation and HDR tone mapping are not built: a PQ / HLG frame is converted by its matrix only."""

    def __init__(self, y, u, v, *, chroma_step: int, bit_depth: int = 10, shift: int = 0, matrix: str = "bt709", full_range: bool = False):
        who = "YUV420Frame16"
        if chroma_step not in (1, 2):
            raise ValueError(f"{who}: chroma_step {chroma_step} (in 16-bit elements: 1 = planar, 2 = interleaved)")
        if bit_depth not in (10, 12):
            raise ValueError(f"{who}: bit_depth {bit_depth!r} (10 or 12)")
        if not isinstance(shift, (int, np.integer)) or isinstance(shift, bool) or not 0 <= shift <= 16 - bit_depth:
            raise ValueError(f"{who}: shift {shift!r} outside 0 .. 16 - bit_depth = {16 - bit_depth}")
        if chroma_step == 2 and any(isinstance(p, np.ndarray) for p in (u, v)):
            raise ValueError(f"{who}: interleaved NumPy chroma views would be uploaded as two buffers; use from_p010 with the whole surface")
        y, u, v = _as_words(y, f"{who}: y"), _as_words(u, f"{who}: u"), _as_words(v, f"{who}: v")
        if y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1:
            raise ValueError(f"{who}: y must be [h, w] with h, w >= 1; got {tuple(y.shape)}")
        h, w = int(y.shape[0]), int(y.shape[1])
        ch, cw = (h + 1) // 2, (w + 1) // 2
        if tuple(u.shape) != (ch, cw) or tuple(v.shape) != (ch, cw):
            raise ValueError(f"{who}: a {h} x {w} frame has chroma planes [{ch}, {cw}]; got u {tuple(u.shape)}, v {tuple(v.shape)}")
        if not (y.device == u.device == v.device):
            raise ValueError(f"{who}: planes on different devices: {y.device}, {u.device}, {v.device}")
        if w > 1 and y.stride(1) != 1:
            raise ValueError(f"{who}: the luma samples of a row must be dense (strides (pitch, 1)); got {y.stride()}")
        y_pitch = _pitch(y, 0, w)
        if y_pitch < w:
            raise ValueError(f"{who}: luma pitch {y_pitch} < width {w}")
        for name, p in (("u", u), ("v", v)):
            if cw > 1 and p.stride(1) != chroma_step:
                raise ValueError(f"{who}: {name} has samples {p.stride(1)} elements apart, chroma_step says {chroma_step}")
        uv_pitch, v_pitch = _pitch(u, 0, chroma_step * cw), _pitch(v, 0, chroma_step * cw)
        if ch > 1 and uv_pitch != v_pitch:
            raise ValueError(f"{who}: u and v rows are {uv_pitch} and {v_pitch} elements apart; the two chroma planes share one pitch")
        if uv_pitch < chroma_step * cw:
            raise ValueError(f"{who}: chroma pitch {uv_pitch} < chroma_step * ((w + 1) // 2) = {chroma_step * cw}")
        coef = yuv_coefficients(matrix, full_range, bit_depth)
        self.y, self.u, self.v = y, u, v
        self._words = tuple(p if p.dtype == torch.int16 else p.view(torch.int16) for p in (y, u, v))  # torch has no shift for uint16: the same memory as int16
        self.chroma_step, self.bit_depth, self.shift = int(chroma_step), int(bit_depth), int(shift)
        self.matrix, self.full_range = matrix, bool(full_range)
        self.y_pitch, self.uv_pitch = y_pitch, uv_pitch  # in elements, like the strides
        self.coefficients = coef

    # ---- views of decoder output ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _surface(buffer, who: str) -> torch.Tensor:
        """The surface as one flat int16 view of the buffer (uint8 buffers: an even number of bytes from an even address)."""
        t = _as_words(buffer, who, surface=True)
        if not t.is_contiguous():
            raise ValueError(f"{who}: the surface must be one contiguous buffer; got strides {t.stride()}")
        t = t.reshape(-1)
        if t.dtype == torch.uint8:
            if t.storage_offset() % 2 or (t.device.type != "meta" and t.numel() and t.data_ptr() % 2):
                raise ValueError(f"{who}: the surface starts at an odd byte; 16-bit words need an even address")
            t = t[:t.numel() & ~1]
        return t if t.dtype == torch.int16 else t.view(torch.int16)

    @staticmethod
    def _view(flat: torch.Tensor, who: str, shape, strides, offset: int) -> torch.Tensor:
        last = offset + sum((n - 1) * s for n, s in zip(shape, strides))
        if offset < 0 or last >= flat.numel():
            raise ValueError(f"{who}: bytes [{2 * offset}, {2 * last + 1}] lie outside the surface of {2 * flat.numel()} bytes")
        return torch.as_strided(flat, shape, strides, flat.storage_offset() + offset)

    @staticmethod
    def _geometry(who: str, height, width, pitch, uv_offset, unit: int):
        """-> (h, w, ch, cw, pitch, uv_offset), the last two in BYTES and checked: ``pitch`` a multiple of ``unit``, the chroma behind the luma plane."""
        h, w = int(height), int(width)
        if h < 1 or w < 1:
            raise ValueError(f"{who}: frame of {h} x {w}")
        ch, cw = (h + 1) // 2, (w + 1) // 2
        pitch = int(pitch) if pitch is not None else 4 * cw  # (an odd width needs w + 1 words per chroma row)
        if pitch % unit or pitch < 2 * w or pitch < 4 * cw:
            raise ValueError(f"{who}: pitch {pitch} bytes must be a multiple of {unit} and hold rows of {2 * w} luma / {4 * cw} chroma bytes")
        uv_offset = int(uv_offset) if uv_offset is not None else pitch * h
        if uv_offset % 2 or uv_offset < pitch * (h - 1) + 2 * w:
            raise ValueError(f"{who}: uv_offset {uv_offset} is odd or lies inside the luma plane ({h} rows, {pitch} bytes apart)")
        return h, w, ch, cw, pitch, uv_offset

    @classmethod
    def from_p010(cls, buffer_or_planes, height: int, width: int, pitch: Optional[int] = None, uv_offset: Optional[int] = None, bit_depth: int = 10, **kw) -> "YUV420Frame16":
        """P010: a luma plane and ONE chroma plane of interleaved (U, V) pairs of 16-bit words with the sample in the TOP bits (``shift = 16 - bit_depth``), as
        hardware decoders deliver HEVC Main10 / AV1 10-bit; ``bit_depth=12`` reads a P012 / P016 surface at its top 12 bits.  ``buffer_or_planes``: the whole surface
        as one contiguous buffer (uint8, int16 or uint16) -- rows ``pitch`` BYTES apart (default: 4 * ((width + 1) // 2)), the chroma plane at BYTE ``uv_offset``
        (default ``pitch * height``) -- or a pair (y [h, w], uv [ch, cw, 2]) of 16-bit planes.  Views, no copy (NumPy: one upload).  ``**kw``: matrix, full_range."""
        who = "from_p010"
        if bit_depth not in (10, 12):
            raise ValueError(f"{who}: bit_depth {bit_depth!r} (10 or 12)")
        kw = dict(kw, bit_depth=bit_depth, shift=16 - bit_depth)
        if isinstance(buffer_or_planes, (tuple, list)):
            h, w = int(height), int(width)
            if h < 1 or w < 1:
                raise ValueError(f"{who}: frame of {h} x {w}")
            ch, cw = (h + 1) // 2, (w + 1) // 2
            if len(buffer_or_planes) != 2:
                raise ValueError(f"{who}: planes are (y, uv)")
            y, uv = _as_words(buffer_or_planes[0], f"{who}: y"), _as_words(buffer_or_planes[1], f"{who}: uv")
            if uv.dim() == 2 and uv.shape[1] == 2 * cw and uv.stride(1) == 1:
                uv = uv.unflatten(1, (cw, 2))
            if uv.dim() != 3 or tuple(uv.shape) != (ch, cw, 2):
                raise ValueError(f"{who}: the chroma plane of a {h} x {w} frame is [{ch}, {cw}, 2] (or [{ch}, {2 * cw}]); got {tuple(uv.shape)}")
            if tuple(y.shape) != (h, w):
                raise ValueError(f"{who}: y is {tuple(y.shape)}, not [{h}, {w}]")
            return cls(y, uv[..., 0], uv[..., 1], chroma_step=2, **kw)
        h, w, ch, cw, pitch, uv_offset = cls._geometry(who, height, width, pitch, uv_offset, 2)
        flat = cls._surface(buffer_or_planes, who)
        y = cls._view(flat, who, (h, w), (pitch // 2, 1), 0)
        u = cls._view(flat, who, (ch, cw), (pitch // 2, 2), uv_offset // 2)
        v = cls._view(flat, who, (ch, cw), (pitch // 2, 2), uv_offset // 2 + 1)
        return cls(y, u, v, chroma_step=2, **kw)

    @classmethod
    def from_i010(cls, buffer_or_planes, height: int, width: int, pitch: Optional[int] = None, uv_offset: Optional[int] = None, bit_depth: int = 10, **kw) -> "YUV420Frame16":
        """Planar I010 (``yuv420p10le``; ``bit_depth=12``: ``yuv420p12le``): luma, then the U plane, then the V plane, 16-bit words with the sample in the LOW bits
        (``shift = 0``), as software decoders deliver it.  ``buffer_or_planes``: one contiguous buffer (uint8, int16 or uint16) -- luma rows ``pitch`` BYTES apart (a
        multiple of 4; default 4 * ((width + 1) // 2)), chroma rows ``pitch // 2``, the U plane at BYTE ``uv_offset`` (default ``pitch * height``) and the V plane
        right behind its ``(height + 1) // 2`` rows -- or a triple (y, u, v) of 16-bit planes.  Views, no copy."""
        who = "from_i010"
        if bit_depth not in (10, 12):
            raise ValueError(f"{who}: bit_depth {bit_depth!r} (10 or 12)")
        kw = dict(kw, bit_depth=bit_depth, shift=0)
        if isinstance(buffer_or_planes, (tuple, list)):
            if len(buffer_or_planes) != 3:
                raise ValueError(f"{who}: planes are (y, u, v)")
            y, u, v = buffer_or_planes
            if tuple(getattr(y, "shape", ())) != (int(height), int(width)):
                raise ValueError(f"{who}: y is {tuple(getattr(y, 'shape', ()))}, not [{int(height)}, {int(width)}]")
            return cls(y, u, v, chroma_step=1, **kw)
        h, w, ch, cw, pitch, uv_offset = cls._geometry(who, height, width, pitch, uv_offset, 4)
        flat = cls._surface(buffer_or_planes, who)
        cp = pitch // 4  # chroma rows in words
        y = cls._view(flat, who, (h, w), (pitch // 2, 1), 0)
        u = cls._view(flat, who, (ch, cw), (cp, 1), uv_offset // 2)
        v = cls._view(flat, who, (ch, cw), (cp, 1), uv_offset // 2 + cp * ch)
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

    def _samples(self):
        """The three planes as int32 samples: (word >> shift) & (2^bit_depth - 1), the words read as unsigned."""
        mask = (1 << self.bit_depth) - 1
        return tuple(torch.bitwise_right_shift(p.to(torch.int32) & 0xFFFF, self.shift) & mask for p in self._words)

    def to_rgb(self) -> torch.Tensor:
        """uint8 [h, w, 3] on the frame's device: every pixel by the rule of include/vgh.h (vgh_yuv420p16_image), in int32 torch ops (exactly what the library's
        letterbox fetches)."""
        h, w, _ = self.shape
        D = self.bit_depth
        y_offset, cy, crv, cgu, cgv, cbu = self.coefficients
        ys, us, vs = self._samples()
        up = lambda p: (p - (1 << (D - 1))).repeat_interleave(2, dim=0)[:h].repeat_interleave(2, dim=1)[:, :w]  # noqa: E731  (y >> 1, x >> 1)
        d, e = up(us), up(vs)
        luma = cy * (ys - y_offset) + (1 << (D + 7))
        rgb = torch.stack([luma + crv * e, luma + cgu * d + cgv * e, luma + cbu * d], dim=-1)
        return torch.bitwise_right_shift(rgb, D + 8).clamp_(0, 255).to(torch.uint8)

    def to_8bit(self, layout: Optional[str] = None, out: Optional[YUV420Frame] = None) -> YUV420Frame:
        """The frame narrowed to 8 bits per sample, a ``YUV420Frame`` with this frame's matrix and range: every sample s becomes
        ``min(255, (s + 2^(D-9)) >> (D-8))``.  The bridge to ``anonymize_frame``, ``draw_overlay`` and ``get_head_tensors``, which work in 8-bit planes.  A new dense
        ``layout`` frame ("nv12" for interleaved chroma, "i420" for planar, unless given), or ``out``: a ``YUV420Frame`` of the same size on the same device (its own
        layout is kept, its matrix and range must be this frame's).  Several torch passes over the frame, not a tuned kernel.  In limited range the code values
        scale by 2^(D-8) exactly, so this is the matching 8-bit frame up to rounding; in FULL range (white = 2^D - 1, not 255 * 2^(D-8)) it is a rounded shift, not a
        range-exact rescale.  The detector's result on the 8-bit frame is not that on the deep frame."""
        h, w, _ = self.shape
        if out is None:
            layout = layout if layout is not None else "nv12" if self.chroma_step == 2 else "i420"
            if layout not in LAYOUTS:
                raise ValueError(f"to_8bit: layout must be one of {LAYOUTS}, got {layout!r}")
            out = YUV420Frame.empty(h, w, layout, self.device, matrix=self.matrix, full_range=self.full_range)
        elif not (isinstance(out, YUV420Frame) and out.shape == self.shape and out.device == self.device):
            raise ValueError(f"to_8bit: out must be a YUV420Frame of {h} x {w} on {self.device}; got {out!r}")
        elif (out.matrix, out.full_range) != (self.matrix, self.full_range):
            raise ValueError(f"to_8bit: out is {out!r}; the frame is {self.matrix}, {'full' if self.full_range else 'limited'} range")
        D = self.bit_depth
        for dst, s in zip(out.planes, self._samples()):
            dst.copy_(torch.bitwise_right_shift(s + (1 << (D - 9)), D - 8).clamp_(max=255))
        return out

    def __repr__(self) -> str:
        h, w, _ = self.shape
        return (f"YUV420Frame16({h} x {w}, {self.bit_depth} bits >> {self.shift}, chroma_step={self.chroma_step}, {self.matrix}, "
                f"{'full' if self.full_range else 'limited'} range, {self.device})")


FRAME_TYPES = (YUV420Frame, YUV420Frame16)  # what the detector's and the tracker's entry points take as a video frame


def require_8bit_frame(who: str, frame) -> None:
    """The refusal of the consumers that work in 8-bit planes, for a result whose ``source_frame`` is a deep frame."""
    if isinstance(frame, YUV420Frame16):
        raise ValueError(f"{who}: the source_frame is a {frame.bit_depth}-bit YUV420Frame16 and {who} works in 8-bit planes; narrow it with source_frame.to_8bit() and pass "
                         "that frame (video.anonymize_frame, overlay.draw_heads, head_tensors.head_tensors)")


def frame_rgb(frame: Union[YUV420Frame, YUV420Frame16], rgb: str = "host") -> Union[np.ndarray, torch.Tensor, None]:
    """The ``original_image`` of a result whose input was a frame: ``to_rgb()`` on the host (NumPy, the default, like any other call) or kept on the device; with
    ``rgb="none"`` no RGB copy is made at all (None): the result keeps its ``source_frame``, which ``anonymize_frame`` works on."""
    if rgb not in ("host", "device", "none"):
        raise ValueError(f"rgb={rgb!r}: 'host' (a NumPy original_image), 'device' (a GPU tensor) or 'none' (no RGB copy: video loops that use source_frame alone)")
    if rgb == "none":
        return None
    out = frame.to_rgb()
    return out if rgb == "device" else out.cpu().numpy()


def chroma_box(box) -> Tuple[int, int, int, int]:
    """The chroma box of a luma geometry box (x0, y0, x1, y1): (x0 >> 1, y0 >> 1, (x1 + 1) >> 1, (y1 + 1) >> 1), arithmetic shifts -- it contains every chroma
    sample of every luma pixel of the box.  A luma box with a zero side gets an empty chroma box."""
    x0, y0, x1, y1 = (int(v) for v in box)
    if x1 <= x0 or y1 <= y0:
        return (x0 >> 1, y0 >> 1, x0 >> 1, y0 >> 1)
    return (x0 >> 1, y0 >> 1, (x1 + 1) >> 1, (y1 + 1) >> 1)


def _plane_range(t: torch.Tensor) -> Tuple[int, int]:
    last = sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + last + 1


def _plane_pairs(who: str, frame: YUV420Frame, out: Optional[YUV420Frame]):
    """-> (out, rows): the frame a call of ``who`` writes (``out``, checked: a frame of ``frame``'s size on its device; ``None``: a new dense frame like ``frame``) and
    its planes as include/vgh_video.h and include/vgh_osd.h describe one, (src pointer, dst pointer, src pitch, dst pitch, src step, dst step) each.  A plane of
    ``out`` is exactly its plane of ``frame`` (in place) or overlaps no plane of ``frame``.  A frame that is not on a GPU: (out as given, None), for the caller's refusal."""
    H, W, _ = frame.shape
    if out is not None and not (isinstance(out, YUV420Frame) and out.shape == frame.shape and out.device == frame.device):
        raise ValueError(f"{who}: out must be a YUV420Frame of {H} x {W} on {frame.device}; got {out!r}")
    if not frame.y.is_cuda:
        return out, None
    if out is None:
        out = frame._like()
    rows = []
    for name, (s, sp, ss), (d, dp, ds) in zip("yuv", frame._layout(), out._layout()):
        if not (d.data_ptr() == s.data_ptr() and dp == sp and ds == ss):  # not in place
            d0, d1 = _plane_range(d)
            for other in frame.planes:
                s0, s1 = _plane_range(other)
                if s0 < d1 and d0 < s1:
                    raise ValueError(f"{who}: plane {name} of out overlaps the source frame without being exactly its plane {name} (same memory, pitch and step): "
                                     "pass out=frame for in place, or a frame elsewhere")
        rows.append((s.data_ptr(), d.data_ptr(), sp, dp, ss, ds))
    return out, rows


def anonymize_frame(frame: YUV420Frame, heads, method: str = "pixelate", region: str = "ellipse", *, margin: float = 0.1, cells: int = 8, strength: float = 0.1,
                    color=(0, 0, 0), faces=None, owner=None, out: Optional[YUV420Frame] = None) -> YUV420Frame:
    """``frame`` with every head hidden directly in its luma and chroma planes (csrc/yuv_anonymize.hip, libvghvideo.so; the module text and include/vgh_video.h
    state the rule): no RGB image is made.  The arguments and their checks are those of ``anonymize.anonymize_heads``; ``color`` is RGB and converted by
    ``rgb_to_yuv(color, frame.matrix, frame.full_range)``; ``region="mesh"`` (needs ``faces``) and ``owner=`` (int32 [H, W]) give the LUMA owner map.
    ``out=None``: a new dense frame of the source's layout, matrix and range.  ``out=frame`` (or any frame whose three planes are the same memory with the same
    pitch and step): IN PLACE -- only the samples of the heads are written, nothing is copied, and apart from clearing the owner map the work scales with the heads'
    boxes, not with the frame.  Any other frame of the same size on the same device is written whole and must not overlap the source; its layout may differ
    (NV12 in, I420 out).  Returns the frame written.  There is no CPU path for the samples."""
    from . import _lib_video, anonymize as an
    from ._lib import VghError
    from .mesh_geometry import require_faces

    an._check_choice(method, region)
    if region == "mesh":
        require_faces(faces)
    rgb = an._check_color(color)
    if not isinstance(frame, YUV420Frame):
        raise ValueError(f"anonymize_frame: frame must be a YUV420Frame, got {type(frame).__name__}")
    H, W, _ = frame.shape
    y, u, v = rgb_to_yuv((rgb & 255, rgb >> 8 & 255, rgb >> 16), frame.matrix, frame.full_range)
    n = len(heads)
    tables = an.TapTables()  # one tap table for the call: the luma rows' tables first, the chroma rows' behind them
    plan = an._plan_on_host((H, W), heads, method, region, margin, cells, strength, owner, tables)
    out, planes = _plane_pairs("anonymize_frame", frame, out)
    if planes is None:
        raise VghError("anonymised frames need a GPU: the HIP kernels of libvghvideo.so are the only implementation of the samples")
    lib = _lib_video.load()
    dev = frame.device
    plan, owner_dev = an._plan_on_device(plan, dev, (H, W), heads, method, region, margin, cells, strength, faces, owner, tables)  # the silhouettes at the frame's size
    # the chroma rows: the same formulas on the chroma boxes
    luma_rows = plan.heads
    corners = zip(luma_rows["x0"].tolist(), luma_rows["y0"].tolist(), luma_rows["x1"].tolist(), luma_rows["y1"].tolist())
    chroma_rows, _ = an.plan_rows([chroma_box(b) for b in corners], method, int(cells), float(strength), tables)
    taps = tables.taps()
    job = _lib_video.AnonymizeJob()
    for p, row in zip(job.planes, planes):
        p.src_dev, p.dst_dev, p.src_pitch, p.dst_pitch, p.src_step, p.dst_step = row
    job.height, job.width, job.n_heads, job.method, job.color = H, W, n, plan.method, y | u << 8 | v << 16
    job.region = _lib_video.REGION_MAP if owner_dev is not None else _lib_video.REGION_ELLIPSE if region == "ellipse" else _lib_video.REGION_BOX
    if n:
        job.luma_heads, job.chroma_heads = luma_rows.ctypes.data, chroma_rows.ctypes.data
    if taps.size:
        job.taps, job.n_taps = taps.ctypes.data, taps.size
    if owner_dev is not None:
        job.owner_dev = owner_dev.data_ptr()
    need = int(lib.vghy_anonymize_workspace_bytes(job))
    if need <= 0:
        _lib_video.check(-1)  # raises with the library's own message
    with torch.cuda.device(dev):
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)  # allocated, used and (by the caching allocator) reused in the order of this stream
        _lib_video.check(lib.vghy_anonymize(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out
