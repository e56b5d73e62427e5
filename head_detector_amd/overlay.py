"""On-screen display: boxes, label bars and bitmap text written into the surface that goes on to an encoder or a screen -- the Y, U and V planes of a
``video.YUV420Frame`` where they lie (in place if wanted, no RGB copy of the frame), or the bytes of an RGB image (csrc/osd.hip, libvghosd.so; include/vgh_osd.h
states the rule, tests/osd_ref.py restates it in NumPy and the device equals that bit for bit).

    tracked = tracker.update(frame, rgb="none")
    tracked.draw_overlay(labels="id+score", out=frame)          # every track's box and "#7 93%" in the decoder's own surface
    items = Items().rect((10, 20, 110, 140), (255, 0, 0), 2).text(10, 4, "cam 3", (255, 255, 255), 2)
    render(frame, items, out=frame)                             # anything else: bars, boxes, text

Items are drawn in order and a later item lies over an earlier one; a sample belongs to the LATEST item that covers it (a chroma sample: that touches any of its
four luma pixels) and becomes ``(src * (256 - a) + c * a + 128) >> 8`` of the SOURCE sample -- one blend, never a blend of blends, so the picture does not depend
on scheduling.  Integer arithmetic only.  The work scales with what is drawn, not with the frame, and the number of launches does not depend on the number of
items.  Text is a fixed 5 x 7 bitmap font at an integer scale: space, 0-9, A-Z and ``# % . : - + /``; lower case is drawn as upper case and any other character
as a space.

``PredictionResult.draw()`` remains the function with the reference's look (RGB only, fixed colours, no labels).  NOT here: parity with cv2 of any kind, lines,
circles and the mesh wireframe in YUV planes, anti-aliased or proportional text, lower case, many frames in one call, 10-bit frames.  The defaults of
``head_overlay_plan`` (palette, "auto" thickness and text scale, ``coasting_alpha``) are API defaults, NOT tuned values."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

from . import _vgho
from ._lib import VghError

CHARS = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#%.:-+/"  # glyph code = index (VGHO_GLYPHS of them)

# The mirror of kFont (csrc/osd_rules.h, its single home; tests hold the two and vgho_font equal): 7 row bytes a glyph, top first, bit 0 = the left column.
FONT = (
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00), (0x0e, 0x11, 0x19, 0x15, 0x13, 0x11, 0x0e), (0x04, 0x06, 0x04, 0x04, 0x04, 0x04, 0x0e), (0x0e, 0x11, 0x10, 0x08, 0x04, 0x02, 0x1f),
    (0x0f, 0x10, 0x10, 0x0e, 0x10, 0x10, 0x0f), (0x08, 0x0c, 0x0a, 0x09, 0x1f, 0x08, 0x08), (0x1f, 0x01, 0x0f, 0x10, 0x10, 0x11, 0x0e), (0x0c, 0x02, 0x01, 0x0f, 0x11, 0x11, 0x0e),
    (0x1f, 0x10, 0x08, 0x04, 0x04, 0x02, 0x02), (0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e), (0x0e, 0x11, 0x11, 0x1e, 0x10, 0x08, 0x06), (0x04, 0x0a, 0x11, 0x11, 0x1f, 0x11, 0x11),
    (0x0f, 0x11, 0x11, 0x0f, 0x11, 0x11, 0x0f), (0x0e, 0x11, 0x01, 0x01, 0x01, 0x11, 0x0e), (0x07, 0x09, 0x11, 0x11, 0x11, 0x09, 0x07), (0x1f, 0x01, 0x01, 0x0f, 0x01, 0x01, 0x1f),
    (0x1f, 0x01, 0x01, 0x0f, 0x01, 0x01, 0x01), (0x0e, 0x11, 0x01, 0x1d, 0x11, 0x11, 0x1e), (0x11, 0x11, 0x11, 0x1f, 0x11, 0x11, 0x11), (0x0e, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0e),
    (0x1c, 0x08, 0x08, 0x08, 0x08, 0x09, 0x06), (0x11, 0x09, 0x05, 0x03, 0x05, 0x09, 0x11), (0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x1f), (0x11, 0x1b, 0x15, 0x15, 0x11, 0x11, 0x11),
    (0x11, 0x13, 0x13, 0x15, 0x19, 0x19, 0x11), (0x0e, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e), (0x0f, 0x11, 0x11, 0x0f, 0x01, 0x01, 0x01), (0x0e, 0x11, 0x11, 0x11, 0x15, 0x09, 0x16),
    (0x0f, 0x11, 0x11, 0x0f, 0x05, 0x09, 0x11), (0x1e, 0x01, 0x01, 0x0e, 0x10, 0x10, 0x0f), (0x1f, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04), (0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e),
    (0x11, 0x11, 0x11, 0x11, 0x0a, 0x0a, 0x04), (0x11, 0x11, 0x11, 0x15, 0x15, 0x1b, 0x11), (0x11, 0x11, 0x0a, 0x04, 0x0a, 0x11, 0x11), (0x11, 0x11, 0x0a, 0x04, 0x04, 0x04, 0x04),
    (0x1f, 0x10, 0x08, 0x04, 0x02, 0x01, 0x1f), (0x0a, 0x0a, 0x1f, 0x0a, 0x1f, 0x0a, 0x0a), (0x13, 0x13, 0x08, 0x04, 0x02, 0x19, 0x19), (0x00, 0x00, 0x00, 0x00, 0x00, 0x06, 0x06),
    (0x00, 0x06, 0x06, 0x00, 0x06, 0x06, 0x00), (0x00, 0x00, 0x00, 0x1f, 0x00, 0x00, 0x00), (0x00, 0x04, 0x04, 0x1f, 0x04, 0x04, 0x00), (0x10, 0x10, 0x08, 0x04, 0x02, 0x01, 0x01),
)

# "track" colours: PALETTE[id % 16].  A fixed table, an API default and not a tuned value.
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195))
LABEL_TEXT_COLOR = (255, 255, 255)  # on dark palette entries
LABEL_TEXT_DARK = (0, 0, 0)  # on light ones (a bar whose 2 R + 5 G + B is above 8 * 140)
LABEL_CHOICES = ("id", "score", "id+score")


def encode(string) -> list:
    """The glyph codes of ``string``: lower case becomes upper case, a character outside the font a space."""
    return [max(CHARS.find(ch), 0) for ch in str(string).upper()]


def text_size(string, scale: int) -> Tuple[int, int]:
    """(width, height) in pixels of ``string`` at the integer ``scale``: (6 * scale * len - scale, 7 * scale)."""
    scale = _check_scale("text_size", scale)
    n = len(str(string))
    if not 1 <= n <= _vgho.MAX_TEXT:
        raise ValueError(f"text_size: string of {n} characters outside 1 .. {_vgho.MAX_TEXT}")
    return _vgho.GLYPH_PITCH * scale * n - scale, _vgho.GLYPH_ROWS * scale


def _check_scale(who: str, scale) -> int:
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= int(scale) <= _vgho.MAX_SCALE:
        raise ValueError(f"{who}: scale must be an integer in 1 .. {_vgho.MAX_SCALE}, got {scale!r}")
    return int(scale)


def _check_color(who: str, color) -> Tuple[int, int, int]:
    try:
        c = tuple(color)
    except TypeError:
        c = ()
    if len(c) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255 for v in c):
        raise ValueError(f"{who}: color must be three integers in 0 .. 255 (RGB), got {color!r}")
    return tuple(int(v) for v in c)


def _check_alpha(who: str, alpha, name: str = "alpha") -> int:
    """A float in [0, 1] as the library's 0 .. 256."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 <= float(alpha) <= 1.0:  # (a NaN fails the comparison)
        raise ValueError(f"{who}: {name} must be a number in [0, 1], got {alpha!r}")
    return int(math.floor(float(alpha) * 256.0 + 0.5))


def _check_box(who: str, box) -> Tuple[int, int, int, int]:
    try:
        b = tuple(box)
    except TypeError:
        b = ()
    if len(b) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in b):
        raise ValueError(f"{who}: box must be four integers (x0, y0, x1, y1), got {box!r}")
    x0, y0, x1, y1 = (int(v) for v in b)
    if max(abs(v) for v in (x0, y0, x1, y1)) > _vgho.MAX_COORD or not (0 <= x1 - x0 <= _vgho.MAX_SIDE and 0 <= y1 - y0 <= _vgho.MAX_SIDE):
        raise ValueError(f"{who}: box {(x0, y0, x1, y1)} must have sides of 0 .. {_vgho.MAX_SIDE} and coordinates within +-{_vgho.MAX_COORD}")
    return x0, y0, x1, y1


class Items:
    """What one ``render`` call draws, in order: a later item lies over an earlier one.  Boxes are (x0, y0, x1, y1) in pixels, half-open, and need not lie in
    the target; colours are RGB triples of integers; ``alpha`` is a number in [0, 1] (stored as round(256 alpha)).  Every method returns the builder."""

    def __init__(self):
        self._rows = []  # tuples in the order of _vgho.ITEM_DTYPE
        self._codes = []

    def __len__(self) -> int:
        return len(self._rows)

    def _add(self, who, kind, box, color, alpha, thickness=0, scale=0, code_offset=0, length=0):
        if len(self._rows) >= _vgho.MAX_ITEMS:
            raise ValueError(f"{who}: more than {_vgho.MAX_ITEMS} items in one call")
        self._rows.append((kind, *box, thickness, scale, code_offset, length, alpha, color, 0))
        return self

    def bar(self, box, color, alpha: float = 1.0) -> "Items":
        """A filled box."""
        return self._add("bar", _vgho.BAR, _check_box("bar", box), _check_color("bar", color), _check_alpha("bar", alpha))

    def rect(self, box, color, thickness: int, alpha: float = 1.0) -> "Items":
        """The outline of a box: a band of ``thickness`` pixels INSIDE its four edges."""
        if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)) or not 1 <= int(thickness) <= _vgho.MAX_SIDE:
            raise ValueError(f"rect: thickness must be an integer in 1 .. {_vgho.MAX_SIDE}, got {thickness!r}")
        return self._add("rect", _vgho.RECT, _check_box("rect", box), _check_color("rect", color), _check_alpha("rect", alpha), thickness=int(thickness))

    def text(self, x: int, y: int, string, color, scale: int, alpha: float = 1.0) -> "Items":
        """``string`` with its top left corner at (x, y), ``text_size(string, scale)`` pixels large."""
        w, h = text_size(string, _check_scale("text", scale))
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (x, y)):
            raise ValueError(f"text: x and y must be integers, got {(x, y)!r}")
        box = _check_box("text", (int(x), int(y), int(x) + w, int(y) + h))
        codes = encode(string)
        self._add("text", _vgho.TEXT, box, _check_color("text", color), _check_alpha("text", alpha), scale=int(scale), code_offset=len(self._codes), length=len(codes))
        self._codes += codes
        return self

    def rows(self, convert=None) -> np.ndarray:
        """The ``vgho_item`` rows; ``convert`` maps every RGB colour to the target's three plane bytes."""
        if convert is None:
            return np.array(self._rows, dtype=_vgho.ITEM_DTYPE)
        cache = {c: tuple(convert(c)) for c in {r[10] for r in self._rows}}
        return np.array([(*r[:10], cache[r[10]], 0) for r in self._rows], dtype=_vgho.ITEM_DTYPE)

    def codes(self) -> np.ndarray:
        return np.array(self._codes, dtype=np.uint8)

    def __repr__(self) -> str:
        return f"Items({len(self)} items, {len(self._codes)} glyph codes)"


# ---- render ---------------------------------------------------------------------------------------------------------------------------------------------
def _call(planes, H: int, W: int, rows: np.ndarray, codes: np.ndarray, device) -> None:
    """``planes``: (src tensor, dst tensor, src pitch, dst pitch, src step, dst step, shift) each; pointers are taken here."""
    import torch

    lib = _vgho.load()
    job = _vgho.Job()
    for k, (s, d, sp, dp, ss, ds, shift) in enumerate(planes):
        p = job.planes[k]
        p.src_dev, p.dst_dev, p.src_pitch, p.dst_pitch, p.src_step, p.dst_step, p.shift = s, d, sp, dp, ss, ds, shift
    job.height, job.width, job.n_planes, job.n_items = H, W, len(planes), len(rows)
    if len(rows):
        job.items = rows.ctypes.data
    if len(codes):
        job.codes, job.n_codes = codes.ctypes.data, len(codes)
    need = int(lib.vgho_workspace_bytes(job))
    if need <= 0:
        _vgho.check(-1)  # raises with the library's own message
    with torch.cuda.device(device):
        workspace = torch.empty(need, dtype=torch.uint8, device=device)  # allocated, used and (by the caching allocator) reused in the order of this stream
        _vgho.check(lib.vgho_draw(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))


def _need_gpu() -> None:
    import torch

    if not torch.cuda.is_available():
        raise VghError("overlays need a GPU: the HIP kernels of libvghosd.so are the only implementation of the samples")


def _render_frame(frame, items: Items, out):
    from .video import _plane_pairs, rgb_to_yuv

    H, W, _ = frame.shape
    out, planes = _plane_pairs("render", frame, out)
    rows = items.rows(lambda c: rgb_to_yuv(c, (out or frame).matrix, (out or frame).full_range))
    if planes is None:
        _need_gpu()
        raise VghError("overlays need a frame on a GPU: the HIP kernels of libvghosd.so are the only implementation of the samples")
    _call([(*row, 0 if k == 0 else 1) for k, row in enumerate(planes)], H, W, rows, items.codes(), frame.device)
    return out


def _render_image(target, items: Items, out):
    import torch

    t = target if isinstance(target, torch.Tensor) else np.asarray(target)
    if str(t.dtype).replace("torch.", "") != "uint8" or len(t.shape) != 3 or t.shape[2] != 3:
        raise ValueError(f"render: target must be a video.YUV420Frame or a uint8 image [H, W, 3]; got {t.dtype} {tuple(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    if not (1 <= H <= _vgho.MAX_SIDE and 1 <= W <= _vgho.MAX_SIDE):
        raise ValueError(f"render: target sides must be 1 .. {_vgho.MAX_SIDE} pixels; got {(H, W)}")

    def strides_ok(x):
        return x.stride(2) == 1 and (W == 1 or x.stride(1) == 3) and (H == 1 or x.stride(0) >= 3 * W)

    if isinstance(t, torch.Tensor) and t.is_cuda and not strides_ok(t):
        raise ValueError(f"render: target needs pixels 3 bytes apart and rows at least 3 * W bytes apart; got strides {tuple(t.stride())}")
    if out is not None and out is not target:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3) and out.is_cuda and strides_ok(out)):
            raise ValueError(f"render: out must be the target itself or a uint8 GPU tensor [{H}, {W}, 3] with pixels 3 bytes apart; got {type(out).__name__} "
                             f"{tuple(getattr(out, 'shape', ()))}")
    if out is target and not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError("render: out=target (in place) needs a GPU tensor; a NumPy or CPU image is uploaded and a new GPU tensor returned")
    rows = items.rows()
    _need_gpu()
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not t.is_cuda:
        t = t.contiguous().to(torch.device("cuda", torch.cuda.current_device()))
        if out is None:
            out = t  # the upload is nobody else's: draw in it
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=t.device)
    elif out.device != t.device:
        raise ValueError(f"render: out is on {out.device}, the target on {t.device}")
    sp, dp = (t.stride(0) if H > 1 else 3 * W), (out.stride(0) if H > 1 else 3 * W)
    if out.data_ptr() != t.data_ptr() or sp != dp:
        s0, s1, d0, d1 = t.data_ptr(), t.data_ptr() + (H - 1) * sp + 3 * W, out.data_ptr(), out.data_ptr() + (H - 1) * dp + 3 * W
        if s0 < d1 and d0 < s1:
            raise ValueError("render: out overlaps the target without being the target: pass out=target for in place, or a tensor elsewhere")
    _call([(t.data_ptr() + c, out.data_ptr() + c, sp, dp, 3, 3, 0) for c in range(3)], H, W, rows, items.codes(), t.device)
    return out


def render(target, items: Items, out=None):
    """Draws ``items`` (csrc/osd.hip, libvghosd.so).  ``target``:

    a ``video.YUV420Frame``    -> a ``YUV420Frame``.  ``out=target`` (or any frame over the same planes): IN PLACE, only the samples of the items are written and
                                  nothing walks the frame; ``out=None``: a new dense frame of the target's layout, matrix and range; any other frame of the same
                                  size on the same device is written whole and must not overlap the target (its layout may differ: NV12 in, I420 out).  The
                                  items' RGB colours go through ``video.rgb_to_yuv(color, frame.matrix, frame.full_range)`` of the frame written.
    a uint8 [H, W, 3] NumPy image -> uploaded once; a GPU ``torch.uint8`` tensor is returned.
    a uint8 [H, W, 3] GPU tensor (rows may be pitched) -> a new dense tensor, or ``out``; ``out is target``: in place.

    ValueError for an argument, then VghError without a GPU or without the library: there is no CPU path for the samples."""
    from .video import YUV420Frame

    if not isinstance(items, Items):
        raise ValueError(f"render: items must be an overlay.Items, got {type(items).__name__}")
    if isinstance(target, YUV420Frame):
        return _render_frame(target, items, out)
    if target is None or isinstance(target, (str, bytes)):
        raise ValueError(f"render: target must be a video.YUV420Frame or a uint8 image [H, W, 3]; got {type(target).__name__}")
    return _render_image(target, items, out)


# ---- the plan of a result's heads: the host half ----------------------------------------------------------------------------------------------------------
def _round(v) -> int:
    return int(math.floor(float(v) + 0.5))


def _per_head(who: str, name: str, value, n: int, check):
    """One checked value per head from a single value or a sequence of n."""
    try:
        return [check(who, value)] * n
    except ValueError:
        pass
    try:
        seq = list(value)
    except TypeError:
        seq = None
    if seq is None or len(seq) != n:
        raise ValueError(f"{who}: {name} must be one value or a sequence of {n} (one per head), got {value!r}")
    return [check(f"{who}: {name}[{k}]", v) for k, v in enumerate(seq)]


def head_overlay_plan(shape, heads, *, boxes: bool = True, labels=None, colors="track", thickness="auto", text_scale="auto", alpha: float = 1.0, label_alpha: float = 1.0,
                      track_ids=None, coasting=None, coasting_alpha: float = 0.5) -> Items:
    """The ``Items`` of a result's heads; needs no GPU.  ``shape``: (H, W, ...) of the target.  Per head, in this order: a RECT on its ``bbox`` as
    [x, x + w) x [y, y + h) (``boxes``), then a BAR and a TEXT for its label (``labels``).

    ``labels``: None, "id" (``#<track id>``; the head's index where there are no ``track_ids``), "score" (``<int(round(100 score))>%``), "id+score" (both, a space
    between) or a sequence of one string per head.  With s the text scale the bar is 7 s + 2 s high and the text's width + 2 s wide, left-aligned with the box;
    it sits directly above the box where it fits (y - bar height >= 0), otherwise inside the box's top.  The text is black on a light bar and white on a dark one.
    ``colors``: "track" (``PALETTE[id % 16]``, the id as for "id"), one RGB triple, or one per head.  ``thickness`` and ``text_scale``: an integer, or "auto" =
    max(1, min(H, W) // 360).  ``alpha`` (boxes) and ``label_alpha`` (bars and texts) in [0, 1]; the heads with ``coasting[k]`` set are drawn with
    ``coasting_alpha`` times both.  These defaults are API defaults, NOT tuned values."""
    who = "head_overlay_plan"
    try:
        H, W = int(shape[0]), int(shape[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError(f"{who}: shape must be (H, W, ...), got {shape!r}") from None
    if not (1 <= H <= _vgho.MAX_SIDE and 1 <= W <= _vgho.MAX_SIDE):
        raise ValueError(f"{who}: shape {(H, W)} outside 1 .. {_vgho.MAX_SIDE}")
    n = len(heads)
    if not isinstance(boxes, (bool, np.bool_)):
        raise ValueError(f"{who}: boxes must be True or False, got {boxes!r}")
    auto = max(1, min(H, W) // 360)
    if not (isinstance(thickness, str) and thickness == "auto"):
        if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)) or not 1 <= int(thickness) <= _vgho.MAX_SIDE:
            raise ValueError(f"{who}: thickness must be 'auto' or an integer in 1 .. {_vgho.MAX_SIDE}, got {thickness!r}")
    t = auto if isinstance(thickness, str) else int(thickness)
    if not (isinstance(text_scale, str) and text_scale == "auto"):
        _check_scale(f"{who}: text_scale", text_scale)
    s = min(auto, _vgho.MAX_SCALE) if isinstance(text_scale, str) else int(text_scale)
    a_box, a_label, a_coast = _check_alpha(who, alpha), _check_alpha(who, label_alpha, "label_alpha"), None
    if isinstance(coasting_alpha, bool) or not isinstance(coasting_alpha, (int, float, np.integer, np.floating)) or not 0.0 <= float(coasting_alpha) <= 1.0:
        raise ValueError(f"{who}: coasting_alpha must be a number in [0, 1], got {coasting_alpha!r}")
    a_coast = float(coasting_alpha)
    ids = None
    if track_ids is not None:
        ids = [int(v) for v in np.asarray(track_ids).reshape(-1)]
        if len(ids) != n or any(v < 0 for v in ids):
            raise ValueError(f"{who}: track_ids must be {n} non-negative integers (one per head), got {track_ids!r}")
    coast = [False] * n
    if coasting is not None:
        coast = [bool(v) for v in np.asarray(coasting).reshape(-1)]
        if len(coast) != n:
            raise ValueError(f"{who}: coasting must be {n} booleans (one per head), got {coasting!r}")
    shown = ids if ids is not None else list(range(n))
    if labels is None:
        texts = [None] * n
    elif isinstance(labels, str):
        if labels not in LABEL_CHOICES:
            raise ValueError(f"{who}: labels must be None, one of {LABEL_CHOICES} or a sequence of one string per head, got {labels!r}")
        score = [f"{int(round(100.0 * float(h.score)))}%" for h in heads] if "score" in labels else None
        texts = [f"#{shown[k]}" if labels == "id" else score[k] if labels == "score" else f"#{shown[k]} {score[k]}" for k in range(n)]
    else:
        texts = list(labels)
        if len(texts) != n or any(not isinstance(v, str) or not 1 <= len(v) <= _vgho.MAX_TEXT for v in texts):
            raise ValueError(f"{who}: labels must be None, one of {LABEL_CHOICES} or a sequence of {n} strings of 1 .. {_vgho.MAX_TEXT} characters, got {labels!r}")
    if isinstance(colors, str):
        if colors != "track":
            raise ValueError(f"{who}: colors must be 'track', an RGB triple or a sequence of one per head, got {colors!r}")
        cols = [PALETTE[shown[k] % len(PALETTE)] for k in range(n)]
    else:
        cols = _per_head(who, "colors", colors, n, _check_color)
    items = Items()
    if 3 * n > _vgho.MAX_ITEMS:
        raise ValueError(f"{who}: {n} heads make more than {_vgho.MAX_ITEMS} items")
    limit, th = _vgho.MAX_COORD - _vgho.MAX_SIDE, _vgho.GLYPH_ROWS * s  # corners this far in keep every item's coordinates in range
    for k, head in enumerate(heads):
        x, y, w, h = head.bbox
        x0, y0, x1, y1 = _round(x), _round(y), _round(x + w), _round(y + h)
        x1, y1 = max(x1, x0), max(y1, y0)
        if not (-limit <= x0 <= limit and -limit <= y0 <= limit and x1 - x0 <= _vgho.MAX_SIDE and y1 - y0 <= _vgho.MAX_SIDE):
            raise ValueError(f"{who}: head {k}: bbox {tuple(head.bbox)} must have sides of 0 .. {_vgho.MAX_SIDE} and corners within +-{limit}")
        fade = a_coast if coast[k] else 1.0
        a_rect, a_text = int(math.floor(a_box * fade + 0.5)), int(math.floor(a_label * fade + 0.5))
        # everything below is checked already: the rows are appended as Items.rect / .bar / .text would make them
        if boxes:
            items._rows.append((_vgho.RECT, x0, y0, x1, y1, t, 0, 0, 0, a_rect, cols[k], 0))
        if texts[k] is not None:
            codes = encode(texts[k])
            tw = _vgho.GLYPH_PITCH * s * len(codes) - s
            bar_h = th + 2 * s
            by = y0 - bar_h if y0 - bar_h >= 0 else y0
            r, g, b = cols[k]
            items._rows.append((_vgho.BAR, x0, by, x0 + tw + 2 * s, by + bar_h, 0, 0, 0, 0, a_text, cols[k], 0))
            items._rows.append((_vgho.TEXT, x0 + s, by + s, x0 + s + tw, by + s + th, 0, s, len(items._codes), len(codes), a_text,
                                LABEL_TEXT_DARK if 2 * r + 5 * g + b > 8 * 140 else LABEL_TEXT_COLOR, 0))
            items._codes += codes
    return items


def draw_heads(target, heads, *, out=None, **plan_kw):
    """``render(target, head_overlay_plan(target.shape, heads, **plan_kw), out)``."""
    shape = getattr(target, "shape", None)
    if shape is None:
        raise ValueError(f"draw_heads: target must be a video.YUV420Frame or a uint8 image [H, W, 3]; got {type(target).__name__}")
    return render(target, head_overlay_plan(tuple(shape), heads, **plan_kw), out)
