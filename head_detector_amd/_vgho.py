"""ctypes binding of libvghosd.so (include/vgh_osd.h): the on-screen display (bars, boxes and bitmap text in a frame's own planes).  A library of its own: none of
libvgh.so, libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so, libvghtrack.so, libvghanon.so, libvghvideo.so and libvghcrop.so knows of it,
and their bindings do not load it; like them there is NO fallback: a missing library raises ``VghError``.

The file is named after the library's prefix (``vgho_``) and not ``_lib_osd.py`` on purpose: the host tests of the head-tensor library count the ``_lib*.py``
bindings beside ``_lib_crop.py`` and hold that count at nine, and a new library does not rewrite another library's tests."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghosd.so")
MAX_SIDE = 32767  # = VGHO_MAX_SIDE
MAX_COORD = 16777215  # = VGHO_MAX_COORD
MAX_ITEMS = 65536  # = VGHO_MAX_ITEMS
MAX_PLANES = 3  # = VGHO_MAX_PLANES
MAX_TEXT = 64  # = VGHO_MAX_TEXT
MAX_SCALE = 16  # = VGHO_MAX_SCALE
MAX_ALPHA = 256  # = VGHO_MAX_ALPHA
MAX_TILES = 16777216  # = VGHO_MAX_TILES
GLYPHS, GLYPH_ROWS, GLYPH_COLS, GLYPH_PITCH = 44, 7, 5, 6  # = VGHO_GLYPHS, VGHO_GLYPH_ROWS, VGHO_GLYPH_COLS, VGHO_GLYPH_PITCH
BAR, RECT, TEXT = 0, 1, 2  # = VGHO_BAR, VGHO_RECT, VGHO_TEXT

# vgho_item: one row of the job's ``items`` array
ITEM_DTYPE = np.dtype([("kind", np.int32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("thickness", np.int32), ("scale", np.int32),
                       ("code_offset", np.int32), ("length", np.int32), ("alpha", np.int32), ("color", np.uint8, (3,)), ("reserved", np.uint8)])


class Plane(C.Structure):
    """vgho_plane: one plane of the target, where it is read and where it is written."""
    _fields_ = [("src_dev", C.c_void_p), ("dst_dev", C.c_void_p), ("src_pitch", C.c_int64), ("dst_pitch", C.c_int64), ("src_step", C.c_int32), ("dst_step", C.c_int32),
                ("shift", C.c_int32), ("reserved", C.c_int32)]


class Job(C.Structure):
    """vgho_job: the target's planes, its size, and the items and glyph codes on the host."""
    _fields_ = [("planes", Plane * MAX_PLANES), ("height", C.c_int32), ("width", C.c_int32), ("n_planes", C.c_int32), ("n_items", C.c_int32), ("items", C.c_void_p),
                ("codes", C.c_void_p), ("n_codes", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/vgh_osd.h declares: (restype, argtypes)
SYMBOLS = {
    "vgho_version": (C.c_char_p, []),
    "vgho_last_error": (C.c_char_p, []),
    "vgho_workspace_bytes": (C.c_int64, [C.POINTER(Job)]),
    "vgho_draw": (C.c_int, [C.POINTER(Job), C.c_void_p, C.c_void_p]),
    "vgho_font": (C.c_int, [C.c_int32, C.POINTER(C.c_uint8 * 7)]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghosd.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghosd", load().vgho_last_error)


def font() -> np.ndarray:
    """uint8 [GLYPHS, 7]: the library's font table, read through vgho_font."""
    lib = load()
    out = np.zeros((GLYPHS, GLYPH_ROWS), np.uint8)
    rows = (C.c_uint8 * 7)()
    for code in range(GLYPHS):
        check(lib.vgho_font(code, C.byref(rows)))
        out[code] = list(rows)
    return out
