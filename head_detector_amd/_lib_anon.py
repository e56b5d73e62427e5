"""ctypes binding of libvghanon.so (include/vgh_anon.h): head anonymisation.  A library of its own: none of libvgh.so, libvghview.so, libvghvis.so,
libvghtex.so, libvgheval.so, libvghmerge.so and libvghtrack.so knows of it, and their bindings do not load it; like them there is NO fallback: a missing library
raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghanon.so")
MAX_SIDE = 32767  # = VGHAN_MAX_SIDE
MAX_COORD = 16777216  # = VGHAN_MAX_COORD
MAX_HEADS = 65536  # = VGHAN_MAX_HEADS
MAX_CELLS = 64  # = VGHAN_MAX_CELLS
MAX_RADIUS = 1024  # = VGHAN_MAX_RADIUS
TAP_SUM = 65536  # = VGHAN_TAP_SUM
METHODS = {"fill": 0, "pixelate": 1, "blur": 2}  # = VGHAN_METHOD_*
REGION_BOX, REGION_ELLIPSE, REGION_MAP = 0, 1, 2  # = VGHAN_REGION_*

# vghan_head: one row of the job's ``heads`` array (eight int32)
HEAD_DTYPE = np.dtype([(name, np.int32) for name in ("x0", "y0", "x1", "y1", "cell", "radius", "tap_offset", "reserved")])


class Job(C.Structure):
    """vghan_job: the two images, the sizes, the effect, and the per-head rows and the tap table on the host."""
    _fields_ = [("src_dev", C.c_void_p), ("dst_dev", C.c_void_p), ("src_pitch_bytes", C.c_int64), ("height", C.c_int32), ("width", C.c_int32), ("n_heads", C.c_int32),
                ("method", C.c_int32), ("region", C.c_int32), ("color", C.c_int32), ("heads", C.c_void_p), ("taps", C.c_void_p), ("n_taps", C.c_int32), ("reserved", C.c_int32),
                ("owner_dev", C.c_void_p)]


# every symbol include/vgh_anon.h declares: (restype, argtypes)
SYMBOLS = {
    "vghan_version": (C.c_char_p, []),
    "vghan_last_error": (C.c_char_p, []),
    "vghan_workspace_bytes": (C.c_int64, [C.POINTER(Job)]),
    "vghan_anonymize": (C.c_int, [C.POINTER(Job), C.c_void_p, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghanon.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghanon", load().vghan_last_error)
