"""ctypes binding of libvghvideo.so (include/vgh_video.h): heads anonymised in the planes of a YUV 4:2:0 frame, and RGB packed into such planes.  A library of
its own: none of libvgh.so, libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so, libvghtrack.so and libvghanon.so knows of it, and their
bindings do not load it; this one takes the constants of ``_lib_anon`` (importing that module loads no library: ``load()`` is lazy) and loads nothing but its
own library.  Like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)
# The caps (VGHY_MAX_*, VGHY_TAP_SUM), the methods, the regions and the head row (vghy_head: one row of the job's ``luma_heads`` / ``chroma_heads`` arrays) are
# those of vgh_anon.h, number for number, so that the plan of one serves the other: Python states them once.
from ._lib_anon import HEAD_DTYPE, MAX_CELLS, MAX_COORD, MAX_HEADS, MAX_RADIUS, MAX_SIDE, METHODS, REGION_BOX, REGION_ELLIPSE, REGION_MAP, TAP_SUM  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghvideo.so")


class Plane(C.Structure):
    """vghy_plane: one plane's source and destination, each with its own row pitch and sample step."""
    _fields_ = [("src_dev", C.c_void_p), ("dst_dev", C.c_void_p), ("src_pitch", C.c_int64), ("dst_pitch", C.c_int64), ("src_step", C.c_int32), ("dst_step", C.c_int32)]


class AnonymizeJob(C.Structure):
    """vghy_anonymize_job: the three planes, the sizes, the effect, and the two rows per head and the tap table on the host."""
    _fields_ = [("planes", Plane * 3), ("height", C.c_int32), ("width", C.c_int32), ("n_heads", C.c_int32), ("method", C.c_int32), ("region", C.c_int32), ("color", C.c_int32),
                ("luma_heads", C.c_void_p), ("chroma_heads", C.c_void_p), ("taps", C.c_void_p), ("n_taps", C.c_int32), ("reserved", C.c_int32), ("owner_dev", C.c_void_p)]


class PackJob(C.Structure):
    """vghy_pack_job: the RGB image, the three destination planes, the nine coefficients and the luma offset."""
    _fields_ = [("src_dev", C.c_void_p), ("src_pitch_bytes", C.c_int64), ("planes", Plane * 3), ("height", C.c_int32), ("width", C.c_int32), ("coef", C.c_int32 * 9),
                ("y_offset", C.c_int32)]


# every symbol include/vgh_video.h declares: (restype, argtypes)
SYMBOLS = {
    "vghy_version": (C.c_char_p, []),
    "vghy_last_error": (C.c_char_p, []),
    "vghy_anonymize_workspace_bytes": (C.c_int64, [C.POINTER(AnonymizeJob)]),
    "vghy_anonymize": (C.c_int, [C.POINTER(AnonymizeJob), C.c_void_p, C.c_void_p]),
    "vghy_pack_rgb": (C.c_int, [C.POINTER(PackJob), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghvideo.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghvideo", load().vghy_last_error)
