"""ctypes binding of libvghcrop.so (include/vgh_crop.h): head tensors.  A library of its own: none of libvgh.so, libvghview.so, libvghvis.so, libvghtex.so,
libvgheval.so, libvghmerge.so, libvghtrack.so, libvghanon.so and libvghvideo.so knows of it, and their bindings do not load it; like them there is NO fallback: a
missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghcrop.so")
MAX_SIZE = 1024  # = VGHC_MAX_SIZE
MAX_SUPERSAMPLE = 8  # = VGHC_MAX_SUPERSAMPLE
MAX_HEADS = 65536  # = VGHC_MAX_HEADS
MAX_SIDE = 32767  # = VGHC_MAX_SIDE
MAX_TILES = 16777216  # = VGHC_MAX_TILES
SOURCE_RGB, SOURCE_YUV420 = 0, 1  # = VGHC_SOURCE_*
DTYPES = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3}  # = VGHC_DTYPE_*
LAYOUTS = {"nchw": 0, "nhwc": 1}  # = VGHC_LAYOUT_*
ORDERS = {"rgb": 0, "bgr": 1}  # = VGHC_ORDER_*

# vghc_head: one row of the job's ``heads`` array
HEAD_DTYPE = np.dtype([("x0", np.int64), ("xp", np.int64), ("xq", np.int64), ("y0", np.int64), ("yp", np.int64), ("yq", np.int64), ("source", np.int32),
                       ("supersample", np.int32), ("a", np.float32, (3,)), ("reserved", np.int32)])


class Source(C.Structure):
    """vghc_source: one u8 RGB image or one 8-bit YUV 4:2:0 frame on the device."""
    _fields_ = [("kind", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("chroma_step", C.c_int32), ("rgb_dev", C.c_void_p), ("rgb_pitch_bytes", C.c_int64),
                ("y_dev", C.c_void_p), ("u_dev", C.c_void_p), ("v_dev", C.c_void_p), ("y_pitch_bytes", C.c_int64), ("uv_pitch_bytes", C.c_int64), ("y_offset", C.c_int32),
                ("cy", C.c_int32), ("crv", C.c_int32), ("cgu", C.c_int32), ("cgv", C.c_int32), ("cbu", C.c_int32)]


class Job(C.Structure):
    """vghc_job: the sources and the per-head rows on the host, the crop size, the output's format, and the destination."""
    _fields_ = [("sources", C.c_void_p), ("heads", C.c_void_p), ("n_sources", C.c_int32), ("n_heads", C.c_int32), ("size", C.c_int32), ("dtype", C.c_int32),
                ("layout", C.c_int32), ("channel_order", C.c_int32), ("fill", C.c_int32), ("b", C.c_float * 3), ("dst_dev", C.c_void_p), ("dst_bytes", C.c_int64)]


# every symbol include/vgh_crop.h declares: (restype, argtypes)
SYMBOLS = {
    "vghc_version": (C.c_char_p, []),
    "vghc_last_error": (C.c_char_p, []),
    "vghc_head_tensors": (C.c_int, [C.POINTER(Job), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghcrop.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghcrop", load().vghc_last_error)
