"""ctypes binding of libvgheval.so (include/vgh_eval.h): mesh benchmark metrics.  A library of its own: none of libvgh.so, libvghview.so, libvghvis.so and
libvghtex.so knows of it, and their bindings do not load it; like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvgheval.so")
MAX_HEADS = 1048576  # = VGHEV_MAX_HEADS
MAX_POINTS = 1048576  # = VGHEV_MAX_POINTS
MAX_TOP_K = 16  # = VGHEV_MAX_TOP_K
NEIGHBOURS = {"reference": 0, "nearest": 1}  # = VGHEV_NEIGHBOURS_REFERENCE, VGHEV_NEIGHBOURS_NEAREST


class ZOrderJob(C.Structure):
    """vghev_z_order_job: predicted and ground-truth points of n heads on the device and the agreement counts they give."""
    _fields_ = [("n_heads", C.c_int32), ("n_points", C.c_int32), ("top_k", C.c_int32), ("mode", C.c_int32), ("pred_dev", C.c_void_p), ("gt_dev", C.c_void_p),
                ("agree_dev", C.c_void_p)]


class NearestJob(C.Structure):
    """vghev_nearest_job: queries and points of n heads on the device, the optional per-head scales and transform, and the three outputs."""
    _fields_ = [("n_heads", C.c_int32), ("n_queries", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32), ("query_dev", C.c_void_p),
                ("query_scale_dev", C.c_void_p), ("points_dev", C.c_void_p), ("transform_dev", C.c_void_p), ("point_scale_dev", C.c_void_p),
                ("sqdist_dev", C.c_void_p), ("index_dev", C.c_void_p), ("mean_dev", C.c_void_p)]


# every symbol include/vgh_eval.h declares: (restype, argtypes)
SYMBOLS = {
    "vghev_version": (C.c_char_p, []),
    "vghev_last_error": (C.c_char_p, []),
    "vghev_z_order": (C.c_int, [C.POINTER(ZOrderJob), C.c_void_p]),
    "vghev_nearest": (C.c_int, [C.POINTER(NearestJob), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvgheval.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvgheval", load().vghev_last_error)
