"""ctypes binding of libvghmerge.so (include/vgh_merge.h): the cross-tile merge of sliced detection.  A library of its own: none of libvgh.so, libvghview.so,
libvghvis.so, libvghtex.so and libvgheval.so knows of it, and their bindings do not load it; like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghmerge.so")
MAX_CANDIDATES = 16384  # = VGHM_MAX_CANDIDATES
MAX_HEADS = 1048576  # = VGHM_MAX_HEADS
METRICS = {"iou": 0, "ios": 1}  # = VGHM_METRIC_IOU, VGHM_METRIC_IOS
STATUS_ABSENT, STATUS_KEPT, STATUS_TRUNCATED, STATUS_SUPPRESSED, STATUS_OVER_CAP = range(5)  # = VGHM_STATUS_*


class MergeJob(C.Structure):
    """vghm_merge_job: the per-tile slabs on the device, the three plan tables on the host, the rule's parameters and the outputs."""
    _fields_ = [("n_tiles", C.c_int32), ("keep_k", C.c_int32), ("image_size", C.c_int32), ("max_heads", C.c_int32), ("metric", C.c_int32), ("border", C.c_float),
                ("match_thr", C.c_float), ("reserved", C.c_int32), ("boxes_dev", C.c_void_p), ("scores_dev", C.c_void_p), ("counts_dev", C.c_void_p),
                ("tiles", C.c_void_p), ("scale", C.c_void_p), ("interior", C.c_void_p), ("head_row_dev", C.c_void_p), ("head_tile_dev", C.c_void_p),
                ("boxes_full_dev", C.c_void_p), ("scores_out_dev", C.c_void_p), ("n_heads_dev", C.c_void_p), ("n_kept_uncapped_dev", C.c_void_p),
                ("status_dev", C.c_void_p)]


# every symbol include/vgh_merge.h declares: (restype, argtypes)
SYMBOLS = {
    "vghm_version": (C.c_char_p, []),
    "vghm_last_error": (C.c_char_p, []),
    "vghm_merge_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "vghm_merge_tiles": (C.c_int, [C.POINTER(MergeJob), C.c_void_p, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghmerge.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghmerge", load().vghm_last_error)
