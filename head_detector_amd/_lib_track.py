"""ctypes binding of libvghtrack.so (include/vgh_track.h): head tracking across video frames.  A library of its own: none of libvgh.so, libvghview.so,
libvghvis.so, libvghtex.so, libvgheval.so and libvghmerge.so knows of it, and their bindings do not load it; like them there is NO fallback: a missing library
raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghtrack.so")
MAX_TRACKS = 2048  # = VGHT_MAX_TRACKS
MAX_DETS = 2048  # = VGHT_MAX_DETS
MAX_FRAMES = 1024  # = VGHT_MAX_FRAMES
NUM_PARAMS = 413  # = VGHT_NUM_PARAMS
STATE_HEADER_BYTES = 16  # = VGHT_STATE_HEADER_BYTES


class TrackJob(C.Structure):
    """vght_track_job: sizes, the rule's parameters, the four slabs on the device, the unpad table on the host and the per-frame outputs."""
    _fields_ = [("n_frames", C.c_int32), ("keep_k", C.c_int32), ("max_tracks", C.c_int32), ("image_size", C.c_int32), ("max_out", C.c_int32), ("max_age", C.c_int32),
                ("min_hits", C.c_int32), ("report_misses", C.c_int32), ("high_thr", C.c_float), ("low_thr", C.c_float), ("match_thr", C.c_float),
                ("match_thr_low", C.c_float), ("box_gain", C.c_float), ("vel_gain", C.c_float), ("param_gain", C.c_float), ("reserved", C.c_int32),
                ("boxes_dev", C.c_void_p), ("scores_dev", C.c_void_p), ("flame_dev", C.c_void_p), ("counts_dev", C.c_void_p), ("unpad", C.c_void_p),
                ("n_out_dev", C.c_void_p), ("out_slot_dev", C.c_void_p), ("out_id_dev", C.c_void_p), ("out_det_row_dev", C.c_void_p), ("out_hits_dev", C.c_void_p),
                ("out_misses_dev", C.c_void_p), ("out_box_dev", C.c_void_p), ("out_score_dev", C.c_void_p), ("out_params_dev", C.c_void_p), ("det_id_dev", C.c_void_p),
                ("n_born_dev", C.c_void_p), ("n_freed_dev", C.c_void_p), ("n_dropped_dev", C.c_void_p)]


# every symbol include/vgh_track.h declares: (restype, argtypes)
SYMBOLS = {
    "vght_version": (C.c_char_p, []),
    "vght_last_error": (C.c_char_p, []),
    "vght_state_bytes": (C.c_int64, [C.c_int32]),
    "vght_state_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "vght_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "vght_track_frames": (C.c_int, [C.POINTER(TrackJob), C.c_void_p, C.c_void_p, C.c_void_p]),
}


def state_layout(max_tracks: int) -> Dict[str, int]:
    """Byte offsets of the parts of the state (the layout include/vgh_track.h documents) and its size under "total"."""
    col = (4 * max_tracks + 15) & ~15
    at, off = {}, STATE_HEADER_BYTES
    for name in ("id", "hits", "misses", "age", "det_row", "score"):
        at[name], off = off, off + col
    at["box"], off = off, off + 16 * max_tracks
    at["vel"], off = off, off + 16 * max_tracks
    at["params"], off = off, off + ((4 * NUM_PARAMS * max_tracks + 15) & ~15)
    at["total"] = off
    return at


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghtrack.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghtrack", load().vght_last_error)
