"""ctypes binding of libvghvis.so (include/vgh_vis.h): head visibility buffers.  A library of its own: neither libvgh.so nor libvghview.so knows of
it, and ``_lib`` / ``_lib_view`` do not load it; like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghvis.so")
MAX_SIDE = 32767  # = VGHVIS_MAX_SIDE
MAX_HEADS = 65536  # = VGHVIS_MAX_HEADS
MODES = {"order": 0, "depth": 1}  # = VGHVIS_MODE_ORDER, VGHVIS_MODE_DEPTH


class Job(C.Structure):
    """vghvis_job: the meshes of one image (vertices on the device, topology and per-head pixel bounds on the host) and the buffers they are measured into."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("n_heads", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("mode", C.c_int32),
                ("z_sign", C.c_float), ("verts_dev", C.c_void_p), ("triangles", C.c_void_p), ("bounds", C.c_void_p), ("depth_dev", C.c_void_p), ("triangle_dev", C.c_void_p),
                ("head_dev", C.c_void_p), ("bary_dev", C.c_void_p), ("visible_px_dev", C.c_void_p), ("covered_px_dev", C.c_void_p), ("vertex_visible_dev", C.c_void_p)]


# every symbol include/vgh_vis.h declares: (restype, argtypes)
SYMBOLS = {
    "vghvis_version": (C.c_char_p, []),
    "vghvis_last_error": (C.c_char_p, []),
    "vghvis_rasterize_triangles": (C.c_int, [C.POINTER(Job), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghvis.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghvis", load().vghvis_last_error)
