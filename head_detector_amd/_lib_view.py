"""ctypes binding of libvghview.so (include/vgh_view.h): the companion library of result-side image helpers.  libvgh.so knows nothing of it
and ``_lib`` does not load it; like ``_lib`` there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghview.so")
MAX_SIDE = 32767  # = VGHV_MAX_SIDE
MAX_COORD = 1 << 24  # = VGHV_MAX_COORD
MAX_RADIUS = 32  # = VGHV_MAX_RADIUS
MAX_DRAW_HEADS = 65536  # = VGHV_MAX_DRAW_HEADS


class Crop(C.Structure):
    """vghv_crop: one crop of an affinely warped u8 RGB image (tables and result addressed by offsets into the call's shared arrays)."""
    _fields_ = [("src_dev", C.c_void_p), ("src_pitch_bytes", C.c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("src_channels", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32), ("table_offset", C.c_int64), ("dst_offset", C.c_int64)]


class DrawJob(C.Structure):
    """vghv_draw_job: one image and everything that is painted over it (points, boxes and topology are host arrays, uploaded by the call)."""
    _fields_ = [("src_dev", C.c_void_p), ("src_pitch_bytes", C.c_int64), ("dst_dev", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("n_heads", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("n_indices", C.c_int32), ("radius", C.c_int32), ("points", C.c_void_p),
                ("boxes", C.c_void_p), ("triangles", C.c_void_p), ("indices", C.c_void_p), ("half_widths", C.c_void_p)]


class MeshJob(C.Structure):
    """vghv_mesh_job: one image and the meshes blended over it (vertices and colours on the device, topology and per-head pixel bounds on the host)."""
    _fields_ = [("src_dev", C.c_void_p), ("src_pitch_bytes", C.c_int64), ("dst_dev", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("n_heads", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("reverse", C.c_int32), ("colors_per_head", C.c_int32), ("shade", C.c_int32),
                ("alpha", C.c_float), ("z_sign", C.c_float), ("ambient", C.c_float), ("diffuse", C.c_float), ("verts_dev", C.c_void_p), ("triangles", C.c_void_p),
                ("bounds", C.c_void_p), ("colors_dev", C.c_void_p), ("color", C.c_float * 3), ("light", C.c_float * 3)]


# every symbol include/vgh_view.h declares: (restype, argtypes)
_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
SYMBOLS = {
    "vghv_version": (C.c_char_p, []),
    "vghv_last_error": (C.c_char_p, []),
    "vghv_warp_crops": (_I, [C.POINTER(Crop), _I, _P, _I64, _P, _I64, _P]),
    "vghv_draw_heads": (_I, [C.POINTER(DrawJob), _P]),
    "vghv_vertex_normals": (_I, [_P, _I, _I, _P, _I, _P, _P]),
    "vghv_render_meshes": (_I, [C.POINTER(MeshJob), _P]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghview.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghview", load().vghv_last_error)
