"""ctypes binding of libvghtex.so (include/vgh_tex.h): head textures.  A library of its own: none of libvgh.so, libvghview.so and libvghvis.so knows
of it, and ``_lib`` / ``_lib_view`` / ``_lib_vis`` do not load it; like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvghtex.so")
MAX_SIDE = 32767  # = VGHTEX_MAX_SIDE
MAX_HEADS = 65536  # = VGHTEX_MAX_HEADS
MAX_CHANNELS = 16  # = VGHTEX_MAX_CHANNELS
MODES = {"order": 0, "depth": 1}  # = VGHTEX_MODE_ORDER, VGHTEX_MODE_DEPTH
MAPPINGS = {"nearest": 0, "bilinear": 1}  # = VGHTEX_MAP_NEAREST, VGHTEX_MAP_BILINEAR
TEX_DTYPES = {"float32": 0, "uint8": 1}  # = VGHTEX_TEX_F32, VGHTEX_TEX_U8


class Job(C.Structure):
    """vghtex_job: the meshes of one image (vertices, texture coordinates and textures on the device, both topologies and the per-head pixel bounds on the
    host) and the buffers they are painted into."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("n_heads", C.c_int32), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32),
                ("n_tex_vertices", C.c_int32), ("tex_height", C.c_int32), ("tex_width", C.c_int32), ("tex_channels", C.c_int32), ("tex_dtype", C.c_int32),
                ("tex_per_head", C.c_int32), ("tex_coords_per_head", C.c_int32), ("dst_per_head", C.c_int32), ("mapping", C.c_int32), ("mode", C.c_int32),
                ("z_sign", C.c_float), ("verts_dev", C.c_void_p), ("triangles", C.c_void_p), ("tex_coords_dev", C.c_void_p), ("tex_triangles", C.c_void_p),
                ("texture_dev", C.c_void_p), ("bounds", C.c_void_p), ("dst_dev", C.c_void_p), ("depth_dev", C.c_void_p), ("triangle_dev", C.c_void_p),
                ("head_dev", C.c_void_p)]


# every symbol include/vgh_tex.h declares: (restype, argtypes)
SYMBOLS = {
    "vghtex_version": (C.c_char_p, []),
    "vghtex_last_error": (C.c_char_p, []),
    "vghtex_render_texture": (C.c_int, [C.POINTER(Job), C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvghtex.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvghtex", load().vghtex_last_error)
