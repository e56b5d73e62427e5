"""What the ctypes bindings of the companion libraries (``_lib_view``, ``_lib_vis``, ``_lib_tex``, ``_lib_eval``) share: loading a library with every
declared symbol bound, and turning a return code into ``VghError``.  NO fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from ._lib import VghError


def load_library(path: str, symbols: dict) -> C.CDLL:
    """Load the library at ``path`` and bind every symbol of ``symbols`` (name -> (restype, argtypes)).  Raises VghError if it is absent or stale."""
    if not os.path.exists(path):
        raise VghError(f"{path} not found: the HIP extension is not built. Run `python -m head_detector_amd.build` (needs hipcc). "
                       "There is no CPU fallback in this package.")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise VghError(f"failed to load {path}: {e}") from e
    for name, (res, args) in symbols.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise VghError(f"{path} does not export {name} (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    return lib


def raise_for(rc: int, libname: str, last_error_fn) -> None:
    """Raise VghError for the non-zero ``rc`` with the calling thread's message (``last_error_fn`` = the library's ``*_last_error``)."""
    raise VghError(f"{libname} error {rc}: {last_error_fn().decode('utf-8', 'replace')}")
