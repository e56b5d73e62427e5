"""CPU: the host side of VGH_IMG_U8_RAW (images of any size, letterboxed inside vgh_detect) -- the C ABI additions, the ctypes mirror of
vgh_raw_image against the C compiler's layout, and the library's C++ port of letterbox.py's tables (bit-identical to the Python spec)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from head_detector_amd import _lib
from head_detector_amd.letterbox import axis_tables, geometry


def _compile(tmp_path, name, source, compiler, extra=()):
    cc = shutil.which(compiler)
    if cc is None:
        pytest.fail(f"{compiler} is needed to check the C / C++ side")
    src = tmp_path / f"{name}.{'c' if compiler == 'gcc' else 'cpp'}"
    src.write_text(source)
    exe = str(tmp_path / name)
    subprocess.run([cc, *extra, str(src), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def test_header_declares_the_raw_image_format():
    hdr = open(os.path.join(ROOT, "include", "vgh.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+VGH_IMG_U8_RAW\s+2\b", code)
    assert re.search(r"#define\s+VGH_SCRATCH_UNPAD\s+5\b", code)
    assert re.search(r"#define\s+VGH_SCRATCH_CANVAS\s+6\b", code)
    assert re.search(r"typedef\s+struct\s+vgh_raw_image\s*\{[^}]*\}\s*vgh_raw_image\s*;", code)
    assert re.search(r"#define\s+VGH_ABI_VERSION\s+8\b", code)
    assert (_lib.VGH_IMG_U8_RAW, _lib.SCRATCH_UNPAD, _lib.SCRATCH_CANVAS) == (2, 5, 6)


def test_abi_version_is_8_in_binding_and_library():
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.vgh_abi_version() == 8


def test_ctypes_raw_image_matches_the_c_layout(tmp_path):
    fields = [f for f, _ in _lib.RawImage._fields_]
    assert fields == ["data_dev", "h", "w", "channels", "pitch_bytes"]
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"vgh.h\"\nint main(void) {\n    printf(\"%zu\\n\", sizeof(vgh_raw_image));\n"
    prog += "".join(f"    printf(\"%zu\\n\", offsetof(vgh_raw_image, {f}));\n" for f in fields) + "    return 0;\n}\n"
    exe = _compile(tmp_path, "raw_layout", prog, "gcc", ["-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include")])
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    import ctypes as C

    assert got == [C.sizeof(_lib.RawImage)] + [getattr(_lib.RawImage, f).offset for f in fields]


# source / destination lengths: identity, up- and downscaling, odd, extreme ratios, one-pixel axes
_PAIRS = [(640, 640), (131, 640), (97, 474), (4000, 640), (3000, 480), (517, 640), (333, 413), (1, 640), (4000, 1), (2, 5), (1920, 640), (1080, 360),
          (211, 320), (307, 320), (7, 320), (12345, 640), (641, 640), (639, 640), (480, 321)]


def test_library_tables_are_bit_identical_to_letterbox_py(tmp_path):
    """csrc/letterbox_tables.h (what vgh_detect builds for VGH_IMG_U8_RAW) against letterbox.axis_tables / letterbox.geometry, the spec."""
    prog = r"""#include <stdio.h>
#include <stdlib.h>
#include "letterbox_tables.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const int src = atoi(argv[i]), dst = atoi(argv[i + 1]);
        const vgh_lb::AxisTables t = vgh_lb::axis_tables(src, dst);
        fwrite(t.ofs.data(), 4, dst, stdout);
        fwrite(t.coef.data(), 2, (size_t)dst * 8, stdout);
        const vgh_lb::Geometry g = vgh_lb::geometry(src, dst, 640);
        const int gi[4] = {g.new_h, g.new_w, g.pad_x, g.pad_y};
        fwrite(gi, 4, 4, stdout);
        fwrite(&g.scale, 8, 1, stdout);
    }
    return 0;
}
"""
    exe = _compile(tmp_path, "lb_tables", prog, "g++", ["-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "head_detector_amd", "csrc")])
    out = subprocess.run([exe] + [str(v) for p in _PAIRS for v in p], check=True, capture_output=True).stdout
    at = 0
    for src, dst in _PAIRS:
        ofs = np.frombuffer(out, np.int32, dst, at)
        at += 4 * dst
        coef = np.frombuffer(out, np.int16, dst * 8, at).reshape(dst, 8)
        at += 16 * dst
        geo = np.frombuffer(out, np.int32, 4, at)
        at += 16
        scale = float(np.frombuffer(out, np.float64, 1, at)[0])
        at += 8
        po, pc = axis_tables(src, dst)
        assert np.array_equal(ofs, po) and np.array_equal(coef, pc), (src, dst)
        assert (*geo.tolist(), scale) == geometry(src, dst, 640), (src, dst)
    assert at == len(out)
