"""Host half of csrc/tile_fold.h (TileLists, first_bad_bound, first_bad_index) against brute force, under the host sanitizers: tests/tile_fold_host.hip is
a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU (it makes no HIP
call).  Also: the pieces the three raster libraries share are defined once."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "head_detector_amd", "csrc")


def test_tile_lists_and_scans_match_brute_force_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "tile_fold_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "tile_fold_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tile_fold host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_shared_pieces_are_defined_once():
    # csrc/raster.hip (libvgh.so) is another algorithm, atomic max then resolve, with a set-up of its own: not part of this
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")) and f != "raster.hip"}
    for piece in ("struct alignas(8) Box", "void boxes_kernel(", "void tri_setup(", "#define compact_hits(", "__ballot(hit)", "grid[(size_t)ty * tiles_x + tx]++;", "struct TileLists", "struct State {"):
        where = [f for f, s in text.items() for _ in range(s.count(piece))]
        assert where == ["tile_fold.h"], (piece, where)
    for f in ("mesh_render.hip", "visibility.hip", "texture.hip"):
        s = text[f]
        assert '#include "tile_fold.h"' in s and "#pragma clang fp contract(off)" in s and "compact_hits(" in s
        assert re.search(r"static_assert\(VGH\w+_OK == OK && VGH\w+_ERR_INVALID == ERR_INVALID && VGH\w+_ERR_HIP == ERR_HIP && VGH\w+_ERR_NOMEM == ERR_NOMEM", s), f
    assert "#pragma clang fp contract(off)" in text["tile_fold.h"]
