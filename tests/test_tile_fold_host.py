"""Host half of csrc/tile_fold.h (TileLists, first_bad_bound, first_bad_index) against brute force, and what csrc/companion_host.h does without the runtime
(align16, the require macro and the message, the queue macro), under the host sanitizers: tests/tile_fold_host.hip is
a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU (it makes no HIP
call).  Also: the pieces the three raster libraries share, and the host plumbing all four companion libraries share, are defined once."""
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


COMPANION_SOURCES = ("aligned.hip", "draw.hip", "mesh_render.hip", "visibility.hip", "texture.hip", "mesh_metrics.hip")


def test_the_shared_pieces_are_defined_once():
    # csrc/raster.hip (libvgh.so) is another algorithm, atomic max then resolve, with a set-up of its own: not part of this
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")) and f != "raster.hip"}

    def homes(piece, skip=()):
        return [f for f, s in text.items() if f not in skip for _ in range(s.count(piece))]

    for piece in ("struct alignas(8) Box", "void boxes_kernel(", "void tri_setup(", "#define compact_hits(", "__ballot(hit)", "grid[(size_t)ty * tiles_x + tx]++;", "struct TileLists", "struct State ",
                  "int first_bad_bound(", "int64_t first_bad_index(", "constexpr int TILE ", "constexpr float BACKGROUND "):
        assert homes(piece) == ["tile_fold.h"], (piece, homes(piece))
    # the host plumbing of the four companion libraries; the core (libvgh.so) has its own message in vgh_internal.h / net.hip
    core = ("vgh_internal.h", "net.hip")
    for piece in ("struct Staging {", "int reserve(Staging&", "int finish(", "thread_local char", "vsnprintf(", "struct Queue {", "struct Scratch {", "bool grow(", "#define CH_HIP(",
                  "#define CH_REQUIRE(", "#define CH_QUEUE(", "constexpr int OK = 0, ERR_INVALID = -1, ERR_HIP = -2, ERR_NOMEM = -3;"):
        assert homes(piece, core) == ["companion_host.h"], (piece, homes(piece, core))
    for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "size_t align16("):  # no companion source does these itself
        assert not [f for f in homes(by_hand) if f in COMPANION_SOURCES + ("tile_fold.h",)], (by_hand, homes(by_hand))
    for gone in ("VGHV_HIP", "VGHV_REQUIRE", "EV_HIP", "EV_REQUIRE", "TF_HIP", "TF_REQUIRE", "TF_QUEUE", "TILE_FOLD_SET_ERROR", "staging_reserve", "vghv_internal"):
        assert homes(gone) == [] and gone not in open(os.path.join(CSRC, "raster.hip")).read(), (gone, homes(gone))
    assert not os.path.exists(os.path.join(CSRC, "vghv_internal.h"))
    for f in ("mesh_render.hip", "visibility.hip", "texture.hip"):
        s = text[f]
        assert '#include "tile_fold.h"' in s and "#pragma clang fp contract(off)" in s and "compact_hits(" in s
    assert "#pragma clang fp contract(off)" in text["tile_fold.h"] and '#include "companion_host.h"' in text["tile_fold.h"]
    for f in COMPANION_SOURCES:  # every library's public codes are the shared ones (include/vgh_eval.h has no NOMEM: that library allocates nothing)
        s = text[f]
        assert '#include "companion_host.h"' in s or '#include "tile_fold.h"' in s, f
        nomem = "" if f == "mesh_metrics.hip" else r" && VGH\w+_ERR_NOMEM == ERR_NOMEM"
        assert re.search(r"static_assert\(VGH\w+_OK == OK && VGH\w+_ERR_INVALID == ERR_INVALID && VGH\w+_ERR_HIP == ERR_HIP" + nomem + ",", s), f
        assert "set_error(const char" not in s and "g_error" not in s, f
