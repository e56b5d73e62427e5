"""Host half of the on-screen display (head_detector_amd/overlay.py, include/vgh_osd.h): the ABI of libvghosd.so, its build declaration and source hygiene, the
font (header text = library = the module's mirror), the restatement (tests/osd_ref.py) against expectations written out BY HAND, the plan of a result's heads,
every refusal of the library, and csrc/osd_rules.h under the host sanitizers (tests/osd_host.hip: a program of its own, never run through Python, never on a GPU).
No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import osd_cases as oc  # noqa: E402
import osd_ref as ref  # noqa: E402

from head_detector_amd import _vgho, overlay, video  # noqa: E402
from head_detector_amd._lib import VghError  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.head_info import Bbox, HeadMetadata  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "head_detector_amd")
C = _vgho.C
WANT = {"vgho_version", "vgho_last_error", "vgho_workspace_bytes", "vgho_draw", "vgho_font"}


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def _head(x, y, w, h, score=0.9):
    return HeadMetadata(Bbox(x, y, w, h), score, None, None, None)


# ---- the library ----------------------------------------------------------------------------------------------------------------------------------
def test_osd_library_abi(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "vgh_osd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"VGHO_API [^;(]*?\b(vgho_[a-z0-9_]+)\s*\(", code))
    assert declared == WANT == set(_vgho.SYMBOLS)
    assert _exported(_vgho.LIB_PATH) == WANT  # hidden visibility: nothing of companion_host.h, no kernel stub
    assert _vgho.load().vgho_version().startswith(b"vghosd")
    for name, value in (("VGHO_MAX_SIDE", _vgho.MAX_SIDE), ("VGHO_MAX_COORD", _vgho.MAX_COORD), ("VGHO_MAX_ITEMS", _vgho.MAX_ITEMS), ("VGHO_MAX_PLANES", _vgho.MAX_PLANES),
                        ("VGHO_MAX_TEXT", _vgho.MAX_TEXT), ("VGHO_MAX_SCALE", _vgho.MAX_SCALE), ("VGHO_MAX_ALPHA", _vgho.MAX_ALPHA), ("VGHO_MAX_TILES", _vgho.MAX_TILES),
                        ("VGHO_GLYPHS", _vgho.GLYPHS), ("VGHO_GLYPH_ROWS", _vgho.GLYPH_ROWS), ("VGHO_GLYPH_COLS", _vgho.GLYPH_COLS), ("VGHO_GLYPH_PITCH", _vgho.GLYPH_PITCH),
                        ("VGHO_BAR", _vgho.BAR), ("VGHO_RECT", _vgho.RECT), ("VGHO_TEXT", _vgho.TEXT)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    assert (_vgho.MAX_SIDE, _vgho.MAX_COORD, _vgho.MAX_ITEMS, _vgho.MAX_TEXT, _vgho.MAX_SCALE, _vgho.MAX_ALPHA, _vgho.GLYPHS) == (32767, (1 << 24) - 1, 65536, 64, 16, 256, 44)
    # the structs, field for field, and the C layout from a compiled offsetof program
    structs = {"vgho_plane": [f for f, _ in _vgho.Plane._fields_], "vgho_job": [f for f, _ in _vgho.Job._fields_], "vgho_item": list(_vgho.ITEM_DTYPE.names)}
    offsets = {"vgho_plane": [C.sizeof(_vgho.Plane)] + [getattr(_vgho.Plane, f).offset for f, _ in _vgho.Plane._fields_],
               "vgho_job": [C.sizeof(_vgho.Job)] + [getattr(_vgho.Job, f).offset for f, _ in _vgho.Job._fields_],
               "vgho_item": [_vgho.ITEM_DTYPE.itemsize] + [_vgho.ITEM_DTYPE.fields[f][1] for f in _vgho.ITEM_DTYPE.names]}
    prog, want = "#include <stddef.h>\n#include <stdio.h>\n#include \"vgh_osd.h\"\nint main(void) {\n", []
    for cname, names in structs.items():
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        in_header = [n for decl in re.findall(r"[\w\s\*]+?([\w\s,\*\[\]]+);", fields) for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.replace("*", " "))]
        assert in_header == names, (cname, in_header)
        prog += f"    printf(\"%zu\\n\", sizeof({cname}));\n" + "".join(f"    printf(\"%zu\\n\", offsetof({cname}, {f}));\n" for f in names)
        want += offsets[cname]
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("gcc is needed to check the C side")
    src = tmp_path / "osd_layout.c"
    src.write_text(prog + "    return 0;\n}\n")
    exe = str(tmp_path / "osd_layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and (C.sizeof(_vgho.Plane), C.sizeof(_vgho.Job), _vgho.ITEM_DTYPE.itemsize) == (48, 184, 44)
    assert _vgho.ITEM_DTYPE["color"].shape == (3,) and _vgho.ITEM_DTYPE["color"].base == np.uint8 and _vgho.ITEM_DTYPE["x0"] == np.int32


def test_the_library_is_declared_in_the_build():
    from head_detector_amd import build

    assert build.OVERLAY == [build.Companion("libvghosd.so", ["osd.hip"], ["companion_host.h", "osd_rules.h", "plane_views.h"], "vgh_osd.h", [], "build_osd")]
    # the four older lists are what they were
    assert [c.lib for c in build.COMPANIONS] == ["libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghtex.so", "libvghvis.so", "libvghview.so"]
    assert build.APPLICATIONS == [build.Companion("libvghanon.so", ["anonymize.hip"], ["companion_host.h", "head_rows.h"], "vgh_anon.h", [], "build_anon")]
    assert build.VIDEO == [build.Companion("libvghvideo.so", ["yuv_anonymize.hip", "yuv_pack.hip"], ["companion_host.h", "head_rows.h", "plane_views.h"], "vgh_video.h", [], "build_video")]
    assert build.DOWNSTREAM == [build.Companion("libvghcrop.so", ["head_tensors.hip"], ["companion_host.h", "head_crop_rules.h"], "vgh_crop.h", ["-ffp-contract=off"], "build_crop")]
    assert "head_detector_amd/build_osd/" in open(os.path.join(ROOT, ".gitignore")).read().split()
    every = build.COMPANIONS + build.APPLICATIONS + build.VIDEO + build.DOWNSTREAM + build.OVERLAY
    assert len(every) == 10 and len({c.lib for c in every}) == 10 and len({c.objdir for c in every}) == 10  # with libvgh.so: eleven libraries
    assert "osd.hip" not in build.SOURCES and not build._needs_build(build.OVERLAY[0])
    # nobody else exports the prefix, it links none of the others, and no other binding names it
    libs = sorted(f for f in os.listdir(PKG) if f.startswith("libvgh") and f.endswith(".so") and f not in ("libvgh_exp.so", "libvgh_var.so"))
    assert set(libs) >= {"libvgh.so", "libvghview.so", "libvghvis.so", "libvghtex.so", "libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghanon.so", "libvghvideo.so",
                         "libvghcrop.so", "libvghosd.so"}
    for f in libs:
        if f != "libvghosd.so":
            assert not [s for s in _exported(os.path.join(PKG, f)) if s.startswith("vgho_")], f
    ldd = subprocess.run(["ldd", _vgho.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvgh" not in ldd
    for f in sorted(f for f in os.listdir(PKG) if f.startswith("_lib") and f.endswith(".py")) + ["_companion.py"]:
        text = open(os.path.join(PKG, f)).read()
        assert "libvghosd" not in text and "_vgho" not in text, f
    assert not os.path.basename(_vgho.__file__).startswith("_lib") and "_lib*.py" in _vgho.__doc__  # the module says why it is not named like the others


def test_source_hygiene():
    src = open(os.path.join(PKG, "csrc", "osd.hip")).read()
    rules = open(os.path.join(PKG, "csrc", "osd_rules.h")).read()
    hdr = open(os.path.join(ROOT, "include", "vgh_osd.h")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/vgh_osd.h", "companion_host.h", "osd_rules.h", "plane_views.h"]  # no other library's header
    assert "static_assert(VGHO_OK == OK && VGHO_ERR_INVALID == ERR_INVALID && VGHO_ERR_HIP == ERR_HIP && VGHO_ERR_NOMEM == ERR_NOMEM," in src
    # the rule header and the public header are HIP-free
    assert re.findall(r"#include\s+(\S+)", rules) == ["<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/vgh_osd.h"', '"plane_views.h"']
    assert re.findall(r"#include\s+(\S+)", hdr) == ["<stdint.h>"]
    for text in (rules, hdr):
        assert not [w for w in ("hip/", "hipLaunchKernelGGL", "__global__", "hipMemcpy", "hipGetDevice", "threadIdx", "atomicMax") if w in text], "HIP-free"
    # the single home of what must not exist twice
    for once in ("kFont[VGHO_GLYPHS][VGHO_GLYPH_ROWS] = {", "bool covers(", "uint32_t blend(", "Box grown_clipped(", "int64_t tile_count(", "int64_t workspace_bytes(", "const char* validate("):
        assert once in rules and once not in src, once
    assert "0x0e, 0x11" not in src and "0x0e, 0x11" not in hdr
    # a frame's planes addressed in place are csrc/plane_views.h's, shared with libvghvideo.so: generic (no public header, neither library's prefix), its host
    # part without the runtime
    shared = open(os.path.join(PKG, "csrc", "plane_views.h")).read()
    video = [open(os.path.join(PKG, "csrc", f)).read() for f in ("yuv_anonymize.hip", "yuv_pack.hip")]
    for once in ("struct Chan", "int pair_of(", "void plane_range(", "void copy_kernel(", "reinterpret_cast<const uint16_t*>", "bool in_place(", "null plane (src_dev",
                 "the destination overlaps source plane", "in place means exactly the source plane"):
        assert once in shared and not [t for t in (src, rules, *video) if once in t], once
    assert re.findall(r"#include\s+(\S+)", shared) == ["<stddef.h>", "<stdint.h>", "<stdio.h>"]
    assert "hip/" not in shared and "vgho_" not in shared.lower() and "vghy_" not in shared.lower() and "namespace planes {" in shared
    for by_hand in ("float", "double", "asm", "dlopen", "hipMalloc(", "hipHostMalloc(", "hipEventRecord(", "hipEventSynchronize(", "set_error(const char", "g_error", "__shared__",
                    "hipMemset"):
        assert by_hand not in src and by_hand not in rules and by_hand not in hdr, by_hand
    host = open(os.path.join(ROOT, "tests", "osd_host.hip")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["../head_detector_amd/csrc/osd_rules.h"] and "hip" not in " ".join(re.findall(r"#include <([^>]+)>", host))


def test_host_rules_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "osd_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "osd_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "osd host checks passed" in r.stdout, r.stdout + r.stderr


# ---- the font -------------------------------------------------------------------------------------------------------------------------------------
def test_font_is_one_table():
    parsed = ref.parse_font()
    assert parsed.shape == (44, 7) and np.array_equal(_vgho.font(), parsed) and np.array_equal(np.array(overlay.FONT, dtype=np.uint8), parsed)
    assert overlay.CHARS == ref.CHARS == " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#%.:-+/" and len(overlay.CHARS) == _vgho.GLYPHS
    assert (parsed < 32).all() and not parsed[0].any() and all(parsed[k].any() for k in range(1, 44))  # 5 columns; the space alone is empty
    assert len({parsed[k].tobytes() for k in range(44)}) == 44  # every glyph differs from every other, the digits among them
    digits = [parsed[k].tobytes() for k in range(1, 11)]
    assert len(set(digits)) == 10
    lib = _vgho.load()
    rows = (C.c_uint8 * 7)()
    for code in (-1, 44, 255, 1 << 20):
        assert lib.vgho_font(code, C.byref(rows)) == -1 and b"outside the font" in lib.vgho_last_error()
    assert lib.vgho_font(0, None) == -1 and b"null rows_out" in lib.vgho_last_error()
    assert overlay.encode("id 7: ok?") == [ref.CHARS.index(c) for c in "ID 7: OK "] == ref.encode("id 7: ok?")  # lower case -> upper case, anything else -> space
    assert overlay.text_size("#7 93%", 2) == (6 * 2 * 6 - 2, 14) == ref.text_size(6, 2)


# ---- the restatement against expectations written by hand -----------------------------------------------------------------------------------------------------
ONE = ["..#..",
       ".##..",
       "..#..",
       "..#..",
       "..#..",
       "..#..",
       ".###."]


def _bits(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def test_restatement_against_hand_written_expectations():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (12, 17), dtype=np.uint8)
    # an opaque BAR is a slice assignment; clipped by the target
    got, = ref.render([src], (0,), 12, 17, [ref.bar((3, 2, 9, 7), (200,), 256), ref.bar((14, 10, 30, 30), (7,), 256), ref.bar((-4, -4, 2, 1), (9,), 256)])
    want = src.copy()
    want[2:7, 3:9], want[10:, 14:], want[:1, :2] = 200, 7, 9
    assert np.array_equal(got, want)
    # "1" at scale 1 and at scale 2
    K = ref.key_plane(9, 8, [ref.text(1, 1, "1", (0,), 1)])
    want = np.zeros((9, 8), dtype=bool)
    want[1:8, 1:6] = _bits(ONE)
    assert np.array_equal(K == 1, want) and set(np.unique(K)) == {0, 1}
    K = ref.key_plane(16, 12, [ref.text(1, 1, "1", (0,), 2)])
    want = np.zeros((16, 12), dtype=bool)
    want[1:15, 1:11] = np.repeat(np.repeat(_bits(ONE), 2, axis=0), 2, axis=1)
    assert np.array_equal(K == 1, want)
    # two glyphs: the sixth column between them is blank
    K = ref.key_plane(7, 11, [ref.text(0, 0, "11", (0,), 1)])
    assert np.array_equal(K == 1, np.concatenate([_bits(ONE), np.zeros((7, 1), dtype=bool), _bits(ONE)], axis=1))
    # a thickness-1 RECT on a 5 x 4 box
    K = ref.key_plane(6, 7, [ref.rect((1, 1, 6, 5), (0,), 1)])
    assert np.array_equal(K == 1, _bits([".......",
                                         ".#####.",
                                         ".#...#.",
                                         ".#...#.",
                                         ".#####.",
                                         "......."]))
    assert (ref.key_plane(6, 7, [ref.rect((1, 1, 6, 5), (0,), 2)])[1:5, 1:6] == 1).all()  # half the shorter side fills it
    # the blend
    assert int(ref.blend(10, 200, 128)) == (10 * 128 + 200 * 128 + 128) >> 8 == 105
    assert int(ref.blend(10, 200, 256)) == 200 and int(ref.blend(10, 200, 0)) == 10 and int(ref.blend(255, 255, 1)) == 255
    got, = ref.render([np.full((3, 3), 10, np.uint8)], (0,), 3, 3, [ref.bar((0, 0, 3, 3), (200,), 128)])
    assert (got == 105).all()
    # the topmost item is blended against the SOURCE only; a transparent top item owns its pixels and leaves them as the source
    got, = ref.render([np.full((4, 4), 10, np.uint8)], (0,), 4, 4, [ref.bar((0, 0, 4, 4), (90,), 256), ref.bar((1, 1, 3, 3), (200,), 128), ref.bar((2, 2, 4, 4), (77,), 0)])
    assert got.tolist() == [[90, 90, 90, 90], [90, 105, 105, 90], [90, 105, 10, 10], [90, 90, 10, 10]]
    # a 1-pixel luma item at odd (x, y) owns exactly one chroma sample; the latest item that touches a chroma sample's four pixels owns it
    y, u = np.zeros((6, 6), np.uint8), np.zeros((3, 3), np.uint8)
    gy, gu, gv = ref.render([y, u, u], (0, 1, 1), 6, 6, [ref.bar((3, 3, 4, 4), (50, 60, 70), 256)])
    assert gy.sum() == 50 and gy[3, 3] == 50 and gu.sum() == 60 and gu[1, 1] == 60 and gv.sum() == 70 and gv[1, 1] == 70
    gy, gu, gv = ref.render([y, u, u], (0, 1, 1), 6, 6, [ref.bar((0, 0, 6, 6), (1, 2, 3), 256), ref.bar((3, 3, 5, 5), (50, 60, 70), 256)])
    assert (gu == [[2, 2, 2], [2, 60, 60], [2, 60, 60]]).all() and (gy == 50).sum() == 4  # odd edges: four chroma samples for four luma pixels
    # an odd target: the last chroma row and column serve one luma row and column
    o = ref.owner(ref.key_plane(3, 5, [ref.bar((4, 2, 5, 3), (0, 0, 0), 256)]), 1)
    assert o.shape == (2, 3) and o.tolist() == [[-1, -1, -1], [-1, -1, 0]]
    # a grey item on a frame gives U = V = 128
    for matrix in video.MATRICES:
        for full in (False, True):
            for c in (0, 1, 77, 128, 254, 255):
                assert video.rgb_to_yuv((c, c, c), matrix, full)[1:] == (128, 128)
    assert video.rgb_to_yuv((255, 255, 255), "bt709", True)[0] == 255 and video.rgb_to_yuv((0, 0, 0), "bt709", False)[0] == 16


def test_every_planted_case_contains_what_it_claims():
    cases = oc.cases()
    assert {c["shape"] for c in cases.values()} == {(97, 131), (64, 64), (2, 2), (1, 1)}
    for name, case in cases.items():  # the restatement takes every case on both kinds of target; nothing drawn = nothing changed
        for layout in ("nv12", "rgb"):
            src, want = oc.expected(name, case, layout)
            drawn = any((ref.key_plane(*case["shape"], [it]) > 0).any() and it["alpha"] > 0 for it in case["items"])
            assert drawn or all(np.array_equal(a, b) for a, b in zip(src, want)), name
    assert len(cases["many_heads"]["items"]) == 900 and cases["many_heads"]["shape"] == (64, 64) and cases["no_items"]["items"] == []
    parity = {tuple(v & 1 for v in it["box"]) for it in cases["odd"]["items"]}
    assert len(parity) == 16  # x0, y0, x1, y1 odd or even in every combination
    every = [it for c in cases.values() for it in c["items"]]
    assert {it["alpha"] for it in every} >= {0, 1, 128, 255, 256} and {it["kind"] for it in every} == {"bar", "rect", "text"}
    texts = [it for it in cases["text"]["items"]]
    assert {it["scale"] for it in texts} == {1, 2, 3, 16} and max(len(it["codes"]) for it in texts) == 64
    assert sorted(c for it in texts[:2] for c in it["codes"]) == list(range(44))  # every glyph once
    h, w = cases["text"]["shape"]
    assert any(it["box"][0] < 0 for it in texts) and any(it["box"][1] < 0 for it in texts) and any(it["box"][2] > w for it in texts) and any(it["box"][3] > h for it in texts)
    edges = cases["edges"]["items"]
    assert any(it["box"][2] <= 0 or it["box"][0] >= w for it in edges) and any(it["box"][0] == it["box"][2] for it in edges) and min(it["box"][0] for it in edges) < -(1 << 22)
    rects = cases["rects"]["items"]
    sides = [(it["thickness"], min(it["box"][2] - it["box"][0], it["box"][3] - it["box"][1])) for it in rects]
    assert any(t == 1 for t, _ in sides) and any(2 * t == s for t, s in sides) and any(t > s for t, s in sides)
    # the stack: the transparent item on top shows the source, not the items below it
    src, want = oc.expected("stack", cases["stack"], "nv12")
    K = ref.key_plane(97, 131, cases["stack"]["items"])
    top = K == 11  # item 10: the transparent bar
    assert top.any() and np.array_equal(want[0][top], src[0][top]) and not np.array_equal(want[0], src[0])
    # what a surface is: planes by meaning, sentinels everywhere else
    for layout in oc.LAYOUTS:
        for pitched in (False, True):
            planes = oc.content((97, 131), layout, 3)
            buf, geom = oc.surface((97, 131), layout, pitched, planes, 3)
            assert all(np.array_equal(v, p) for v, p in zip(oc.views(buf, geom), planes)), layout
            covered = np.zeros(geom["size"], dtype=bool)
            for v in oc.views(covered, geom):
                assert not v.any()  # no two planes share a byte
                v[...] = True
            assert (~covered).sum() >= 8 and (pitched is False or (~covered).sum() > 97 * 10), layout


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------
def _rows(items):
    return items.rows(), items.codes()


def test_plan_of_a_results_heads():
    heads = [_head(10, 40, 30, 20, 0.934), _head(50, 0, 20, 25, 0.5), _head(5, 8, 10, 10, 0.071)]
    ids = np.array([7, 23, 16], dtype=np.int64)
    shape = (100, 120, 3)
    p = overlay.head_overlay_plan(shape, heads, labels="id+score", track_ids=ids)
    rows, codes = _rows(p)
    assert len(p) == 9 and rows["kind"].tolist() == [_vgho.RECT, _vgho.BAR, _vgho.TEXT] * 3  # per head: the box, the bar, the text
    text = lambda k: "".join(overlay.CHARS[c] for c in codes[rows["code_offset"][k]:rows["code_offset"][k] + rows["length"][k]])  # noqa: E731
    assert [text(k) for k in (2, 5, 8)] == ["#7 93%", "#23 50%", "#16 7%"]
    assert [text(k) for k in (2, 5, 8)] != [] and overlay.head_overlay_plan(shape, heads, labels="id", track_ids=ids).codes().tolist() == overlay.encode("#7#23#16")
    assert overlay.head_overlay_plan(shape, heads, labels="score").codes().tolist() == overlay.encode("93%50%7%")
    assert overlay.head_overlay_plan(shape, heads, labels="id").codes().tolist() == overlay.encode("#0#1#2")  # no ids: the head's index
    assert overlay.head_overlay_plan(shape, heads, labels=["a", "B c", "-"]).codes().tolist() == overlay.encode("AB C-")
    box = lambda k: (int(rows["x0"][k]), int(rows["y0"][k]), int(rows["x1"][k]), int(rows["y1"][k]))  # noqa: E731
    # auto: min(100, 120) // 360 = 0 -> 1
    assert rows["thickness"][0] == 1 and rows["scale"][2] == 1
    assert box(0) == (10, 40, 40, 60) and box(3) == (50, 0, 70, 25)
    tw, th = overlay.text_size("#7 93%", 1)
    assert box(1) == (10, 40 - 9, 10 + tw + 2, 40) and box(2) == (11, 32, 11 + tw, 32 + 7)  # above the box: 7 s + 2 s high, left-aligned
    tw, _ = overlay.text_size("#23 50%", 1)
    assert box(4) == (50, 0, 50 + tw + 2, 9) and box(5) == (51, 1, 51 + tw, 8)  # the box is at row 0: inside its top
    assert box(7) == (5, 8, 5 + overlay.text_size("#16 7%", 1)[0] + 2, 17)  # 8 - 9 < 0: inside as well
    assert rows["color"][0].tolist() == list(overlay.PALETTE[7]) and rows["color"][3].tolist() == list(overlay.PALETTE[23 % 16]) and rows["color"][6].tolist() == list(overlay.PALETTE[0])
    assert rows["color"][1].tolist() == rows["color"][0].tolist() and len(overlay.PALETTE) == 16 and len(set(overlay.PALETTE)) == 16
    assert (rows["alpha"] == 256).all()
    # scale and thickness: "auto" on a 4K frame, or given
    big = overlay.head_overlay_plan((2160, 3840), heads[:1], labels="id", track_ids=[3]).rows()
    assert big["thickness"][0] == 6 and big["scale"][2] == 6 and (big["y1"][1] - big["y0"][1]) == 9 * 6
    given = overlay.head_overlay_plan(shape, heads[:1], labels="id", thickness=3, text_scale=2).rows()
    assert given["thickness"][0] == 3 and given["scale"][2] == 2 and (given["x0"][2], given["y0"][2]) == (12, 40 - 18 + 2)
    # alphas and coasting tracks
    faded = overlay.head_overlay_plan(shape, heads, labels="id", alpha=0.5, label_alpha=1.0, track_ids=ids, coasting=[False, True, False], coasting_alpha=0.5).rows()
    assert faded["alpha"].tolist() == [128, 256, 256, 64, 128, 128, 128, 256, 256]
    # boxes or labels alone, colours given
    assert overlay.head_overlay_plan(shape, heads, boxes=False, labels="id").rows()["kind"].tolist() == [_vgho.BAR, _vgho.TEXT] * 3
    only = overlay.head_overlay_plan(shape, heads, colors=(1, 2, 3)).rows()
    assert only["kind"].tolist() == [_vgho.RECT] * 3 and only["color"].tolist() == [[1, 2, 3]] * 3
    assert overlay.head_overlay_plan(shape, heads, colors=[(1, 2, 3), (4, 5, 6), (7, 8, 9)]).rows()["color"].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert len(overlay.head_overlay_plan(shape, [])) == 0
    # fractional boxes are rounded half up, corner by corner
    assert overlay.head_overlay_plan(shape, [_head(1.5, 2.49, 3.0, 4.0)]).rows()[["x0", "y0", "x1", "y1"]].tolist() == [(2, 2, 5, 6)]


def test_argument_errors_and_their_order():
    heads = [_head(10, 40, 30, 20), _head(50, 0, 20, 25)]
    image = np.zeros((60, 80, 3), np.uint8)
    res = PredictionResult(image, heads)
    for kw, words in ((dict(labels="name"), "labels"), (dict(labels=["a"]), "labels"), (dict(labels=["a", ""]), "labels"), (dict(colors="rainbow"), "colors"),
                      (dict(colors=(1, 2)), "colors"), (dict(colors=(1, 2, 256)), "colors"), (dict(colors=[(1, 2, 3)]), "colors"), (dict(thickness=0), "thickness"),
                      (dict(thickness=1.5), "thickness"), (dict(text_scale=0), "text_scale"), (dict(text_scale=17), "text_scale"), (dict(text_scale="big"), "text_scale"),
                      (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(label_alpha=-0.1), "label_alpha"), (dict(coasting_alpha=2), "coasting_alpha"),
                      (dict(track_ids=[1]), "track_ids"), (dict(track_ids=[1, -2]), "track_ids"), (dict(coasting=[True]), "coasting"), (dict(boxes="yes"), "boxes")):
        for call in (lambda **k: overlay.head_overlay_plan(image.shape, heads, **k), lambda **k: overlay.draw_heads(image, heads, **k), lambda **k: res.draw_overlay(**k)):
            with pytest.raises(ValueError, match=words):  # before any GPU is looked for
                call(**kw)
    with pytest.raises(ValueError, match="shape"):
        overlay.head_overlay_plan((0, 10), heads)
    with pytest.raises(ValueError, match="shape"):
        overlay.head_overlay_plan(None, heads)
    items = overlay.Items()
    for call, words in ((lambda: items.bar((0, 0, 1), (1, 2, 3)), "box"), (lambda: items.bar((0, 0, 1.5, 2), (1, 2, 3)), "box"), (lambda: items.bar((5, 0, 4, 2), (1, 2, 3)), "box"),
                        (lambda: items.bar((0, 0, 40000, 2), (1, 2, 3)), "box"), (lambda: items.bar((1 << 24, 0, (1 << 24) + 1, 2), (1, 2, 3)), "box"),
                        (lambda: items.bar((0, 0, 1, 1), (1, 2)), "color"), (lambda: items.bar((0, 0, 1, 1), (1.0, 2, 3)), "color"), (lambda: items.bar((0, 0, 1, 1), (1, 2, 3), 1.01), "alpha"),
                        (lambda: items.rect((0, 0, 9, 9), (1, 2, 3), 0), "thickness"), (lambda: items.text(0, 0, "", (1, 2, 3), 1), "string"),
                        (lambda: items.text(0, 0, "x" * 65, (1, 2, 3), 1), "string"), (lambda: items.text(0, 0, "x", (1, 2, 3), 17), "scale"),
                        (lambda: items.text(0.5, 0, "x", (1, 2, 3), 1), "x and y"), (lambda: overlay.text_size("x", 0), "scale")):
        with pytest.raises(ValueError, match=words):
            call()
    assert len(items) == 0 and len(items.bar((0, 0, 1, 1), (1, 2, 3)).rect((0, 0, 9, 9), (1, 2, 3), 2, 0.5).text(3, 4, "ok", (9, 9, 9), 2)) == 3
    assert items.rows()["alpha"].tolist() == [256, 128, 256]
    for bad, words in ((np.zeros((40, 50), np.uint8), "target"), (np.zeros((40, 50, 3), np.float32), "target"), (np.zeros((40, 50, 4), np.uint8), "target"), (None, "target"),
                       ("image.png", "target")):
        with pytest.raises(ValueError, match=words):
            overlay.render(bad, items)
    with pytest.raises(ValueError, match="items"):
        overlay.render(image, [])
    with pytest.raises(ValueError, match="out"):
        overlay.render(image, items, out=np.zeros((60, 80, 3), np.uint8))
    with pytest.raises(ValueError, match="neither"):
        PredictionResult(None, heads).draw_overlay()
    with pytest.raises(ValueError, match="to_host"):
        res.draw_overlay(to_host="yes")
    if not torch.cuda.is_available():  # and only then the missing GPU
        with pytest.raises(VghError, match="need a GPU"):
            overlay.render(image, items)
        with pytest.raises(VghError, match="need a GPU"):
            res.draw_overlay(labels="score")
        y, u = torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((2, 3), dtype=torch.uint8)
        frame = video.YUV420Frame(y, u, u.clone(), chroma_step=1)
        with pytest.raises(ValueError, match="out must be a YUV420Frame"):
            overlay.render(frame, items, out=y)
        with pytest.raises(VghError, match="need a GPU"):
            overlay.render(frame, items, out=frame)
        with pytest.raises(VghError, match="need a GPU"):
            PredictionResult(None, heads, source_frame=frame).draw_overlay(labels="id", out=frame)
    # the tracker's results carry the method too, and pass their ids by themselves
    from head_detector_amd.tracking import TrackedPredictionResult

    assert TrackedPredictionResult.draw_overlay is PredictionResult.draw_overlay


# ---- every refusal of the library, without a GPU ----------------------------------------------------------------------------------------------------------
def test_an_invalid_job_is_refused_before_a_gpu_is_looked_for():
    lib = _vgho.load()
    mem = np.zeros(1 << 16, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16
    rows = np.zeros(3, _vgho.ITEM_DTYPE)
    rows[0] = (_vgho.BAR, 1, 1, 30, 20, 0, 0, 0, 0, 256, (1, 2, 3), 0)
    rows[1] = (_vgho.RECT, 2, 2, 9, 9, 1, 0, 0, 0, 128, (1, 2, 3), 0)
    rows[2] = (_vgho.TEXT, 0, 0, 22, 14, 0, 2, 2, 2, 256, (1, 2, 3), 0)
    codes = np.array([2, 0, 43, 11], dtype=np.uint8)

    def job(table=rows, glyphs=codes, planes=(), **over):
        j = _vgho.Job()
        j.height, j.width, j.n_planes, j.n_items, j.items, j.codes, j.n_codes = 20, 30, 3, len(table), table.ctypes.data, glyphs.ctypes.data, len(glyphs)
        for k in range(3):
            p = j.planes[k]
            p.src_dev = p.dst_dev = base + 16384 + (1024 + (k - 1) if k else 0)
            p.src_pitch = p.dst_pitch = 32
            p.src_step = p.dst_step = 2 if k else 1
            p.shift = 1 if k else 0
        for k, field, value in planes:
            setattr(j.planes[k], field, value)
        for k, v in over.items():
            setattr(j, k, v)
        return j

    def item(k, **over):
        changed = rows.copy()
        for name, v in over.items():
            changed[name][k] = v
        return changed

    assert lib.vgho_workspace_bytes(job()) == 4 * 20 * 30 and lib.vgho_workspace_bytes(job(height=1, width=1)) == 16
    refusals = [(dict(height=0), b"target 0 x 30"), (dict(width=32768), b"target 20 x 32768"), (dict(n_planes=0), b"n_planes 0"), (dict(n_planes=4), b"n_planes 4"),
                (dict(n_items=65537), b"n_items 65537"), (dict(items=None), b"null items"), (dict(codes=None), b"item 2: null codes"), (dict(n_codes=3), b"outside the 3 codes"),
                (dict(reserved=5), b"reserved is 5"), (dict(planes=[(1, "shift", 2)]), b"plane 1: shift 2"), (dict(planes=[(2, "src_step", 4)]), b"plane 2: steps 4 and 2"),
                (dict(planes=[(0, "src_pitch", 29)]), b"plane 0: src_pitch 29"), (dict(planes=[(1, "dst_pitch", 28)]), b"plane 1: dst_pitch 28"),
                (dict(planes=[(2, "dst_dev", None)]), b"plane 2: null plane"), (dict(planes=[(0, "reserved", 1)]), b"plane 0: reserved"),
                (dict(planes=[(0, "dst_pitch", 40)]), b"in place means exactly the source plane"), (dict(planes=[(0, "dst_dev", base + 16384 + 8)]), b"plane 0: the destination overlaps source plane 0"),
                (dict(table=item(0, kind=3)), b"item 0: unknown kind 3"), (dict(table=item(1, thickness=0)), b"item 1: thickness 0"), (dict(table=item(0, alpha=257)), b"item 0: alpha 257"),
                (dict(table=item(1, alpha=-1)), b"item 1: alpha -1"), (dict(table=item(0, x1=0)), b"item 0: box sides -1 x 19"), (dict(table=item(0, y1=32769)), b"item 0: box sides 29 x 32768"),
                (dict(table=item(0, x0=-(1 << 24))), b"item 0: box coordinate -16777216"), (dict(table=item(0, reserved=1)), b"item 0: reserved"),
                (dict(table=item(2, scale=0)), b"item 2: scale 0"), (dict(table=item(2, scale=17)), b"item 2: scale 17"), (dict(table=item(2, length=65)), b"item 2: length 65"),
                (dict(table=item(2, code_offset=-1)), b"item 2: code_offset -1"), (dict(table=item(2, x1=23)), b"item 2: box 23 x 14 of a TEXT is not its run's size 22 x 14"),
                (dict(glyphs=np.array([2, 0, 44, 11], dtype=np.uint8)), b"item 2: code 44 (at 2) outside the font")]
    for over, words in refusals:
        j = job(**over)
        assert lib.vgho_workspace_bytes(j) == 0 and words in lib.vgho_last_error(), (words, lib.vgho_last_error())
        assert lib.vgho_draw(j, base, None) == -1 and words in lib.vgho_last_error(), (words, lib.vgho_last_error())
    assert lib.vgho_workspace_bytes(None) == 0 and b"null job" in lib.vgho_last_error()
    assert lib.vgho_draw(None, base, None) == -1 and b"null job" in lib.vgho_last_error()
    assert lib.vgho_draw(job(), None, None) == -1 and b"null workspace" in lib.vgho_last_error()
    assert lib.vgho_draw(job(), base + 4, None) == -1 and b"workspace is not 16-byte aligned" in lib.vgho_last_error()
    many = np.zeros(65536, _vgho.ITEM_DTYPE)
    many["x1"], many["y1"], many["alpha"] = 272, 272, 256
    big = [(k, f, 272) for k in range(3) for f in ("src_pitch", "dst_pitch")]
    assert lib.vgho_workspace_bytes(job(table=many, height=272, width=272, planes=big)) == 0 and b"tiles exceed one launch" in lib.vgho_last_error()
    assert lib.vgho_workspace_bytes(job(table=many[:58052], height=272, width=272, planes=big)) == (4 * 272 * 272)
    # nothing to draw and nothing to copy: accepted, and nothing is queued (no GPU is looked for)
    assert lib.vgho_draw(job(n_items=0), base, None) == 0
    outside = rows[:1].copy()
    outside["x0"], outside["x1"] = 100, 129
    assert lib.vgho_draw(job(table=outside), base, None) == 0
    assert not mem.any()
