"""Host half of head anonymisation in YUV planes and of the RGB packer (head_detector_amd/video.py, include/vgh_video.h): the ABI of libvghvideo.so, every
refusal of the C calls, the workspace size and the plan against hand-computed values, the packer's coefficients and their exhaustive properties, facts of the
restatement (tests/yuv_anonymize_ref.py), every planted case against what it claims to contain, and the host code of csrc/yuv_anonymize.hip and
csrc/yuv_pack.hip under the host sanitizers (tests/yuv_anonymize_host.hip: a program of its own, never run through Python, never on a GPU).  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_ref as ref  # noqa: E402
import yuv_anonymize_cases as yc  # noqa: E402
import yuv_anonymize_ref as yref  # noqa: E402
import yuv_ref  # noqa: E402

from head_detector_amd import _lib_anon, _lib_video, anonymize, video  # noqa: E402
from head_detector_amd._lib import VghError  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib_video.C
WANT = {"vghy_version", "vghy_last_error", "vghy_anonymize_workspace_bytes", "vghy_anonymize", "vghy_pack_rgb"}
SOURCES = ("yuv_anonymize.hip", "yuv_pack.hip")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


# ---- the library ----------------------------------------------------------------------------------------------------------------------------------
def test_video_library_abi(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "vgh_video.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghy_[a-z0-9_]+)\s*\(", code))
    assert declared == WANT == set(_lib_video.SYMBOLS)
    assert _exported(_lib_video.LIB_PATH) == WANT  # hidden visibility: nothing of companion_host.h, no kernel stub
    lib = _lib_video.load()
    assert lib.vghy_version().startswith(b"vghvideo")
    for name, value in (("VGHY_MAX_SIDE", _lib_video.MAX_SIDE), ("VGHY_MAX_COORD", _lib_video.MAX_COORD), ("VGHY_MAX_HEADS", _lib_video.MAX_HEADS), ("VGHY_MAX_CELLS", _lib_video.MAX_CELLS),
                        ("VGHY_MAX_RADIUS", _lib_video.MAX_RADIUS), ("VGHY_TAP_SUM", _lib_video.TAP_SUM), ("VGHY_METHOD_FILL", _lib_video.METHODS["fill"]),
                        ("VGHY_METHOD_PIXELATE", _lib_video.METHODS["pixelate"]), ("VGHY_METHOD_BLUR", _lib_video.METHODS["blur"]), ("VGHY_REGION_BOX", _lib_video.REGION_BOX),
                        ("VGHY_REGION_ELLIPSE", _lib_video.REGION_ELLIPSE), ("VGHY_REGION_MAP", _lib_video.REGION_MAP)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    # the caps, the methods and the regions are those of vgh_anon.h: the plan of one serves the other
    for name in ("MAX_SIDE", "MAX_COORD", "MAX_HEADS", "MAX_CELLS", "MAX_RADIUS", "TAP_SUM", "METHODS", "REGION_BOX", "REGION_ELLIPSE", "REGION_MAP", "HEAD_DTYPE"):
        assert getattr(_lib_video, name) == getattr(_lib_anon, name), name
    assert "vgh_anon.h" not in hdr.split("*/", 1)[1]  # the rule is written out, not referred to
    # the structs, field for field, and the C layout from a compiled offsetof program
    structs = {"vghy_plane": _lib_video.Plane, "vghy_anonymize_job": _lib_video.AnonymizeJob, "vghy_pack_job": _lib_video.PackJob}
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"vgh_video.h\"\nint main(void) {\n    printf(\"%zu\\n\", sizeof(vghy_head));\n"
    want = [_lib_video.HEAD_DTYPE.itemsize]
    for cname, cls in structs.items():
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        names = re.findall(r"(\w+)(?:\[\d+\])?;", fields)
        assert names == [f for f, _ in cls._fields_], cname
        prog += f"    printf(\"%zu\\n\", sizeof({cname}));\n" + "".join(f"    printf(\"%zu\\n\", offsetof({cname}, {f}));\n" for f in names)
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in names]
    row = re.search(r"typedef struct vghy_head \{(.*?)\} vghy_head;", code, flags=re.S).group(1)
    assert re.findall(r"int32_t ([^;]+);", row) == ["x0, y0, x1, y1", "cell", "radius", "tap_offset", "reserved"]
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("gcc is needed to check the C side")
    src = tmp_path / "video_layout.c"
    src.write_text(prog + "    return 0;\n}\n")
    exe = str(tmp_path / "video_layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and (C.sizeof(_lib_video.Plane), C.sizeof(_lib_video.AnonymizeJob), C.sizeof(_lib_video.PackJob)) == (40, 184, 184)


LUMA = [(10, 10, 60, 50, 7, 1, 0, 0), (-20, -5, 30, 40, 8, 0, 2, 0), (90, 80, 90, 95, 1, 1, 0, 0)]
CHROMA = [(5, 5, 30, 25, 4, 1, 0, 0), (-10, -3, 15, 20, 4, 0, 2, 0), (45, 40, 45, 48, 1, 1, 0, 0)]
Y_AT, UV_AT, OUT_AT, WS_AT = 0, 10240, 65536, 32768  # offsets in the block that stands for device memory


def _job(luma=None, chroma=None, table=None, planes=None, **over):
    """A valid in-place blur job on an NV12 frame of 97 x 100 in host memory that is never touched: the argument checks come first.  ``planes``:
    {index: {field: value}}, a tuple value being an offset from the block's base."""
    mem = np.zeros(1 << 17, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16
    luma = np.array(LUMA if luma is None else luma, dtype=_lib_video.HEAD_DTYPE)
    chroma = np.array(CHROMA if chroma is None else chroma, dtype=_lib_video.HEAD_DTYPE)
    table = np.array([65534, 1, 65536, 0] if table is None else table, dtype=np.int32)
    job = _lib_video.AnonymizeJob(height=97, width=100, n_heads=len(luma), method=2, region=1, color=0, luma_heads=luma.ctypes.data, chroma_heads=chroma.ctypes.data,
                                  taps=table.ctypes.data, n_taps=len(table), reserved=0, owner_dev=None)
    for k, (at, step) in enumerate(((Y_AT, 1), (UV_AT, 2), (UV_AT + 1, 2))):
        p = job.planes[k]
        p.src_dev = p.dst_dev = base + at
        p.src_pitch = p.dst_pitch = 104
        p.src_step = p.dst_step = step
    for k, fields in (planes or {}).items():
        for f, v in fields.items():
            setattr(job.planes[k], f, base + v[0] if isinstance(v, tuple) else v)
    for f, v in over.items():
        setattr(job, f, base + v[0] if isinstance(v, tuple) else v)
    job._keep = (mem, luma, chroma, table)
    return job, base


def test_workspace_bytes_of_hand_computed_jobs():
    lib = _lib_video.load()
    up = lambda v: (v + 15) & ~15  # noqa: E731
    owner = 4 * 97 * 100
    # blur: one byte a luma and two a chroma sample of the clipped boxes; the h rows: r = 1 adds a row above and below, u16 a luma sample and two a chroma sample
    values_l, values_c = 50 * 40 + 30 * 40, 2 * (25 * 20 + 15 * 20)
    h_l, h_c = 2 * (42 * 50 + 40 * 30), 4 * (22 * 25 + 20 * 15)
    assert lib.vghy_anonymize_workspace_bytes(_job()[0]) == up(up(up(up(owner) + values_l) + values_c) + h_l) + up(h_c)
    assert lib.vghy_anonymize_workspace_bytes(_job(method=0)[0]) == up(owner)
    assert lib.vghy_anonymize_workspace_bytes(_job(method=1)[0]) == up(up(owner + 8 * 6 + 7 * 6) + 2 * (7 * 5 + 7 * 6))  # the cells of the UNCLIPPED boxes that touch the plane
    assert lib.vghy_anonymize_workspace_bytes(_job(method=1, region=2, owner_dev=(64,))[0]) == up(up(8 * 6 + 7 * 6) + 2 * (7 * 5 + 7 * 6))
    empty = np.zeros(0, _lib_video.HEAD_DTYPE)
    assert lib.vghy_anonymize_workspace_bytes(_job(luma=empty, chroma=empty)[0]) == up(owner)  # no heads: the owner plane alone
    out_of_place = {0: dict(dst_dev=(OUT_AT,), dst_pitch=100), 1: dict(dst_dev=(OUT_AT + 9700,), dst_pitch=50, dst_step=1), 2: dict(dst_dev=(OUT_AT + 12150,), dst_pitch=50, dst_step=1)}
    assert lib.vghy_anonymize_workspace_bytes(_job(planes=out_of_place)[0]) == lib.vghy_anonymize_workspace_bytes(_job()[0])  # NV12 -> I420 elsewhere: the same
    for shape in ((1, 1), (97, 131), (3000, 4000)):
        far = {k: dict(dst_dev=(1 << 40,), src_pitch=8192, dst_pitch=8192) for k in range(3)}
        far[0]["dst_dev"], far[1]["dst_dev"], far[2]["dst_dev"] = ((1 << 40),), ((1 << 41),), ((1 << 41) + 1,)
        for k in range(3):
            far[k]["src_dev"] = ((1 << 42) + (k << 30) + (k == 2),)
        need = lib.vghy_anonymize_workspace_bytes(_job(planes=far, height=shape[0], width=shape[1])[0])
        assert need % 16 == 0 and need >= 16, lib.vghy_last_error()
    assert lib.vghy_anonymize_workspace_bytes(None) == 0 and b"null job" in lib.vghy_last_error()


def test_every_invalid_job_carries_its_message_and_needs_no_gpu():
    lib = _lib_video.load()

    def refused(words, ws=WS_AT, **kw):
        job, base = _job(**kw)
        rc = lib.vghy_anonymize(job, None if ws is None else base + ws, None)
        msg = lib.vghy_last_error()
        assert rc == -1 and words in msg, (words, rc, msg)
        if ws == WS_AT:
            assert lib.vghy_anonymize_workspace_bytes(job) == 0, words
        assert not job._keep[0].any()

    assert lib.vghy_anonymize(None, None, None) == -1 and b"null job" in lib.vghy_last_error()
    refused(b"null workspace", ws=None)
    refused(b"workspace is not 16-byte aligned", ws=WS_AT + 8)
    for planes, words in (({0: dict(src_dev=None)}, b"plane Y: null plane"), ({2: dict(dst_dev=None)}, b"plane V: null plane"), ({1: dict(src_step=3)}, b"plane U: steps 3 and 2 are not 1 or 2"),
                          ({0: dict(dst_step=0)}, b"plane Y: steps 1 and 0"), ({0: dict(src_pitch=99)}, b"plane Y: src_pitch 99 outside 100"),
                          ({1: dict(dst_pitch=98)}, b"plane U: dst_pitch 98 outside 99"),
                          # in place means exactly the source plane: the same pointer with another pitch or step is refused
                          ({0: dict(dst_pitch=105)}, b"plane Y: the destination starts where the source does with another pitch or step"),
                          ({1: dict(dst_step=1)}, b"plane U: the destination starts where the source does"),
                          # a partial overlap of a destination with any source plane
                          ({0: dict(dst_dev=(Y_AT + 104,))}, b"plane Y: the destination overlaps source plane Y"), ({0: dict(dst_dev=(UV_AT - 104,))}, b"plane Y: the destination overlaps source plane U"),
                          ({2: dict(dst_dev=(UV_AT + 3,))}, b"plane V: the destination overlaps source plane U"),
                          ({1: dict(dst_dev=(Y_AT + 96 * 104 + 99,), dst_pitch=50, dst_step=1)}, b"plane U: the destination overlaps source plane Y")):
        refused(words, planes=planes)
    for over, words in ((dict(height=0), b"frame 0 x 100"), (dict(width=32768), b"outside 1 .. 32767"), (dict(n_heads=-1), b"n_heads -1"), (dict(n_heads=65537), b"n_heads 65537 outside 0 .. 65536"),
                        (dict(method=3), b"unknown method 3"), (dict(method=-1), b"unknown method -1"), (dict(region=3), b"unknown region 3"), (dict(color=1 << 24), b"color"),
                        (dict(reserved=2), b"reserved is 2"), (dict(region=2), b"owner_dev is null"), (dict(owner_dev=(64,)), b"owner_dev is set"),
                        (dict(region=2, owner_dev=(68,)), b"not 16-byte aligned"), (dict(luma_heads=None), b"null heads"), (dict(chroma_heads=None), b"null heads"),
                        (dict(taps=None), b"blur needs a tap table"), (dict(n_taps=0), b"blur needs a tap table"), (dict(n_taps=-1), b"n_taps -1"),
                        (dict(n_taps=2), b"luma head 1: taps 2 .. 2 outside the table of 2")):
        refused(words, **over)
    ok = (0, 0, 50, 50, 1, 0, 2, 0)
    for group in ("luma", "chroma"):  # the caps and the taps, in either plane group
        name = group.encode()
        for rows, method, words in (([ok, (1 << 24, 0, (1 << 24) + 5, 5, 1, 0, 2, 0)], 2, b" head 1: corner"), ([(0, 0, 32768, 5, 1, 0, 2, 0)], 2, b" head 0: box sides 32768 x 5"),
                                    ([ok, ok, (5, 5, 4, 9, 1, 0, 2, 0)], 0, b" head 2: box sides -1 x 4"), ([ok, (0, 0, 5, 5, 1, 0, 2, 3)], 0, b" head 1: reserved"),
                                    ([ok, (0, 0, 50, 50, 0, 0, 2, 0)], 1, b" head 1: cell side 0"), ([ok, ok, (0, 0, 130, 50, 2, 0, 2, 0)], 1, b" head 2: 65 x 25 cells of side 2 exceed 64"),
                                    ([(0, 0, 50, 50, 1, 1025, 0, 0)], 2, b" head 0: radius 1025 outside 0 .. 1024"), ([ok, (0, 0, 50, 50, 1, -1, 0, 0)], 2, b" head 1: radius -1"),
                                    ([ok, (0, 0, 50, 50, 1, 1, 3, 0)], 2, b" head 1: taps 3 .. 4 outside the table of 4"), ([ok, ok, (0, 0, 50, 50, 1, 0, -1, 0)], 2, b" head 2: taps -1"),
                                    ([ok, (0, 0, 50, 50, 1, 1, 1, 0)], 2, b" head 1: tap sum 131073 is not 65536"), ([ok, ok, (0, 0, 50, 50, 1, 0, 3, 0)], 2, b" head 2: tap sum 0 is not 65536")):
            fine = [ok] * len(rows)
            refused(name + words, method=method, **{group: rows, "chroma" if group == "luma" else "luma": fine})
    refused(b"chroma head 1: tap 1 is -1", luma=[ok, ok], chroma=[ok, (0, 0, 50, 50, 1, 1, 2, 0)], table=[65534, 1, 65536, -1])
    # the most boxes one launch takes: 65536 heads of the largest box on the largest frame
    big = np.zeros(65536, _lib_video.HEAD_DTYPE)
    big["x1"], big["y1"], big["tap_offset"] = 32767, 32767, 2
    far = {0: dict(src_pitch=32768, dst_pitch=32768), 1: dict(src_dev=(1 << 40,), dst_dev=(1 << 40,), src_pitch=32768, dst_pitch=32768),
           2: dict(src_dev=((1 << 40) + 1,), dst_dev=((1 << 40) + 1,), src_pitch=32768, dst_pitch=32768)}
    refused(b"exceed one launch", luma=big, chroma=np.zeros(65536, _lib_video.HEAD_DTYPE), height=32767, width=32767, planes=far)


def _pack_job(planes=None, **over):
    mem = np.zeros(1 << 17, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16
    job = _lib_video.PackJob(src_dev=base, src_pitch_bytes=304, height=97, width=100, y_offset=16)
    for k, v in enumerate(video.rgb_to_yuv_coefficients("bt709", False)[1:]):
        job.coef[k] = v
    for k, (at, step) in enumerate(((OUT_AT, 1), (OUT_AT + UV_AT, 2), (OUT_AT + UV_AT + 1, 2))):
        job.planes[k].dst_dev, job.planes[k].dst_pitch, job.planes[k].dst_step = base + at, 104, step
    for k, fields in (planes or {}).items():
        for f, v in fields.items():
            setattr(job.planes[k], f, base + v[0] if isinstance(v, tuple) else v)
    for f, v in over.items():
        if f.startswith("coef"):
            job.coef[int(f[4:])] = v
        else:
            setattr(job, f, base + v[0] if isinstance(v, tuple) else v)
    job._keep = mem
    return job


def test_every_invalid_pack_job_carries_its_message_and_needs_no_gpu():
    lib = _lib_video.load()
    assert lib.vghy_pack_rgb(None, None) == -1 and b"null job" in lib.vghy_last_error()
    for kw, words in ((dict(src_dev=None), b"null image"), (dict(height=0), b"image 0 x 100 outside 1 .. 32767"), (dict(width=40000), b"outside 1 .. 32767"),
                      (dict(src_pitch_bytes=299), b"src_pitch_bytes 299 < width * 3 = 300"), (dict(y_offset=256), b"y_offset 256 outside 0 .. 255"), (dict(y_offset=-1), b"y_offset -1"),
                      (dict(coef4=(1 << 20) + 1), b"coefficient 4 is 1048577"), (dict(coef8=-(1 << 20) - 1), b"coefficient 8 is -1048577"),
                      (dict(planes={1: dict(dst_dev=None)}), b"plane U: null plane"), (dict(planes={0: dict(src_pitch=104)}), b"plane Y: the src_ fields"),
                      (dict(planes={2: dict(src_dev=(64,))}), b"plane V: the src_ fields"), (dict(planes={2: dict(dst_step=4)}), b"plane V: step 4 is not 1 or 2"),
                      (dict(planes={0: dict(dst_pitch=99)}), b"plane Y: dst_pitch 99 outside 100"), (dict(planes={0: dict(dst_dev=(96 * 304 + 299,))}), b"plane Y overlaps the source image"),
                      (dict(planes={2: dict(dst_dev=(5,))}), b"plane V overlaps the source image")):
        job = _pack_job(**kw)
        rc = lib.vghy_pack_rgb(job, None)
        assert rc == -1 and words in lib.vghy_last_error(), (words, rc, lib.vghy_last_error())
        assert not job._keep.any()


def test_host_checks_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "yuv_anonymize_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "yuv_anonymize_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "yuv_anonymize host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_library_is_declared_in_the_build():
    from head_detector_amd import build

    assert build.ANON_HEADERS == build.HOST_HEADERS + ["head_rows.h"]
    assert build.PLANE_HEADERS == ["plane_views.h"]
    assert build.VIDEO == [build.Companion("libvghvideo.so", list(SOURCES), build.HOST_HEADERS + ["head_rows.h", "plane_views.h"], "vgh_video.h", [], "build_video")]
    # the two older lists are as they were
    assert [c.lib for c in build.COMPANIONS] == ["libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghtex.so", "libvghvis.so", "libvghview.so"]
    assert build.APPLICATIONS == [build.Companion("libvghanon.so", ["anonymize.hip"], build.ANON_HEADERS, "vgh_anon.h", [], "build_anon")]
    # the core does not take the new sources, or the headers they share with the RGB anonymiser and with the overlay, for its own
    core = {f for f in os.listdir(build.CSRC)} - {f for c in build.COMPANIONS + build.APPLICATIONS + build.VIDEO for f in c.sources + c.headers}
    assert not core & (set(SOURCES) | {"head_rows.h", "plane_views.h"}) and set(build.SOURCES) <= core
    # the head rows are csrc/head_rows.h's, shared with csrc/anonymize.hip: included, and defined here no longer
    anon = open(os.path.join(build.CSRC, SOURCES[0])).read()
    assert '#include "head_rows.h"' in anon
    for moved in ("struct HeadRow", "head_of(const uint32_t", "in_ellipse(const HeadRow", "void paint_owner_kernel(const HeadRow", "int64_t up16("):
        assert moved not in anon, moved
    # a frame's planes addressed in place are csrc/plane_views.h's, shared with csrc/osd.hip: included by both sources, and defined here no longer
    shared = open(os.path.join(build.CSRC, "plane_views.h")).read()
    for name in SOURCES:
        src = open(os.path.join(build.CSRC, name)).read()
        assert '#include "plane_views.h"' in src
        for moved in ("struct Chan", "int pair_of(", "void plane_range(", "void copy_kernel(", "reinterpret_cast<const uint16_t*>", "null plane (src_dev", "the destination overlaps source plane"):
            assert moved in shared and moved not in src, (name, moved)
    assert "hip/" not in shared and "include/" not in shared and "vgho_" not in shared.lower() and "vghy_" not in shared.lower()
    for name in SOURCES + ("head_rows.h", "plane_views.h"):
        src = open(os.path.join(ROOT, "head_detector_amd", "csrc", name)).read()
        assert name == "plane_views.h" or ('#include "companion_host.h"' in src and ('#include "../../include/vgh_video.h"' in src or name == "head_rows.h"))
        # no floating point, no inline assembly, static LDS only, all host plumbing from companion_host.h, nothing of the other libraries
        for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "hipMalloc(", "set_error(const char", "g_error", "asm", "dlopen", "float", "double",
                        "hipFuncSetAttribute", "extern __shared__", "vgh_anon.h", "vgh.h", "vghan_"):
            assert by_hand not in src, (name, by_hand)
    assert "static_assert(VGHY_OK == OK && VGHY_ERR_INVALID == ERR_INVALID && VGHY_ERR_HIP == ERR_HIP && VGHY_ERR_NOMEM == ERR_NOMEM," in open(os.path.join(build.CSRC, SOURCES[0])).read()
    assert "head_detector_amd/build_video/" in open(os.path.join(ROOT, ".gitignore")).read().split()
    # nine libraries; nobody else exports the prefix, and this one links none of the others
    pkg = os.path.join(ROOT, "head_detector_amd")
    libs = sorted(f for f in os.listdir(pkg) if f.startswith("libvgh") and f.endswith(".so") and f not in ("libvgh_exp.so", "libvgh_var.so"))
    assert set(libs) >= {"libvgh.so", "libvghview.so", "libvghvis.so", "libvghtex.so", "libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghanon.so", "libvghvideo.so"}
    for f in libs:
        if f != "libvghvideo.so":
            assert not [s for s in _exported(os.path.join(pkg, f)) if s.startswith("vghy_")], f
    ldd = subprocess.run(["ldd", _lib_video.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvgh" not in ldd
    for other in ("_lib.py", "_lib_anon.py", "_lib_view.py", "_lib_vis.py", "_lib_tex.py", "_lib_eval.py", "_lib_merge.py", "_lib_track.py"):
        assert "libvghvideo" not in open(os.path.join(pkg, other)).read(), other  # and none of their bindings loads it


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------
def test_chroma_rows_of_hand_computed_heads():
    assert video.chroma_box((6, 17, 54, 53)) == (3, 8, 27, 27) and video.chroma_box((-12, -3, 27, 89)) == (-6, -2, 14, 45) and video.chroma_box((5, 5, 6, 6)) == (2, 2, 3, 3)
    assert video.chroma_box((50, 59, 50, 71)) == (25, 29, 25, 29) and video.chroma_box((7, 9, 21, 9)) == (3, 4, 3, 4)  # a zero side: empty, though (x1 + 1) >> 1 > x0 >> 1
    # the chroma box contains every chroma sample of every luma pixel of the luma box, and no row or column more
    for x0 in range(-5, 6):
        for x1 in range(x0, x0 + 8):
            for y0, y1 in ((-3, 4), (2, 3), (1, 1)):
                box = (x0, y0, x1, y1)
                c = video.chroma_box(box)
                assert c == yref.chroma_box(box)
                samples = {(x >> 1, y >> 1) for x in range(x0, x1) for y in range(y0, y1)}
                if not samples:
                    assert c[2] == c[0] and c[3] == c[1]
                    continue
                assert all(c[0] <= sx < c[2] and c[1] <= sy < c[3] for sx, sy in samples), box
                assert (c[0], c[2] - 1) == (min(s[0] for s in samples), max(s[0] for s in samples)) and (c[1], c[3] - 1) == (min(s[1] for s in samples), max(s[1] for s in samples)), box
    # plan_rows is what anonymize_plan does with its boxes, and what the chroma rows get: the same formulas on the chroma box
    heads = [yc.head((10, 20, 40, 30)), yc.head((-9, 5, 33, 77)), yc.head((50, 60, 0, 10)), yc.head((5, 5, 1, 1))]
    plan = anonymize.anonymize_plan((97, 131), heads, "pixelate", "ellipse", margin=0.1, cells=8)
    boxes = [tuple(r)[:4] for r in plan.heads.tolist()]
    assert boxes == [(6, 17, 54, 53), (-12, -2, 27, 89), (50, 59, 50, 71), (5, 5, 6, 6)]
    tables = anonymize.TapTables()
    rows, _ = anonymize.plan_rows(boxes, "pixelate", 8, 0.1, tables)
    assert np.array_equal(rows, plan.heads) and tables.taps().size == 0
    chroma, _ = anonymize.plan_rows([video.chroma_box(b) for b in boxes], "pixelate", 8, 0.1, tables)
    # chroma boxes 24 x 19, 20 x 46, empty, 1 x 1: cell side ceil(max side / 8), at least 1
    assert [tuple(r) for r in chroma.tolist()] == [(3, 8, 27, 27, 3, 0, 0, 0), (-6, -1, 14, 45, 6, 0, 0, 0), (25, 29, 25, 29, 1, 0, 0, 0), (2, 2, 3, 3, 1, 0, 0, 0)]
    plan = anonymize.anonymize_plan((97, 131), heads, "blur", "box", margin=0.0, strength=0.05)
    boxes = [tuple(r)[:4] for r in plan.heads.tolist()]
    tables = anonymize.TapTables()
    rows, sigmas = anonymize.plan_rows(boxes, "blur", 8, 0.05, tables)
    assert np.array_equal(rows, plan.heads) and np.array_equal(tables.taps(), plan.taps) and np.array_equal(sigmas, plan.sigmas)
    chroma, csig = anonymize.plan_rows([video.chroma_box(b) for b in boxes], "blur", 8, 0.05, tables)
    # chroma boxes 20 x 15, 17 x 39, empty, 1 x 1 (luma (5, 5, 6, 6)): sigma = 0.05 * max side = 1.0, 1.95, 0, 0.05 -> r = 3, 6, 0, 1; the tables go behind the luma's 25 taps, and
    # the 1 x 1 box shares the luma table of its 1 x 1 luma box
    assert chroma["radius"].tolist() == [3, 6, 0, 1] and chroma["tap_offset"].tolist() == [25, 29, 36, 23] and tables.taps().size == 37
    assert np.array_equal(tables.taps()[:25], plan.taps)
    for i in range(4):
        at, r = int(chroma["tap_offset"][i]), int(chroma["radius"][i])
        assert tables.taps()[at:at + r + 1].tolist() == ref.taps(float(csig[i]), r)
    # the caps hold for chroma whenever they hold for luma
    rng = np.random.default_rng(3)
    for _ in range(300):
        x0, y0 = (int(v) for v in rng.integers(-40, 40, 2))
        w, h = (int(v) for v in rng.integers(0, 2000, 2))
        c = video.chroma_box((x0, y0, x0 + w, y0 + h))
        assert max(c[2] - c[0], c[3] - c[1]) <= max(w, h)
        for cells in (1, 7, 64):
            side = ref.cell_side(c, cells)
            assert -(-(c[2] - c[0]) // side) <= cells and -(-(c[3] - c[1]) // side) <= cells
    # the restatement's own arithmetic gives the same chroma rows for every api case
    for name, case in yc.cases().items():
        if case["kind"] == "api" and case["region"] != "mesh":
            r = yc.rows_of(case)
            tables = anonymize.TapTables()
            got, _ = anonymize.plan_rows([video.chroma_box(b) for b in r["luma_boxes"]], case["method"], case["cells"], case["strength"], tables)
            assert [tuple(q)[:4] for q in got.tolist()] == [tuple(b) for b in r["chroma_boxes"]], name
            if case["method"] == "pixelate":
                assert got["cell"].tolist() == r["chroma_cell"], name
            if case["method"] == "blur":
                for i, t in enumerate(r["chroma_taps"]):
                    at = int(got["tap_offset"][i])
                    assert tables.taps()[at:at + len(t)].tolist() == t and int(got["radius"][i]) == len(t) - 1, (name, i)
            assert video.rgb_to_yuv(case["color"], case["matrix"], case["full_range"]) == r["color_yuv"], name


def test_python_errors_come_before_a_gpu_is_looked_for():
    y, u, v = (torch.from_numpy(p) for p in yuv_ref.picture(40, 50, 1))
    frame = YUV420Frame(y, u, v, chroma_step=1)
    heads = [yc.head((5, 5, 10, 10)), yc.head((1, 1, 4, 4))]
    res = PredictionResult(None, heads, source_frame=frame)
    assert "num heads=2" in repr(res)
    for call in (lambda **kw: video.anonymize_frame(frame, heads, **kw), lambda **kw: res.anonymize_frame(**kw)):
        for kw, words in ((dict(method="pose"), "method must be one of"), (dict(region="hair"), "region must be one of"), (dict(region="mesh"), "no triangle list"),
                          (dict(color=(0, 0, 256)), "color"), (dict(color=(0, 0)), "color"), (dict(margin=-0.1), "margin"), (dict(cells=0), "cells"), (dict(cells=65), "cells"),
                          (dict(method="blur", strength=float("inf")), "strength"), (dict(out="frame"), "out must be a YUV420Frame"),
                          (dict(out=YUV420Frame(*(torch.from_numpy(p) for p in yuv_ref.picture(40, 52, 1)), chroma_step=1)), "out must be a YUV420Frame of 40 x 50")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    for bad, words in ((yc.head((5, 5, -1, 10)), "head 1: bbox"), (yc.head((5, 5, 40000, 10)), "head 1: box sides"), (yc.head((1 << 25, 5, 4, 10)), "head 1: box corner")):
        with pytest.raises(ValueError, match=words):
            video.anonymize_frame(frame, [heads[0], bad])
    with pytest.raises(ValueError, match=r'head 1: a blur of strength 0.5 .* needs radius 1500 > 1024; use method="pixelate"'):
        video.anonymize_frame(frame, [heads[0], yc.head((0, 0, 1000, 10))], "blur", "box", margin=0.0, strength=0.5)
    with pytest.raises(ValueError, match="owner must be int32"):
        video.anonymize_frame(frame, heads, owner=np.zeros((40, 50), np.int64))
    with pytest.raises(ValueError, match="owner must be int32"):
        video.anonymize_frame(frame, heads, owner=np.zeros((40, 51), np.int32))
    with pytest.raises(ValueError, match="frame must be a YUV420Frame"):
        video.anonymize_frame(np.zeros((40, 50, 3), np.uint8), heads)
    with pytest.raises(ValueError, match=r"anonymize\(\)"):  # no frame: the message names the RGB route
        PredictionResult(np.zeros((40, 50, 3), np.uint8), heads).anonymize_frame()
    assert PredictionResult(np.zeros((40, 50, 3), np.uint8), heads).source_frame is None
    assert video.frame_rgb(frame, "none") is None and video.frame_rgb(frame, "host").shape == (40, 50, 3)
    with pytest.raises(ValueError, match="'none'"):
        video.frame_rgb(frame, "both")
    for bad in (dict(layout="yv12"), dict(layout="nv12", matrix="bt470")):
        with pytest.raises(ValueError):
            YUV420Frame.from_rgb(np.zeros((4, 4, 3), np.uint8), **bad)
    with pytest.raises(ValueError, match="layout must be one of"):
        YUV420Frame.empty(4, 4, "yv12", "cpu")
    e = YUV420Frame.empty(5, 7, "i420", "cpu", matrix="bt601", full_range=True)  # (no kernel runs: a CPU surface is only viewed)
    assert e.shape == (5, 7, 3) and (e.chroma_step, e.matrix, e.full_range, e.y_pitch, e.uv_pitch) == (1, "bt601", True, 8, 4)
    n = YUV420Frame.empty(5, 7, "nv21", "cpu")
    assert n.chroma_step == 2 and n.u.data_ptr() == n.v.data_ptr() + 1  # (V, U) pairs
    if not torch.cuda.is_available():  # after them, and only then: the missing GPU
        with pytest.raises(VghError, match="need a GPU"):
            video.anonymize_frame(frame, heads)
        with pytest.raises(VghError, match="need a GPU"):
            YUV420Frame.from_rgb(np.zeros((4, 4, 3), np.uint8))


# ---- the packer's coefficients --------------------------------------------------------------------------------------------------------------------
def test_packer_coefficients_are_pinned():
    assert video.rgb_to_yuv_coefficients("bt709", False) == (16, 11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639)
    assert video.rgb_to_yuv_coefficients("bt601", False) == (16, 16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681)
    for matrix in video.MATRICES:
        for full in (False, True):
            k = video.rgb_to_yuv_coefficients(matrix, full)
            assert k == yref.coefficients(matrix, full) and len(k) == 10 and all(isinstance(c, int) for c in k)
            assert k[0] == (0 if full else 16) and sum(k[1:4]) == (65536 if full else round(65536 * 219 / 255)) and sum(k[4:7]) == 0 and sum(k[7:10]) == 0 and k[6] == k[7]
            for color in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (12, 200, 99)):
                assert video.rgb_to_yuv(color, matrix, full) == yref.pixel_yuv(color, k)
    with pytest.raises(ValueError, match="not one of"):
        video.rgb_to_yuv_coefficients("bt470")
    for bad in ((0, 0, 256), (0, 0), (0.5, 1, 2)):
        with pytest.raises(ValueError, match="three integers"):
            video.rgb_to_yuv(bad)


@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
def test_packer_properties_over_all_colours(matrix):
    """All 2^24 colours, both ranges, on the restatement's rule for one pixel (vectorised as in ``yref.pack``): greys are neutral, black and white land on the
    range's ends, limited range stays inside its bounds, and ``to_rgb`` of the packed colour is within 2 (limited) or 1 (full range) of the colour."""
    r = np.arange(256, dtype=np.int32).reshape(256, 1, 1)
    g = np.arange(256, dtype=np.int32).reshape(1, 256, 1)
    b = np.arange(256, dtype=np.int32).reshape(1, 1, 256)
    grey = np.arange(256)
    for full in (False, True):
        o, *k = yref.coefficients(matrix, full)
        y = np.clip(o + ((k[0] * r + k[1] * g + k[2] * b + 32768) >> 16), 0, 255)
        u = np.clip(128 + ((k[3] * r + k[4] * g + k[5] * b + 32768) >> 16), 0, 255)
        v = np.clip(128 + ((k[6] * r + k[7] * g + k[8] * b + 32768) >> 16), 0, 255)
        assert y.shape == (256, 256, 256) and y.dtype == np.int32
        assert (u[grey, grey, grey] == 128).all() and (v[grey, grey, grey] == 128).all()
        assert (int(y[0, 0, 0]), int(y[255, 255, 255])) == ((0, 255) if full else (16, 235))
        if not full:
            assert y.min() == 16 and y.max() == 235 and u.min() >= 16 and u.max() <= 240 and v.min() >= 16 and v.max() <= 240
        # a few colours through the loop restatement: the vectorised lines above are the same rule
        for color in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (17, 130, 244)):
            assert yref.pixel_yuv(color, (o, *k)) == (int(y[color]), int(u[color]), int(v[color]))
        y_offset, cy, crv, cgu, cgv, cbu = video.yuv_coefficients(matrix, full)  # back, by the rule of include/vgh.h
        luma = cy * (y - y_offset) + 32768
        d, e = u - 128, v - 128
        worst = 0
        for back, want in ((luma + crv * e, r), (luma + cgu * d + cgv * e, g), (luma + cbu * d, b)):
            worst = max(worst, int(np.abs(np.clip(back >> 16, 0, 255) - want).max()))
        assert worst <= (1 if full else 2), (matrix, full, worst)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def test_restatement_facts():
    rng = np.random.default_rng(0)
    # the packer: the loop and the vectorised form agree, on odd sizes and on saturating content
    for h, w in ((1, 1), (2, 2), (1, 7), (5, 3), (12, 17)):
        for image in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)):
            for matrix, full in (("bt709", False), ("bt601", True), ("bt2020", False)):
                k = yref.coefficients(matrix, full)
                a, b = yref.pack_loop(image, k), yref.pack(image, k)
                assert all(np.array_equal(p, q) and p.dtype == np.uint8 for p, q in zip(a, b)) and a[1].shape == ((h + 1) // 2, (w + 1) // 2)
    const = np.empty((6, 9, 3), np.uint8)
    const[:] = (200, 30, 77)
    y, u, v = yref.pack(const, yref.coefficients("bt709", False))
    assert (y == y[0, 0]).all() and (u == u[0, 0]).all() and (v == v[0, 0]).all() and (int(y[0, 0]), int(u[0, 0]), int(v[0, 0])) == yref.pixel_yuv((200, 30, 77), yref.coefficients("bt709", False))
    # a block's chroma comes from the rounded mean of its in-image pixels: (0, 0, 0) and (255, 255, 255) side by side in a 1 x 2 image -> the grey 128
    pair = np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8)
    k = yref.coefficients("bt601", True)
    assert yref.pack(pair, k)[1][0, 0] == 128 and yref.pack(pair, k)[0].tolist() == [[0, 255]]
    # the chroma owner: the maximum of four, out-of-range values count as -1, the in-image pixels only
    owner = np.array([[-1, 0, 2, 7, 1], [-1, -1, 1, -5, 0], [3, -1, -1, -1, -1]], np.int32)
    assert yref.chroma_owner(owner, 3).tolist() == [[0, 2, 1], [-1, -1, -1]]
    assert yref.chroma_owner(owner, 4).tolist() == [[0, 2, 1], [3, -1, -1]] and yref.chroma_owner(owner, 8).tolist() == [[0, 7, 1], [3, -1, -1]]
    # a frame: every plane is the pinned restatement of a one-channel image; nobody's samples are untouched; a chroma sample goes as soon as one luma pixel is owned
    y, u, v = yuv_ref.picture(23, 31, 4)
    boxes = [(-5, 3, 20, 19), (10, -4, 40, 30)]
    owner = ref.owner_map(23, 31, boxes, "ellipse")
    oc = yref.chroma_owner(owner, 2)
    for method, kw in (("fill", dict(color_yuv=(1, 2, 3))), ("pixelate", dict(luma_cell=[4, 5], chroma_cell=[2, 3])), ("blur", dict(luma_taps=[ref.taps(1.5, 5)] * 2, chroma_taps=[ref.taps(0.8, 3)] * 2))):
        Y, U, V = yref.render_frame(y, u, v, boxes, owner, method, **kw)
        assert np.array_equal(Y[owner < 0], y[owner < 0]) and np.array_equal(U[oc < 0], u[oc < 0]) and np.array_equal(V[oc < 0], v[oc < 0]) and not np.array_equal(Y, y), method
        stacked = ref.render(np.stack([y, y, y], -1), boxes, owner, method, cell=kw.get("luma_cell"), tap_tables=kw.get("luma_taps"), color=(1, 1, 1))
        assert np.array_equal(Y, stacked[..., 0]), method
    Y, U, V = yref.render_frame(y, u, v, boxes, owner, "fill", color_yuv=(1, 2, 3))
    assert (Y[owner >= 0] == 1).all() and (U[oc >= 0] == 2).all() and (V[oc >= 0] == 3).all()
    lone = np.full((23, 31), -1, np.int32)
    lone[7, 9] = 0  # one owned luma pixel, the odd corner of its 2 x 2 block
    Y, U, V = yref.render_frame(y, u, v, boxes[:1], lone, "fill", color_yuv=(1, 2, 3))
    assert (Y != y).sum() <= 1 and U[3, 4] == 2 and V[3, 4] == 3 and (yref.chroma_owner(lone, 1) >= 0).sum() == 1
    # a sample outside its owner's box OF THAT PLANE stays: chroma boxes of the caller's own
    Y, U, V = yref.render_frame(y, u, v, boxes, owner, "fill", chroma_boxes=[(0, 0, 0, 0), (6, 0, 9, 4)], color_yuv=(1, 2, 3))
    inside = np.zeros_like(oc, dtype=bool)
    inside[0:4, 6:9] = True
    assert np.array_equal(U[~inside], u[~inside]) and (U[inside & (oc == 1)] == 2).all() and np.array_equal(U[inside & (oc != 1)], u[inside & (oc != 1)])


def test_every_planted_case_contains_what_it_claims():
    cases = yc.cases()
    assert len(cases) >= 40 and {c["method"] for c in cases.values()} == {"fill", "pixelate", "blur"} and {c["region"] for c in cases.values()} == {"box", "ellipse", "mesh", "map"}
    assert {c["shape"] for c in cases.values()} >= {(97, 131), (96, 130), (1, 1), (2, 2), (1, 7), (64, 64)}
    for layout in yc.LAYOUTS:
        assert {c["pitched"] for c in cases.values() if c["layout"] == layout} == {True, False}, layout  # every layout pitched and dense
        assert {c["method"] for c in cases.values() if c["layout"] == layout} == {"fill", "pixelate", "blur"}, layout
    assert {c["full_range"] for c in cases.values() if c["kind"] == "api"} == {True, False} and any(c["content"] == "saturating" for c in cases.values())
    identities = {"no_heads", "pixelate_identity", "blur_r0", "tiny_1x1_pixelate", "tiny_1x1_blur"}
    for name, case in cases.items():
        want = yc.expected(name, case)
        planes = yc.planes_of(case)
        h, w = case["shape"]
        assert [p.shape for p in want] == [(h, w), ((h + 1) // 2, (w + 1) // 2)] * 1 + [((h + 1) // 2, (w + 1) // 2)] and all(p.dtype == np.uint8 for p in want), name
        changed = [not np.array_equal(a, b) for a, b in zip(want, planes)]
        if name in identities:
            assert not any(changed), name
        elif (h, w) == (97, 131) or (h, w) == (96, 130) or (h, w) == (64, 64):
            assert all(changed), name
        else:
            assert any(changed), name
        # the surface: sentinel bytes between width and pitch (pitched), and the same sentinels around the expected planes
        buf, pitch, off = yc.surface_of(case)
        wbuf = yc.surface_of(case, want)[0]
        cw = (w + 1) // 2
        assert pitch == (2 * cw + 10 if case["pitched"] else 2 * cw) and off == pitch * (h + (3 if case["pitched"] else 0))
        mask = np.ones(buf.size, bool)  # the bytes of no sample
        frame = yc.frame_of(case, torch.from_numpy(buf))
        index = torch.arange(buf.size, dtype=torch.int64)
        for p in yc.frame_of(case, index.to(torch.uint8)).planes:
            mask[torch.as_strided(index, p.shape, p.stride(), p.storage_offset()).reshape(-1).numpy()] = False
        assert mask.sum() >= 8 and np.array_equal(buf[mask], wbuf[mask]) and (not case["pitched"] or mask.sum() > 10 * h)
        assert all(np.array_equal(p.numpy(), q) for p, q in zip(frame.planes, planes)), name
    H, W = 97, 131
    boxes = [ref.geometry_box(b, 0.1) for b in yc.EDGE_BOXES]
    assert boxes[0][0] < 0 < boxes[0][2] and boxes[1][0] < W < boxes[1][2] and boxes[2][1] < 0 < boxes[2][3] and boxes[3][1] < H < boxes[3][3]
    assert {b[0] % 2 for b in boxes} == {0, 1} and {b[2] % 2 for b in boxes} == {0, 1}  # odd and even corners
    odd = [ref.geometry_box(b, 0.1) for b in yc.ODD_BOXES]
    assert odd[0][0] >= W and odd[1][2] <= 0 and odd[2][0] == odd[2][2] and odd[3][1] == odd[3][3] and odd[4] == (70, 60, 71, 61) and odd[5][0] < 0 and odd[5][2] > W
    r = yc.rows_of(cases["odd_pixelate_box"])
    assert r["chroma_boxes"][2][0] == r["chroma_boxes"][2][2] and r["chroma_boxes"][3][1] == r["chroma_boxes"][3][3] and r["chroma_boxes"][4] == (35, 30, 36, 31)
    assert yc.rows_of(cases["pixelate_identity"])["luma_cell"] == [1] and yc.rows_of(cases["pixelate_identity"])["chroma_cell"] == [1]  # a cell side of 1 in both planes
    radii = {name: (len(yc.rows_of(cases[name])["luma_taps"][0]) - 1, len(yc.rows_of(cases[name])["chroma_taps"][0]) - 1) for name in ("blur_r0", "blur_r70", "blur_all_clamp")}
    assert radii == {"blur_r0": (0, 0), "blur_r70": (70, 36), "blur_all_clamp": (150, 75)} and 150 > max(H, W) and 75 > max((H + 1) // 2, (W + 1) // 2)
    assert len(cases["many_heads_blur"]["heads"]) == 300 and cases["many_heads_blur"]["shape"] == (64, 64) and len(cases["no_heads"]["heads"]) == 0
    own = cases["owner_fill"]["owner"]
    assert (own == -1).any() and (own == 7).any() and (own == -5).any() and own[0, 120] == 1
    raw = cases["raw_free_chroma_fill"]
    assert raw["chroma_boxes"] != [yref.chroma_box(b) for b in raw["luma_boxes"]]  # rows the plan never makes
    oc = yref.chroma_owner(yc.owner_of(raw, raw["luma_boxes"]), 2)
    U = yc.expected("raw_free_chroma_fill", raw)[1]
    u = yc.planes_of(raw)[1]
    assert (oc[21:25, 5:24] == 0).all() and np.array_equal(U[21:25, 5:24], u[21:25, 5:24]) and (oc[8:20, 8:20] == 0).all() and (U[8:20, 8:20] == 250).all()  # owned, outside the chroma box: unchanged
