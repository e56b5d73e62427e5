"""Host half of head anonymisation (head_detector_amd/anonymize.py, include/vgh_anon.h): the ABI of libvghanon.so, every refusal of the C call, the plan against
hand-computed rows, the taps, facts of the restatement (tests/anonymize_ref.py), every planted case against what it claims to contain, and the host code of
csrc/anonymize.hip under the host sanitizers (tests/anonymize_host.hip: a program of its own, never run through Python, never on a GPU).  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_cases as ac  # noqa: E402
import anonymize_ref as ref  # noqa: E402

from head_detector_amd import _lib_anon, anonymize  # noqa: E402
from head_detector_amd._lib import VghError  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib_anon.C
WANT = {"vghan_version", "vghan_last_error", "vghan_workspace_bytes", "vghan_anonymize"}


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


# ---- the library ----------------------------------------------------------------------------------------------------------------------------------
def test_anon_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_anon.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghan_[a-z0-9_]+)\s*\(", code))
    assert declared == WANT == set(_lib_anon.SYMBOLS)
    assert _exported(_lib_anon.LIB_PATH) == WANT  # hidden visibility: nothing of companion_host.h, no kernel stub
    lib = _lib_anon.load()
    assert lib.vghan_version().startswith(b"vghanon")
    for name, value in (("VGHAN_MAX_SIDE", _lib_anon.MAX_SIDE), ("VGHAN_MAX_COORD", _lib_anon.MAX_COORD), ("VGHAN_MAX_HEADS", _lib_anon.MAX_HEADS), ("VGHAN_MAX_CELLS", _lib_anon.MAX_CELLS),
                        ("VGHAN_MAX_RADIUS", _lib_anon.MAX_RADIUS), ("VGHAN_TAP_SUM", _lib_anon.TAP_SUM), ("VGHAN_METHOD_FILL", _lib_anon.METHODS["fill"]),
                        ("VGHAN_METHOD_PIXELATE", _lib_anon.METHODS["pixelate"]), ("VGHAN_METHOD_BLUR", _lib_anon.METHODS["blur"]), ("VGHAN_REGION_BOX", _lib_anon.REGION_BOX),
                        ("VGHAN_REGION_ELLIPSE", _lib_anon.REGION_ELLIPSE), ("VGHAN_REGION_MAP", _lib_anon.REGION_MAP)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    assert (_lib_anon.MAX_SIDE, _lib_anon.MAX_HEADS, _lib_anon.MAX_CELLS, _lib_anon.MAX_RADIUS, _lib_anon.TAP_SUM) == (32767, 65536, 64, 1024, 65536)
    assert (ref.TAP_SUM, ref.MAX_RADIUS) == (_lib_anon.TAP_SUM, _lib_anon.MAX_RADIUS)
    # the job, field for field
    fields = re.search(r"typedef struct vghan_job \{(.*?)\} vghan_job;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _lib_anon.Job._fields_]
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [C.c_void_p if star else kinds[t] for t, star in re.findall(r"^\s*(?:const )?(\w+)(\*?) \w+;", fields, flags=re.M)] == [k for _, k in _lib_anon.Job._fields_]
    assert C.sizeof(_lib_anon.Job) == 80
    # the head row: eight int32 in the header's order
    row = re.search(r"typedef struct vghan_head \{(.*?)\} vghan_head;", code, flags=re.S).group(1)
    assert re.findall(r"int32_t ([^;]+);", row) == ["x0, y0, x1, y1", "cell", "radius", "tap_offset", "reserved"]
    assert _lib_anon.HEAD_DTYPE.names == ("x0", "y0", "x1", "y1", "cell", "radius", "tap_offset", "reserved") and _lib_anon.HEAD_DTYPE.itemsize == 32


def _job(rows=None, table=None, **over):
    """A valid blur job on host memory that is never touched: the argument checks come first."""
    mem = np.zeros(1 << 16, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16
    rows = np.array([(10, 10, 60, 50, 7, 1, 0, 0), (-20, -5, 30, 40, 8, 0, 2, 0), (90, 80, 90, 95, 1, 1, 0, 0)] if rows is None else rows, dtype=_lib_anon.HEAD_DTYPE)
    table = np.array([65534, 1, 65536, 0] if table is None else table, dtype=np.int32)
    fields = dict(src_dev=base, dst_dev=base + 32768, src_pitch_bytes=300, height=97, width=100, n_heads=len(rows), method=2, region=1, color=0, heads=rows.ctypes.data,
                  taps=table.ctypes.data, n_taps=len(table), reserved=0, owner_dev=None)
    fields.update({k: base + v[0] if isinstance(v, tuple) else v for k, v in over.items()})  # a tuple is an offset from the block's base
    job = _lib_anon.Job(**fields)
    job._keep = (mem, rows, table)
    return job, base


def test_workspace_bytes_of_hand_computed_jobs():
    lib = _lib_anon.load()
    up = lambda v: (v + 15) & ~15  # noqa: E731
    owner = 4 * 97 * 100
    job, base = _job()
    assert lib.vghan_workspace_bytes(job) == up(up(owner + 4 * (50 * 40 + 30 * 40)) + 2 * 3 * (42 * 50 + 40 * 30))  # r = 1: 40 + 2 rows of h; r = 0: 40
    assert lib.vghan_workspace_bytes(_job(method=0)[0]) == up(owner)
    assert lib.vghan_workspace_bytes(_job(method=1)[0]) == up(owner + 4 * (8 * 6 + 7 * 6))
    job, base = _job(method=1, region=2)
    job.owner_dev = base + 64
    assert lib.vghan_workspace_bytes(job) == up(4 * (8 * 6 + 7 * 6))
    job, base = _job(rows=np.zeros(0, _lib_anon.HEAD_DTYPE))
    assert lib.vghan_workspace_bytes(job) == up(owner)  # no heads: the owner plane alone
    for shape in ((1, 1), (97, 131), (3000, 4000)):
        job, _ = _job(height=shape[0], width=shape[1], src_pitch_bytes=3 * shape[1] + 5, dst_dev=base + (1 << 40))
        assert lib.vghan_workspace_bytes(job) % 16 == 0 and lib.vghan_workspace_bytes(job) >= 16
    assert lib.vghan_workspace_bytes(None) == 0 and b"null job" in lib.vghan_last_error()


def test_every_invalid_job_carries_its_message_and_needs_no_gpu():
    lib = _lib_anon.load()

    def refused(words, ws=16, rows=None, table=None, **over):
        job, base = _job(rows, table, **over)
        rc =lib.vghan_anonymize(job, None if ws is None else base + ws, None)
        msg = lib.vghan_last_error()
        assert rc == -1 and words in msg, (words, rc, msg)
        if ws == 16:
            assert lib.vghan_workspace_bytes(job) == 0, words
        assert not job._keep[0].any()

    assert lib.vghan_anonymize(None, None, None) == -1 and b"null job" in lib.vghan_last_error()
    refused(b"null workspace", ws=None)
    refused(b"workspace is not 16-byte aligned", ws=24)
    for over, words in ((dict(src_dev=None), b"null image"), (dict(dst_dev=None), b"null image"), (dict(dst_dev=(32770,)), b"not 4-byte aligned"), (dict(height=0), b"image 0 x 100"),
                        (dict(width=32768), b"outside 1 .. 32767"), (dict(src_pitch_bytes=299), b"src_pitch_bytes 299 < width * 3 = 300"), (dict(n_heads=-1), b"n_heads -1"),
                        (dict(n_heads=65537), b"n_heads 65537 outside 0 .. 65536"), (dict(method=3), b"unknown method 3"), (dict(method=-1), b"unknown method -1"),
                        (dict(region=3), b"unknown region 3"), (dict(color=1 << 24), b"color"), (dict(reserved=2), b"reserved is 2"), (dict(region=2), b"owner_dev is null"),
                        (dict(owner_dev=(64,)), b"owner_dev is set"), (dict(region=2, owner_dev=(68,)), b"not 16-byte aligned"), (dict(heads=None), b"null heads"),
                        (dict(taps=None), b"blur needs a tap table"), (dict(n_taps=0), b"blur needs a tap table"), (dict(n_taps=-1), b"n_taps -1"),
                        (dict(n_taps=2), b"head 1: taps 2 .. 2 outside the table of 2"), (dict(dst_dev=(96 * 300,)), b"source and destination overlap"),
                        (dict(src_dev=(32768 + 97 * 300 - 4,)), b"source and destination overlap")):
        refused(words, **over)
    ok = (0, 0, 50, 50, 1, 0, 2, 0)
    for rows, method, words in (([ok, (1 << 24, 0, (1 << 24) + 5, 5, 1, 0, 2, 0)], 2, b"head 1: corner"), ([(0, 0, 32768, 5, 1, 0, 2, 0)], 2, b"head 0: box sides 32768 x 5"),
                                ([ok, ok, (5, 5, 4, 9, 1, 0, 2, 0)], 0, b"head 2: box sides -1 x 4"), ([ok, (0, 0, 5, 5, 1, 0, 2, 3)], 0, b"head 1: reserved"),
                                ([ok, (0, 0, 50, 50, 0, 0, 2, 0)], 1, b"head 1: cell side 0"), ([ok, ok, (0, 0, 130, 50, 2, 0, 2, 0)], 1, b"head 2: 65 x 25 cells of side 2 exceed 64"),
                                ([(0, 0, 50, 50, 1, 1025, 0, 0)], 2, b"head 0: radius 1025 outside 0 .. 1024"), ([ok, (0, 0, 50, 50, 1, -1, 0, 0)], 2, b"head 1: radius -1"),
                                ([ok, (0, 0, 50, 50, 1, 1, 3, 0)], 2, b"head 1: taps 3 .. 4 outside the table of 4"), ([ok, ok, (0, 0, 50, 50, 1, 0, -1, 0)], 2, b"head 2: taps -1"),
                                ([ok, (0, 0, 50, 50, 1, 1, 1, 0)], 2, b"head 1: tap sum 131073 is not 65536"), ([ok, ok, (0, 0, 50, 50, 1, 0, 3, 0)], 2, b"head 2: tap sum 0 is not 65536")):
        refused(words, rows=rows, method=method)
    refused(b"head 1: tap 1 is -1", rows=[ok, (0, 0, 50, 50, 1, 1, 2, 0)], table=[65534, 1, 65536, -1])
    # the most boxes one launch takes: 65536 heads of the largest box on the largest image
    big = np.zeros(65536, _lib_anon.HEAD_DTYPE)
    big["x1"], big["y1"], big["tap_offset"] = 32767, 32767, 2
    refused(b"exceed one launch", rows=big, height=32767, width=32767, src_pitch_bytes=3 * 32767, dst_dev=(1 << 40,))


def test_host_checks_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "anonymize_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "anonymize_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "anonymize host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_library_is_declared_in_the_build():
    from head_detector_amd import build

    assert len(build.COMPANIONS) == 6 and not [c for c in build.COMPANIONS if c.lib == "libvghanon.so"]
    assert build.ANON_HEADERS == build.HOST_HEADERS + ["head_rows.h"]
    assert build.APPLICATIONS == [build.Companion("libvghanon.so", ["anonymize.hip"], build.ANON_HEADERS, "vgh_anon.h", [], "build_anon")]
    src = open(os.path.join(ROOT, "head_detector_amd", "csrc", "anonymize.hip")).read()
    assert '#include "companion_host.h"' in src and "static_assert(VGHAN_OK == OK && VGHAN_ERR_INVALID == ERR_INVALID && VGHAN_ERR_HIP == ERR_HIP && VGHAN_ERR_NOMEM == ERR_NOMEM," in src
    # the head rows are csrc/head_rows.h's, shared with csrc/yuv_anonymize.hip: included, and defined here no longer
    assert '#include "head_rows.h"' in src
    for moved in ("struct HeadRow", "head_of(const uint32_t", "in_ellipse(const HeadRow", "void paint_owner_kernel(const HeadRow", "int64_t up16("):
        assert moved not in src, moved
    shared = open(os.path.join(ROOT, "head_detector_amd", "csrc", "head_rows.h")).read()
    assert all(moved in shared for moved in ("struct HeadRow", "head_of(const uint32_t", "in_ellipse(const HeadRow", "void paint_owner_kernel(const HeadRow", "int64_t up16("))
    assert '#include "companion_host.h"' in shared and "include/" not in shared and "vghan_" not in shared.lower() and "vghy_" not in shared.lower()  # no public header
    for text in (src, shared):
        for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "hipMalloc(", "set_error(const char", "g_error", "asm", "dlopen", "float", "double",
                        "hipFuncSetAttribute", "extern __shared__"):
            assert by_hand not in text, by_hand
    assert "head_detector_amd/build_anon/" in open(os.path.join(ROOT, ".gitignore")).read().split()
    # nobody else exports the prefix, and the other libraries keep their exports
    pkg = os.path.join(ROOT, "head_detector_amd")
    libs = sorted(f for f in os.listdir(pkg) if f.startswith("libvgh") and f.endswith(".so") and f not in ("libvgh_exp.so", "libvgh_var.so"))
    assert set(libs) >= {"libvgh.so", "libvghview.so", "libvghvis.so", "libvghtex.so", "libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghanon.so"}
    for f in libs:
        if f != "libvghanon.so":
            assert not [s for s in _exported(os.path.join(pkg, f)) if s.startswith("vghan_")], f
    assert len({s for s in _exported(os.path.join(pkg, "libvgh.so")) if s.startswith("vgh")}) == 86 and len(_exported(os.path.join(pkg, "libvghview.so"))) == 6
    ldd = subprocess.run(["ldd", _lib_anon.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvgh" not in ldd  # it links none of the others


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------
def test_plan_matches_hand_computed_rows():
    heads = [ac.head((10, 20, 40, 30)), ac.head((-9, 5, 33, 77)), ac.head((50, 60, 0, 10)), ac.head((5, 5, 1, 1))]
    p = anonymize.anonymize_plan((97, 131), heads, "pixelate", "ellipse", margin=0.1, cells=8)
    # margins int(w * 0.1), int(h * 0.1): (4, 3), (3, 7), (0, 1), (0, 0); cell side ceil(max side / 8), at least 1
    assert [tuple(r) for r in p.heads.tolist()] == [(6, 17, 54, 53, 6, 0, 0, 0), (-12, -2, 27, 89, 12, 0, 0, 0), (50, 59, 50, 71, 2, 0, 0, 0), (5, 5, 6, 6, 1, 0, 0, 0)]
    assert p.method == 1 and p.taps.size == 0 and p.heads.dtype == _lib_anon.HEAD_DTYPE
    p = anonymize.anonymize_plan((97, 131), heads, "blur", "box", margin=0.0, strength=0.05)
    # sigma = 0.05 * max side = 2.0, 3.85, 0.5, 0.05 -> r = 6, 12, 2, 1; tables end to end
    assert p.heads["radius"].tolist() == [6, 12, 2, 1] and p.heads["tap_offset"].tolist() == [0, 7, 20, 23] and p.taps.size == 25 and p.method == 2
    assert np.array_equal(p.sigmas, [0.05 * 40, 0.05 * 77, 0.05 * 10, 0.05 * 1])
    for i in range(4):
        at, r = int(p.heads["tap_offset"][i]), int(p.heads["radius"][i])
        assert p.taps[at:at + r + 1].tolist() == ref.taps(float(p.sigmas[i]), r)
    same = anonymize.anonymize_plan((97, 131), [heads[0], heads[0], heads[3], heads[0]], "blur", "box", margin=0.0, strength=0.05)
    assert same.heads["tap_offset"].tolist() == [0, 0, 7, 0] and same.taps.size == 9  # heads of one strength and size share a table
    p = anonymize.anonymize_plan((97, 131), heads[:2], "fill", "mesh", bounds=[[3, 4, 20, 30], [0, 0, -1, -1]])
    assert [tuple(r) for r in p.heads.tolist()] == [(3, 4, 21, 31, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0)] and p.method == 0  # inclusive -> half-open; empty stays empty
    p = anonymize.anonymize_plan((97, 131), [ac.head((0, 0, 27307, 10))], "blur", "box", margin=0.1, strength=0.0104)
    assert int(p.heads["x1"][0] - p.heads["x0"][0]) == 32767 and int(p.heads["radius"][0]) == 1023
    # the restatement's own arithmetic gives the same rows for every api case
    for name, case in ac.cases().items():
        if case["kind"] == "api" and case["region"] != "mesh":
            plan = anonymize.anonymize_plan((case["buffer"].shape[0], case["width"]), case["heads"], case["method"], case["region"], case["margin"], case["cells"], case["strength"])
            boxes, cell, tables = ac.rows_of(case)
            assert [tuple(r)[:4] for r in plan.heads.tolist()] == [tuple(b) for b in boxes], name
            if case["method"] == "pixelate":
                assert plan.heads["cell"].tolist() == cell, name
            if case["method"] == "blur":
                for i, t in enumerate(tables):
                    at = int(plan.heads["tap_offset"][i])
                    assert plan.taps[at:at + len(t)].tolist() == t and int(plan.heads["radius"][i]) == len(t) - 1, (name, i)


def test_python_errors_come_before_a_gpu_is_looked_for():
    image = np.zeros((40, 50, 3), np.uint8)
    heads = [ac.head((5, 5, 10, 10)), ac.head((1, 1, 4, 4))]
    res = PredictionResult(image, heads)
    for call in (lambda **kw: anonymize.anonymize_heads(image, heads, **kw), lambda **kw: res.anonymize(**kw)):
        for kw, words in ((dict(method="pose"), "method must be one of"), (dict(region="hair"), "region must be one of"), (dict(region="mesh"), "no triangle list"),
                          (dict(color=(0, 0, 256)), "color"), (dict(color=(0, 0)), "color"), (dict(margin=-0.1), "margin"), (dict(margin=float("nan")), "margin"),
                          (dict(cells=0), "cells"), (dict(cells=65), "cells"), (dict(cells=2.5), "cells"), (dict(method="blur", strength=float("inf")), "strength"),
                          (dict(method="blur", strength=-1.0), "strength")):
            with pytest.raises(ValueError, match=words):
                call(**kw)
    for bad, words in ((ac.head((5, 5, -1, 10)), "head 1: bbox"), (ac.head((5, 5, 40000, 10)), "head 1: box sides"), (ac.head((1 << 25, 5, 4, 10)), "head 1: box corner")):
        with pytest.raises(ValueError, match=words):
            anonymize.anonymize_heads(image, [heads[0], bad])
    with pytest.raises(ValueError, match=r'head 1: a blur of strength 0.5 .* needs radius 1500 > 1024; use method="pixelate"'):
        anonymize.anonymize_heads(image, [heads[0], ac.head((0, 0, 1000, 10))], "blur", "box", margin=0.0, strength=0.5)
    with pytest.raises(ValueError, match="65537 heads exceed"):
        anonymize.anonymize_plan((40, 50), [heads[0]] * 65537, "fill", "box")
    with pytest.raises(ValueError, match=r"uint8 image \[H,W,3\]"):
        anonymize.anonymize_heads(np.zeros((40, 50), np.uint8), heads)
    with pytest.raises(ValueError, match="1 .. 32767 pixels a side"):
        anonymize.anonymize_plan((40000, 50), heads, "fill", "box")
    with pytest.raises(ValueError, match="owner must be int32"):
        anonymize.anonymize_heads(image, heads, owner=np.zeros((40, 50), np.int64))
    with pytest.raises(ValueError, match="owner must be int32"):
        anonymize.anonymize_heads(image, heads, owner=np.zeros((40, 51), np.int32))
    if not torch.cuda.is_available():  # after them, and only then: the missing GPU
        with pytest.raises(VghError, match="need a GPU"):
            anonymize.anonymize_heads(image, heads)
        with pytest.raises(VghError, match="need a GPU"):
            res.anonymize("fill", "mesh", faces=np.array([[0, 1, 2]]))


def test_gaussian_taps():
    """The sum is exactly 65536, no tap is negative, and the taps do not increase away from the centre.  The side taps are a monotone rounding of a decreasing
    sequence, so they never increase, for any sigma.  The centre takes the remainder, so it carries the side taps' rounding errors: at most 0.5 each, twice each,
    r in all around the unrounded centre c = 65536 g_0 / G.  It is therefore GUARANTEED not to lie below tap 1 only where the unrounded gap
    65536 (g_0 - g_1) / G is at least r + 0.5, which holds for small sigma alone (the gap falls like 13070 / sigma^3: sigma = 33 gives the centre 790 under
    tap 1 = 794).  The whole table is held to "non-increasing" where that condition holds, and the centre to its bound |centre - c| <= r everywhere."""
    assert anonymize.gaussian_taps(0.0, 0).tolist() == [65536] and anonymize.gaussian_taps(5.0, 0).tolist() == [65536]
    sweep = [0.05, 0.2, 1 / 3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.3, 4.8, 7.25, 10.0, 16.0, 23.25, 33.0, 50.0, 77.7, 100.0, 150.0, 200.0, 250.5, 300.0, 341.0, 1024 / 3]
    whole = 0
    for sigma in sweep:
        r = int(np.ceil(3.0 * sigma))
        t = anonymize.gaussian_taps(sigma, r)
        assert t.dtype == np.int32 and t.shape == (r + 1,) and int(t[0]) + 2 * int(t[1:].sum()) == 65536, sigma
        assert (t >= 0).all() and (np.diff(t[1:]) <= 0).all(), sigma
        g = np.exp(-np.arange(r + 1, dtype=np.float64) ** 2 / (2 * sigma * sigma))
        G = g[0] + 2 * g[1:].sum()
        assert abs(int(t[0]) - 65536 * g[0] / G) <= r, sigma
        if 65536 * (g[0] - g[1]) / G >= r + 0.5:
            whole += 1
            assert (np.diff(t) <= 0).all(), sigma
        assert t.tolist() == ref.taps(sigma, r), sigma
    assert whole >= 8
    for bad in ((1.0, -1), (1.0, 1025), (0.0, 3), (float("nan"), 2)):
        with pytest.raises(ValueError):
            anonymize.gaussian_taps(*bad)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def test_restatement_facts():
    rng = np.random.default_rng(0)
    const = np.empty((23, 31, 3), np.uint8)
    const[:] = (255, 0, 77)
    boxes = [(-5, 3, 20, 19), (10, -4, 40, 30)]
    owner = ref.owner_map(23, 31, boxes, "ellipse")
    assert (owner == 0).any() and (owner == 1).any() and (owner == -1).any()
    for t in ([65536], [65534, 1], ref.taps(2.0, 6), ref.taps(40.0, 120)):  # constant in, constant out: blur (also where every tap clamps) and pixelate
        assert np.array_equal(ref.blur_image(const, t), const)
        assert np.array_equal(ref.render(const, boxes, owner, "blur", tap_tables=[t, t]), const)
    for side in (1, 3, 7, 64):
        assert np.array_equal(ref.render(const, boxes, owner, "pixelate", cell=[side, side]), const)
    image = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    assert np.array_equal(ref.blur_image(image, [65536]), image)  # r = 0 is the identity
    assert np.array_equal(ref.render(image, boxes, owner, "pixelate", cell=[1, 1]), image)  # and so is cell side 1
    for method, kw in (("fill", dict(color=(1, 2, 3))), ("pixelate", dict(cell=[4, 5])), ("blur", dict(tap_tables=[ref.taps(1.5, 5)] * 2))):
        out = ref.render(image, boxes, owner, method, **kw)
        assert np.array_equal(out[owner < 0], image[owner < 0]) and not np.array_equal(out, image), method  # owner -1: untouched
        loose = owner.copy()
        loose[0:3, 0:3] = 1  # outside head 1's box: unchanged whatever the map says
        loose[20:23, 25:31] = 9  # out of range
        other = ref.render(image, boxes, loose, method, **kw)
        assert np.array_equal(other[0:3, 0:3], image[0:3, 0:3]) and np.array_equal(other[20:23, 25:31], image[20:23, 25:31]), method
    fill = ref.render(image, boxes, owner, "fill", color=(9, 8, 7))
    assert (fill[owner >= 0] == (9, 8, 7)).all()
    # a pixelated cell is the rounded mean of ALL its in-image pixels, owned or not: the box (2, 2, 10, 10), side 4, ellipse
    one = ref.owner_map(23, 31, [(2, 2, 10, 10)], "ellipse")
    out = ref.render(image, [(2, 2, 10, 10)], one, "pixelate", cell=[4])
    assert one[2, 2] == -1 and one[5, 5] == 0
    for c in range(3):
        S = int(image[2:6, 2:6, c].astype(np.int64).sum())
        assert out[5, 5, c] == (2 * S + 16) // 32 and out[2, 2, c] == image[2, 2, c]
    # the ellipse: symmetric under both flips of its box, a 1 x 1 box is that pixel, it touches all four sides of an odd box and never leaves the box
    for box in ((0, 0, 9, 5), (3, 2, 11, 12), (-4, -3, 13, 6), (5, 5, 6, 6), (2, 3, 4, 9), (0, 0, 1, 7)):
        x0, y0, x1, y1 = box
        inside = np.array([[ref.in_ellipse(box, px, py) for px in range(x0 - 1, x1 + 1)] for py in range(y0 - 1, y1 + 1)])
        assert np.array_equal(inside, inside[::-1]) and np.array_equal(inside, inside[:, ::-1]), box
        assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any() and inside[1:-1, 1:-1].any(), box
    assert ref.in_ellipse((5, 5, 6, 6), 5, 5) and ref.owner_map(9, 9, [(5, 5, 6, 6)], "ellipse")[5, 5] == 0 and (ref.owner_map(9, 9, [(5, 5, 6, 6)], "ellipse") >= 0).sum() == 1
    big = (0, 0, 32767, 32767)  # the largest sides: exact in Python integers, and below 2^61 as the header says
    assert ref.in_ellipse(big, 16383, 0) and not ref.in_ellipse(big, 0, 0) and 2 * (32767 ** 2) * (32767 ** 2) < 2 ** 61
    # a later head owns the overlap
    assert ref.owner_map(20, 20, [(0, 0, 10, 10), (5, 5, 15, 15)], "box")[7, 7] == 1 and ref.owner_map(20, 20, [(0, 0, 10, 10), (5, 5, 15, 15)], "box")[4, 7] == 0


def test_every_planted_case_contains_what_it_claims():
    cases = ac.cases()
    assert len(cases) >= 35 and {c["method"] for c in cases.values()} == {"fill", "pixelate", "blur"} and {c["region"] for c in cases.values()} == {"box", "ellipse", "mesh", "map"}
    for name, case in cases.items():
        image = ac.view_of(case["buffer"], case["width"])
        assert not image.flags["C_CONTIGUOUS"] and image.strides[0] > 3 * image.shape[1], name  # a pitched view
        want = ac.expected(name, case)
        assert want.shape == image.shape and want.dtype == np.uint8
        if name not in ("no_heads", "pixelate_identity", "blur_r0", "raw_asymmetric_mass"):  # those four are identities
            assert not np.array_equal(want, image), name
    H, W = ac.H, ac.W
    assert H % 2 == 1 and W % 2 == 1 and W % 64 and H % 4 and (ac.LEFT * 3) % 4  # odd, no tile multiple, a source that starts off a dword
    assert ac.buffer_of("checker").min() == 0 and ac.buffer_of("checker").max() == 255
    boxes = [ref.geometry_box(b, 0.1) for b in ac.EDGE_BOXES]
    assert boxes[0][0] < 0 < boxes[0][2] and boxes[1][0] < W < boxes[1][2] and boxes[2][1] < 0 < boxes[2][3] and boxes[3][1] < H < boxes[3][3]
    odd = [ref.geometry_box(b, 0.1) for b in ac.ODD_BOXES]
    assert odd[0][0] >= W and odd[1][2] <= 0 and odd[2][0] == odd[2][2] and odd[3][1] == odd[3][3] and odd[4] == (70, 60, 71, 61) and odd[5][0] < 0 and odd[5][2] > W and odd[5][1] < 0 and odd[5][3] > H
    for name in ("odd_fill_box", "odd_pixelate_ellipse"):
        assert np.array_equal(ac.owner_of(cases[name], odd) >= 0, ac.owner_of(cases[name], odd) >= 4)  # outside and zero-sided boxes own nothing
    over = ac.owner_of(cases["overlap_fill_box"], [ref.geometry_box(b, 0.0) for b in ac.OVERLAP_BOXES])
    assert over[50, 60] == 2 and over[40, 50] == 3 and over[25, 25] == 1 and over[12, 12] == 0 and over[5, 5] == -1  # the later head owns the overlap; nested ones show
    assert ac.rows_of(cases["pixelate_identity"])[1] == [1] and np.array_equal(ac.expected("pixelate_identity", cases["pixelate_identity"]), ac.view_of(cases["pixelate_identity"]["buffer"]))
    assert ac.rows_of(cases["pixelate_ragged"])[1] == [8] and 50 % 8 and 31 % 8
    (b64,), (c64,), _ = ac.rows_of(cases["pixelate_64"])
    assert cases["pixelate_64"]["cells"] == 64 and c64 == 3 and -(-(b64[2] - b64[0]) // c64) == 47
    radii = {name: len(ac.rows_of(cases[name])[2][0]) - 1 for name in ("blur_r0", "blur_r1", "blur_r70", "blur_all_clamp")}
    assert radii == {"blur_r0": 0, "blur_r1": 1, "blur_r70": 70, "blur_all_clamp": 150} and 150 > max(H, W)
    assert np.array_equal(ac.expected("blur_r0", cases["blur_r0"]), ac.view_of(cases["blur_r0"]["buffer"]))
    assert cases["raw_asymmetric_mass"]["tap_tables"] == [[65534, 1]]
    assert len(cases["no_heads"]["heads"]) == 0 and np.array_equal(ac.expected("no_heads", cases["no_heads"]), ac.view_of(cases["no_heads"]["buffer"]))
    assert len(cases["one_head"]["heads"]) == 1 and len(cases["many_heads_blur"]["heads"]) == 300 and cases["many_heads_blur"]["buffer"].shape[0] == cases["many_heads_blur"]["width"] == 64
    own = cases["owner_fill"]["owner"]
    assert (own == -1).any() and (own == 7).any() and (own == -5).any() and own[0, 120] == 1
    filled = ac.expected("owner_fill", cases["owner_fill"])
    image = ac.view_of(cases["owner_fill"]["buffer"])
    assert np.array_equal(filled[0:3, 100:131], image[0:3, 100:131]) and np.array_equal(filled[20:30, 20:30], image[20:30, 20:30]) and np.array_equal(filled[5:10, 5:70], image[5:10, 5:70])
    assert (filled[10:50, 10:60][own[10:50, 10:60] == 0] == (0, 255, 0)).all() and (own[10:50, 10:60] == 0).any()
    mesh = cases["mesh_fill"]
    mo = ac.owner_of(mesh, None)
    b0, b1 = ac.rows_of(mesh)[0]
    assert (mo == 0).any() and (mo == 1).any() and b0[0] < b1[2] and b1[0] < b0[2] and b0[1] < b1[3] and b1[1] < b0[3]  # two silhouettes, overlapping bounds
    for i, (x0, y0, x1, y1) in enumerate((b0, b1)):  # the bounds hold the silhouette
        ys, xs = np.nonzero(mo == i)
        assert x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1
