"""Host half of head tensors (head_detector_amd/head_tensors.py, include/vgh_crop.h): the ABI of libvghcrop.so, the plan against hand-computed heads, the matrices
against the composite map, facts of the restatement (tests/head_tensors_ref.py: the identity, the ramp check, the sum bound), every planted case against what it
claims to contain, the argument errors and their order, and csrc/head_crop_rules.h under the host sanitizers (tests/head_crop_host.hip: a program of its own,
never run through Python, never on a GPU).  No GPU."""
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_tensors_cases as hc  # noqa: E402
import head_tensors_ref as ref  # noqa: E402

from head_detector_amd import _lib_crop, aligned, head_tensors as ht  # noqa: E402
from head_detector_amd._lib import VghError  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "head_detector_amd")
C = _lib_crop.C
WANT = {"vghc_version", "vghc_last_error", "vghc_head_tensors"}
ONE = 1 << 32
HALF_FRACTION = 1 << 26


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


# ---- the library ----------------------------------------------------------------------------------------------------------------------------------
def test_crop_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_crop.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghc_[a-z0-9_]+)\s*\(", code))
    assert declared == WANT == set(_lib_crop.SYMBOLS)
    assert _exported(_lib_crop.LIB_PATH) == WANT  # hidden visibility: nothing of companion_host.h, no kernel stub
    assert _lib_crop.load().vghc_version().startswith(b"vghcrop")
    for name, value in (("VGHC_MAX_SIZE", _lib_crop.MAX_SIZE), ("VGHC_MAX_SUPERSAMPLE", _lib_crop.MAX_SUPERSAMPLE), ("VGHC_MAX_HEADS", _lib_crop.MAX_HEADS),
                        ("VGHC_MAX_SIDE", _lib_crop.MAX_SIDE), ("VGHC_MAX_TILES", _lib_crop.MAX_TILES), ("VGHC_SOURCE_RGB", _lib_crop.SOURCE_RGB),
                        ("VGHC_SOURCE_YUV420", _lib_crop.SOURCE_YUV420), ("VGHC_DTYPE_U8", _lib_crop.DTYPES["uint8"]), ("VGHC_DTYPE_F32", _lib_crop.DTYPES["float32"]),
                        ("VGHC_DTYPE_F16", _lib_crop.DTYPES["float16"]), ("VGHC_DTYPE_BF16", _lib_crop.DTYPES["bfloat16"]), ("VGHC_LAYOUT_NCHW", _lib_crop.LAYOUTS["nchw"]),
                        ("VGHC_LAYOUT_NHWC", _lib_crop.LAYOUTS["nhwc"]), ("VGHC_ORDER_RGB", _lib_crop.ORDERS["rgb"]), ("VGHC_ORDER_BGR", _lib_crop.ORDERS["bgr"])):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    assert (_lib_crop.MAX_SIZE, _lib_crop.MAX_SUPERSAMPLE, _lib_crop.MAX_HEADS, _lib_crop.MAX_SIDE) == (1024, 8, 65536, 32767)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64}

    def fields(struct):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", code, flags=re.S).group(1)
        out = []
        for line in body.split(";"):
            m = re.match(r"\s*(?:const )?(\w+)\s*(\*?)\s*(.+)$", line.strip(), flags=re.S)
            if not m:
                continue
            for name in m.group(3).split(","):
                name = name.strip()
                star = bool(m.group(2)) or name.startswith("*")
                array = re.match(r"(\w+)\[(\d+)\]", name.lstrip("*"))
                out.append((array.group(1), ("float", int(array.group(2)))) if array else (name.lstrip("*"), C.c_void_p if star else kinds[m.group(1)]))
        return out

    assert fields("vghc_source") == list(_lib_crop.Source._fields_)
    job = fields("vghc_job")
    assert [n for n, _ in job] == [n for n, _ in _lib_crop.Job._fields_]
    assert [k if not isinstance(k, tuple) else C.c_float * k[1] for _, k in job] == [k for _, k in _lib_crop.Job._fields_]
    head = fields("vghc_head")
    assert [n for n, _ in head] == list(_lib_crop.HEAD_DTYPE.names) == ["x0", "xp", "xq", "y0", "yp", "yq", "source", "supersample", "a", "reserved"]
    assert _lib_crop.HEAD_DTYPE["a"].shape == (3,) and _lib_crop.HEAD_DTYPE["a"].base == np.float32 and _lib_crop.HEAD_DTYPE["x0"] == np.int64
    assert (C.sizeof(_lib_crop.Source), C.sizeof(_lib_crop.Job), _lib_crop.HEAD_DTYPE.itemsize) == (96, 72, 72)
    assert [_lib_crop.HEAD_DTYPE.fields[n][1] for n in _lib_crop.HEAD_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 68]  # C's layout: no padding


def test_the_library_is_declared_in_the_build():
    from head_detector_amd import build

    assert build.DOWNSTREAM == [build.Companion("libvghcrop.so", ["head_tensors.hip"], build.HOST_HEADERS + ["head_crop_rules.h"], "vgh_crop.h", ["-ffp-contract=off"], "build_crop")]
    # the three older lists are what they were
    assert [(c.lib, c.sources, c.headers, c.public, c.flags, c.objdir) for c in build.COMPANIONS] == [
        ("libvgheval.so", ["mesh_metrics.hip", "detection_ap.hip"], ["companion_host.h"], "vgh_eval.h", ["-ffp-contract=off"], "build_eval"),
        ("libvghmerge.so", ["slice_merge.hip"], ["companion_host.h"], "vgh_merge.h", ["-ffp-contract=off"], "build_merge"),
        ("libvghtrack.so", ["head_track.hip"], ["companion_host.h"], "vgh_track.h", ["-ffp-contract=off"], "build_track"),
        ("libvghtex.so", ["texture.hip"], ["companion_host.h", "tile_fold.h"], "vgh_tex.h", [], "build_tex"),
        ("libvghvis.so", ["visibility.hip"], ["companion_host.h", "tile_fold.h"], "vgh_vis.h", [], "build_vis"),
        ("libvghview.so", ["aligned.hip", "draw.hip", "mesh_render.hip"], ["companion_host.h", "tile_fold.h"], "vgh_view.h", [], "build_view")]
    assert build.APPLICATIONS == [build.Companion("libvghanon.so", ["anonymize.hip"], ["companion_host.h", "head_rows.h"], "vgh_anon.h", [], "build_anon")]
    assert build.VIDEO == [build.Companion("libvghvideo.so", ["yuv_anonymize.hip", "yuv_pack.hip"], ["companion_host.h", "head_rows.h", "plane_views.h"], "vgh_video.h", [], "build_video")]
    assert "head_detector_amd/build_crop/" in open(os.path.join(ROOT, ".gitignore")).read().split()
    src = open(os.path.join(PKG, "csrc", "head_tensors.hip")).read()
    rules = open(os.path.join(PKG, "csrc", "head_crop_rules.h")).read()
    assert '#include "companion_host.h"' in src and '#include "head_crop_rules.h"' in src
    assert "static_assert(VGHC_OK == OK && VGHC_ERR_INVALID == ERR_INVALID && VGHC_ERR_HIP == ERR_HIP && VGHC_ERR_NOMEM == ERR_NOMEM," in src
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/vgh_crop.h", "companion_host.h", "head_crop_rules.h"]  # no other library's header
    # the rule header is HIP-free and holds what must not exist twice
    assert re.findall(r"#include\s+(\S+)", rules) == ["<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/vgh_crop.h"']
    assert re.findall(r"#include\s+(\S+)", open(os.path.join(ROOT, "include", "vgh_crop.h")).read()) == ["<stdint.h>"]
    for once in ("int64_t sub_position(", "int32_t tap4(", "int32_t round_u8(", "int32_t yuv_channel(", "const char* validate(", "int64_t tile_count(", "static_assert(255ll * kWeightSum"):
        assert once in rules and once not in src, once
    for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "hipMalloc(", "set_error(const char", "g_error", "asm", "dlopen", "hipFuncSetAttribute",
                    "extern __shared__", "fmaf(", "__fmaf"):
        assert by_hand not in src and by_hand not in rules, by_hand
    host = open(os.path.join(ROOT, "tests", "head_crop_host.hip")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["../head_detector_amd/csrc/head_crop_rules.h"] and "hip" not in " ".join(re.findall(r"#include <([^>]+)>", host))
    # nobody else exports the prefix, it links none of the others, and no other binding names it
    libs = sorted(f for f in os.listdir(PKG) if f.startswith("libvgh") and f.endswith(".so") and f not in ("libvgh_exp.so", "libvgh_var.so"))
    assert set(libs) >= {"libvgh.so", "libvghview.so", "libvghvis.so", "libvghtex.so", "libvgheval.so", "libvghmerge.so", "libvghtrack.so", "libvghanon.so", "libvghvideo.so",
                         "libvghcrop.so"}
    for f in libs:
        if f != "libvghcrop.so":
            assert not [s for s in _exported(os.path.join(PKG, f)) if s.startswith("vghc_")], f
    ldd = subprocess.run(["ldd", _lib_crop.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvgh" not in ldd
    bindings = sorted(f for f in os.listdir(PKG) if f.startswith("_lib") and f.endswith(".py") and f != "_lib_crop.py")
    assert len(bindings) == 9
    for f in bindings + ["_companion.py"]:
        text = open(os.path.join(PKG, f)).read()
        assert "libvghcrop" not in text and "_lib_crop" not in text, f


def test_host_rules_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "head_crop_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "head_crop_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "head crop host checks passed" in r.stdout, r.stdout + r.stderr


def test_an_invalid_job_is_refused_before_a_gpu_is_looked_for():
    lib = _lib_crop.load()
    mem = np.zeros(4096, np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16
    source = (_lib_crop.Source * 1)()
    source[0].kind, source[0].h, source[0].w, source[0].rgb_dev, source[0].rgb_pitch_bytes = 0, 8, 8, base, 24
    rows = np.zeros(1, _lib_crop.HEAD_DTYPE)
    rows["xp"], rows["yq"], rows["supersample"] = ONE, ONE, 1

    def job(**over):
        j = _lib_crop.Job()
        j.sources, j.heads, j.n_sources, j.n_heads, j.size, j.dtype, j.dst_dev, j.dst_bytes = C.addressof(source), rows.ctypes.data, 1, 1, 4, 0, base + 1024, 48
        for k, v in over.items():
            setattr(j, k, v)
        return j

    for over, words in ((dict(size=0), b"size 0"), (dict(size=1025), b"size 1025"), (dict(n_heads=65537), b"n_heads 65537"), (dict(dst_bytes=47), b"needs 48 bytes"),
                        (dict(dtype=7), b"unknown dtype 7"), (dict(dst_dev=None), b"null dst_dev"), (dict(heads=None), b"null heads"), (dict(fill=1 << 24), b"fill")):
        assert lib.vghc_head_tensors(job(**over), None) == -1 and words in lib.vghc_last_error(), words
    rows["x0"] = 1 << 62
    assert lib.vghc_head_tensors(job(), None) == -1 and b"head 0: |x0| + S K (|xp| + |xq|) reaches 2^62" in lib.vghc_last_error()
    rows["x0"], rows["supersample"] = 0, 9
    assert lib.vghc_head_tensors(job(), None) == -1 and b"supersample 9" in lib.vghc_last_error()
    assert lib.vghc_head_tensors(None, None) == -1 and b"null job" in lib.vghc_last_error()
    assert not mem.any()


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------
def _plan(boxes, size, **kw):
    return ht.head_tensor_plan((97, 131, 3), [hc.box_head(b) for b in boxes], size, aligned=False, **kw)


def test_plan_matches_hand_computed_heads():
    # scale 1 on integer coordinates: K = 1, sub-sample 0 at the rect's first pixel centre
    p = _plan([(10, 20, 30, 30)], 30, margin=0.0)
    assert p.coefficients.tolist() == [[10 * ONE + HALF_FRACTION, ONE, 0, 20 * ONE + HALF_FRACTION, 0, ONE]] and p.supersample.tolist() == [1] and p.sides.tolist() == [30]
    assert p.coefficients.dtype == np.int64 and p.supersample.dtype == np.int32 and p.matrices.dtype == np.float64 and p.size == 30 and len(p) == 1
    # side 24 at S = 16: K = 2, sub-samples 0.75 apart, the first at 10 + 0.375 - 0.5
    p = _plan([(10, 20, 24, 24)], 16, margin=0.0)
    assert p.coefficients.tolist() == [[int(9.875 * ONE) + HALF_FRACTION, 3 * ONE // 4, 0, int(19.875 * ONE) + HALF_FRACTION, 0, 3 * ONE // 4]] and p.supersample.tolist() == [2]
    assert np.array_equal(p.matrices[0], [[1.5, 0.0, 10.25], [0.0, 1.5, 20.25]])  # crop pixel 0 covers canvas [9.5, 11): its centre is 10.25
    # the margin and the square: (10, 20, 30, 40) grows to (7, 16, 36, 48), the square is (1, 16, 48, 48)
    p = _plan([(10, 20, 30, 40)], 48)
    assert p.coefficients.tolist() == [[ONE + HALF_FRACTION, ONE, 0, 16 * ONE + HALF_FRACTION, 0, ONE]] and p.sides.tolist() == [48]
    # K: ceil(side / S), at most 8, at least 1; forced values are taken as they are
    assert _plan([(0, 0, 48, 48), (0, 0, 49, 49), (0, 0, 5, 5), (0, 0, 1000, 1000), (0, 0, 0, 0)], 12, margin=0.0).supersample.tolist() == [4, 5, 1, 8, 1]
    assert _plan([(0, 0, 48, 48), (0, 0, 5, 5)], 12, margin=0.0, supersample=3).supersample.tolist() == [3, 3]
    p = _plan([(1, 16, 48, 48)], 12, margin=0.0, supersample=4)  # 48 sub-samples a side, one per pixel
    assert p.coefficients.tolist() == [[ONE + HALF_FRACTION, ONE, 0, 16 * ONE + HALF_FRACTION, 0, ONE]]
    # a rect of side 0 becomes one pixel: 7 sub-samples a seventh of a pixel apart, centred on it
    p = _plan([(50, 40, 0, 0)], 7, margin=0.0)
    assert p.sides.tolist() == [1] and p.supersample.tolist() == [1] and p.coefficients[0, 1] == int(np.rint(ONE / 7)) and p.coefficients[0, 2] == 0
    assert p.coefficients[0, 0] == int(np.rint((50 + 0.5 / 7 - 0.5) * ONE)) + HALF_FRACTION
    # far away: positions beyond int32, nothing wraps
    p = _plan([(40000, -40000, 30, 30)], 15, margin=0.0)
    assert p.coefficients[0, 0] == int((40000 + 0.5 - 0.5) * ONE) + HALF_FRACTION and p.coefficients[0, 3] == -40000 * ONE + HALF_FRACTION and p.coefficients[0, 1] == ONE
    assert len(_plan([], 16)) == 0 and _plan([], 16).matrices.shape == (0, 2, 3)
    # aligned=True is get_aligned_heads' geometry: the matrix and the rect of aligned_head_plan, margin = its offset
    heads = [hc.mesh_head(60.0, 50.0, 25.0, 30.0, seed=1), hc.mesh_head(40.0, 60.0, 12.0, 77.0, yaw=75.0, seed=3)]
    for margin in (0.1, 0.25):
        p = ht.head_tensor_plan((97, 131, 3), heads, 16, head_indices=hc.HIDX, margin=margin)
        theirs = aligned.aligned_head_plan((97, 131, 3), heads, hc.HIDX, offset=margin)
        assert [t.rotated for t in theirs] == [True, False] and p.sides.tolist() == [t.rect[2] for t in theirs] and all(t.rect[2] == t.rect[3] for t in theirs)
    assert aligned.aligned_head_plan((97, 131, 3), heads, hc.HIDX)[0].rect == aligned.aligned_head_plan((97, 131, 3), heads, hc.HIDX, offset=0.1)[0].rect


def test_matrices_are_the_composite_map():
    """Crop pixel centre -> canvas point of the rect -> invert_affine(matrix): ``matrices``, ``to_image`` and the mean of a pixel's sub-sample positions agree."""
    heads = [hc.mesh_head(60.0, 50.0, 25.0, 30.0, seed=1), hc.mesh_head(70.0, 40.0, 30.0, -170.0, seed=2), hc.mesh_head(40.0, 60.0, 12.0, 77.0, yaw=75.0, seed=3)]
    S = 17
    p = ht.head_tensor_plan((97, 131, 3), heads, S, head_indices=hc.HIDX)
    theirs = aligned.aligned_head_plan((97, 131, 3), heads, hc.HIDX)
    t = ht.HeadTensors(None, p.matrices, p.supersample, np.zeros(3, np.int64))
    jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    crop_points = np.stack([jj.ravel(), ii.ravel()], axis=1)
    for k, plan in enumerate(theirs):
        x, y, side, _ = plan.rect
        canvas = np.stack([x + (crop_points[:, 0] + 0.5) * side / S - 0.5, y + (crop_points[:, 1] + 0.5) * side / S - 0.5], axis=1)
        a00, a01, b0, a10, a11, b1 = aligned.invert_affine(plan.matrix)
        want = np.stack([a00 * canvas[:, 0] + a01 * canvas[:, 1] + b0, a10 * canvas[:, 0] + a11 * canvas[:, 1] + b1], axis=1)
        assert np.abs(t.to_image(crop_points, k) - want).max() < 1e-9, k
        # forward again: the plan's own matrix brings the image point back to the canvas point
        back = want @ plan.matrix[:, :2].T + plan.matrix[:, 2]
        assert np.abs(back - canvas).max() < 1e-8, k
        # the K^2 sub-samples of a pixel are symmetric about that point (2^26 is the rounding offset of the fraction, not a shift)
        K = int(p.supersample[k])
        X0, XP, XQ, Y0, YP, YQ = (int(v) for v in p.coefficients[k])
        for j, i in ((0, 0), (S - 1, 0), (5, 11), (S - 1, S - 1)):
            px = np.mean([X0 - HALF_FRACTION + (j * K + a) * XP + (i * K + b) * XQ for a in range(K) for b in range(K)]) / ONE
            py = np.mean([Y0 - HALF_FRACTION + (j * K + a) * YP + (i * K + b) * YQ for a in range(K) for b in range(K)]) / ONE
            assert abs(px - want[i * S + j, 0]) < 1e-6 and abs(py - want[i * S + j, 1]) < 1e-6, (k, j, i)
    assert theirs[0].rotated and theirs[1].rotated and not theirs[2].rotated and abs(p.matrices[1][0, 0]) > 0.5 and p.matrices[1][0, 0] < 0  # -170 degrees: upside down


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def test_identity_crop_is_the_source_slice():
    """K = 1, S = side, no rotation: a uint8 NHWC crop equals the source slice byte for byte (and the other dtypes are its normalisation)."""
    img = hc.rgb_of(hc.rgb_source())
    for (x, y, side) in ((10, 20, 33), (0, 0, 97), (98, 64, 33)):
        p = _plan([(x, y, side, side)], side, margin=0.0)
        assert p.supersample.tolist() == [1]
        s = ref.sums([img], p.coefficients, p.supersample, [0], side)
        got = ref.finish(s, p.supersample, "uint8", "nhwc")
        assert got.dtype == np.uint8 and np.array_equal(got[0], img[y:y + side, x:x + side])
        assert np.array_equal(ref.finish(s, p.supersample, "uint8", "nchw")[0], img[y:y + side, x:x + side].transpose(2, 0, 1))
        assert np.array_equal(ref.sums([img], p.coefficients, p.supersample, [0], side, order="bgr")[..., ::-1], s)
        f = ref.finish(s, p.supersample, "float32", "nhwc", scale=1.0, mean=(0, 0, 0), std=(1, 1, 1))
        assert f.dtype == np.float32 and np.array_equal(f[0], img[y:y + side, x:x + side].astype(np.float32))


def _ramp(h, w, grads, offsets):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.stack([o + gx * x + gy * y for (gx, gy), o in zip(grads, offsets)], axis=-1)
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8)


def test_ramp_check_of_the_restatement():
    """On images v = gx x + gy y every uint8 output pixel whose taps all lie inside the image is within (|gx| + |gy|) / 64 + 0.5 + 1e-3 of the ramp at the mapped
    pixel centre: the position is quantised to 1/32 pixel, rounded to nearest (1/64 a coordinate), bilinear interpolation of a ramp is exact, the sub-samples
    are symmetric about the centre, and one byte rounding is applied.  A restatement that is consistently half a pixel off fails this by |gx| / 2."""
    h, w = 97, 131
    grads, offsets = [(1, 1), (-1, 1), (-1, -1)], [0, 140, 230]
    img = _ramp(h, w, grads, offsets)
    checked = 0
    plans = [ht.head_tensor_plan(img.shape, [hc.mesh_head(60.0, 50.0, 25.0, 30.0, seed=1), hc.mesh_head(70.0, 40.0, 30.0, -170.0, seed=2)], 17, head_indices=hc.HIDX),
             _plan([(10, 20, 33, 33), (5, 9, 60, 41), (-20, 30, 40, 40), (70, 30, 35, 50)], 16), _plan([(3, 4, 90, 80)], 7, supersample=3), _plan([(40, 30, 9, 9)], 33),
             _plan([(20, 10, 64, 64)], 16, supersample=8, margin=0.0)]
    for p in plans:
        S, n = p.size, len(p)
        got = ref.finish(ref.sums([img], p.coefficients, p.supersample, np.zeros(n, np.int64), S), p.supersample, "uint8", "nhwc").astype(np.float64)
        t = ht.HeadTensors(None, p.matrices, p.supersample, np.zeros(n, np.int64))
        jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
        for k in range(n):
            K = int(p.supersample[k])
            X0, XP, XQ, Y0, YP, YQ = (int(v) for v in p.coefficients[k])
            pp, qq = np.arange(S * K, dtype=np.int64)[None, :], np.arange(S * K, dtype=np.int64)[:, None]
            sx, sy = (X0 + pp * XP + qq * XQ) >> 32, (Y0 + pp * YP + qq * YQ) >> 32
            inside = ((sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)).reshape(S, K, S, K).all(axis=(1, 3))
            centre = t.to_image(np.stack([jj.ravel(), ii.ravel()], axis=1), k).reshape(S, S, 2)
            for c, ((gx, gy), o) in enumerate(zip(grads, offsets)):
                want = o + gx * centre[..., 0] + gy * centre[..., 1]
                err = np.abs(got[k, :, :, c] - want)[inside]
                assert err.size == 0 or err.max() <= (abs(gx) + abs(gy)) / 64 + 0.5 + 1e-3, (S, k, c, float(err.max()))
            checked += int(inside.sum())
    assert checked > 1500


def test_sum_bound_at_its_extreme():
    """K = 8 on an all-255 image with every tap inside: every sum is 255 * 1024 * 64 = 16 711 680 < 2^24, exactly a float32, and the uint8 result is 255."""
    c = hc.cases()["sum_at_its_bound"]
    s, ks = hc.expected_sums(c)
    assert ks.tolist() == [8] and s.min() == s.max() == ref.MAX_SUM == 16711680 < 2 ** 24
    assert int(np.float32(ref.MAX_SUM)) == ref.MAX_SUM and int(np.float32(ref.MAX_SUM - 1)) == ref.MAX_SUM - 1
    assert 255 * 1024 * 81 >= 2 ** 24  # K = 9 would not fit
    assert (ref.finish(s, ks, "uint8", "nhwc") == 255).all()
    f = ref.finish(s, ks, "float32", "nchw", scale=1.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    assert (f == 255.0).all()  # a = 2^-16 exactly
    # the rounding of the mean: half goes up
    assert ref.finish(np.array([[[[511, 512, 1024 * 64 * 3 + 32767]]]], np.int32), [1], "uint8", "nhwc").tolist() == [[[[0, 1, 224]]]]
    # float: two operations, rounded separately (not one fused multiply-add)
    a, b = ref.coefficients_a_b([1], 1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    s1 = np.array([[[[100 * 1024 + 3, 200 * 1024 + 77, 17 * 1024 + 1]]]], np.int32)
    f = ref.finish(s1, [1], "float32", "nhwc")
    assert np.array_equal(f[0, 0, 0], np.float32(s1[0, 0, 0].astype(np.float32) * a[0]) + b)
    assert np.array_equal(ref.finish(s1, [1], "bfloat16", "nhwc"), torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_every_planted_case_contains_what_it_claims():
    cases = hc.cases()
    assert len(cases) >= 22
    sizes = {c["size"] for c in cases.values()}
    forced = {c["supersample"] for c in cases.values()}
    assert sizes == {1, 7, 16, 17, 33} and forced == {1, 2, 3, 8, "auto"}
    shapes = {hc.rgb_of(s).shape[:2] for c in cases.values() for s, _ in c["pairs"]}
    assert {(97, 131), (64, 64), (2, 3), (1, 1)} <= shapes
    for name, c in cases.items():
        for source, _ in c["pairs"]:
            if source["kind"] == "rgb":  # a pitched view: bytes between width and pitch
                assert source["buffer"].shape[1] == source["width"] + hc.EXTRA and hc.LEFT > 0
            else:
                assert source["pitch"] > source["width"] and (source["height"] % 2 == 1 or source["width"] % 2 == 1), name
    layouts = {(s["layout"], s["full_range"]) for c in cases.values() for s, _ in c["pairs"] if s["kind"] == "yuv"}
    assert {l for l, _ in layouts} == {"nv12", "nv21", "i420"} and {r for _, r in layouts} == {True, False}
    coefficients, ks, index, matrices = hc.plan_of(cases["upright_identity"])
    assert ks.tolist() == [1] and coefficients[0].tolist() == [10 * ONE + HALF_FRACTION, ONE, 0, 20 * ONE + HALF_FRACTION, 0, ONE]
    assert hc.plan_of(cases["S16_auto"])[1].tolist() == [7, 2, 3]
    for name, lo in (("roll_30", 0.4), ("roll_minus_170", 0.1)):  # rotated: off-diagonal terms
        m = hc.plan_of(cases[name])[3][0]
        assert abs(m[0, 1]) > lo * abs(m[0, 0]) > 0, name
    assert hc.plan_of(cases["roll_minus_170"])[3][0][0, 0] < 0 and hc.plan_of(cases["roll_minus_170"])[3][1][0, 1] == 0  # the profile head is not rotated
    fill = np.array(cases["wholly_outside"]["fill"])
    s, ks = hc.expected_sums(cases["wholly_outside"])
    assert (s == fill * 1024 * 4).all()  # nothing but fill
    s, ks = hc.expected_sums(cases["half_outside"])
    u = ref.finish(s, ks, "uint8", "nhwc")
    assert (u[0, :, 0] == fill).all() and not (u[0, :, -1] == fill).all() and (u[1, 0, :] == fill).all() and (u[2, -1, :] == fill).all()
    s, ks = hc.expected_sums(cases["far_away"])
    assert (s[0] == fill * 1024 * 9).all() and (s[1] == fill * 1024 * 25).all() and not (s[2] == fill * 1024 * 9).all()
    far = hc.plan_of(cases["far_away"])[0]
    assert min(abs(int(far[0, 0])), abs(int(far[0, 3])), abs(int(far[1, 0]))) > 2 ** 31 * 1000 and far[1, 0] < 0  # positions far beyond int32, of both signs
    assert hc.plan_of(cases["side_0"])[1].tolist() == [1, 1] and len(cases["many_heads"]["pairs"][0][1]) == 300 and hc.rgb_of(cases["many_heads"]["pairs"][0][0]).shape == (64, 64, 3)
    assert len(cases["no_heads"]["pairs"][0][1]) == 0 and hc.expected_sums(cases["no_heads"])[0].shape == (0, 16, 16, 3)
    for name in ("i420_full_saturating", "nv12_saturating"):
        src = cases[name]["pairs"][0][0]
        assert set(np.unique(src["y"])) <= {0, 255} and {0, 255} <= set(np.unique(hc.rgb_of(src)))
    assert hc.expected_sums(cases["nv12_saturating"])[0].max() > 0.9 * ref.MAX_SUM
    two = cases["two_sources"]
    assert [s["kind"] for s, _ in two["pairs"]] == ["rgb", "rgb", "yuv", "rgb"] and hc.plan_of(two)[2].tolist() == [0, 0, 2, 3]
    assert len({hc.rgb_of(s).shape for s, _ in two["pairs"]}) == 4
    for name, c in cases.items():  # the two channel orders differ wherever the picture is not grey, and agree after flipping
        rgb, ks = hc.expected_sums(c, "rgb")
        bgr, _ = hc.expected_sums(c, "bgr")
        flipped = dict(c, fill=c["fill"][::-1])
        assert np.array_equal(hc.expected_sums(flipped, "bgr")[0][..., ::-1], rgb), name
        if rgb.size and name not in ("sum_at_its_bound", "wholly_outside"):  # (a white picture and a crop of nothing but fill look the same in both orders)
            assert not np.array_equal(bgr, rgb), name  # a channel swap shows
        if name in ("wholly_outside", "half_outside", "far_away"):
            assert not np.array_equal(bgr[..., ::-1], rgb), name  # the fill is in the OUTPUT's order: it does not swap with the picture


# ---- the arguments --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_their_order():
    image = np.zeros((40, 50, 3), np.uint8)
    heads = [hc.box_head((5, 5, 10, 10)), hc.box_head((1, 1, 4, 4))]
    res = PredictionResult(image, heads)
    calls = (lambda **kw: ht.head_tensors(image, heads, **kw), lambda **kw: res.get_head_tensors(**kw), lambda **kw: ht.head_tensors_batch([res, res], **kw))
    for call in calls:
        for kw, words in ((dict(size=0), "size"), (dict(size=1025), "size"), (dict(size=22.5), "size"), (dict(supersample=0), "supersample"), (dict(supersample=9), "supersample"),
                          (dict(supersample="fine"), "supersample"), (dict(margin=-0.1), "margin"), (dict(margin=float("nan")), "margin"), (dict(dtype=torch.int32), "dtype"),
                          (dict(dtype="float32"), "dtype"), (dict(layout="chw"), "layout"), (dict(channel_order="gbr"), "channel_order"), (dict(mean=(0.5, 0.5)), "mean"),
                          (dict(mean=(0.5, 0.5, float("inf"))), "mean"), (dict(std=(1.0, 0.0, 1.0)), "std"), (dict(std=1.0), "std"), (dict(scale=float("nan")), "scale"),
                          (dict(fill=(0, 0, 256)), "fill"), (dict(fill=(0, 0.5, 0)), "fill"), (dict(fill=(0, 0)), "fill"),
                          (dict(out=torch.zeros(2, 3, 16, 16), size=8), "out"), (dict(out=torch.zeros(2, 3, 8, 8, dtype=torch.float16), size=8), "out"),
                          (dict(out=torch.zeros(2, 3, 8, 16)[..., ::2], size=8), "out")):
            with pytest.raises(ValueError, match=words):  # ... also where head_indices is missing: the arguments come first
                call(**kw)
        with pytest.raises(FileNotFoundError, match="head_indices.npy"):  # then the asset, worded like get_aligned_heads
            call()
        if not torch.cuda.is_available():  # and only then the missing GPU
            with pytest.raises(VghError, match="need a GPU"):
                call(aligned=False)
            with pytest.raises(VghError, match="need a GPU"):
                call(aligned=False, size=8, out=torch.zeros(2 if call is not calls[2] else 4, 3, 8, 8))
    for bad, words in ((np.zeros((40, 50), np.uint8), "source"), (np.zeros((40, 50, 3), np.float32), "source"), (np.zeros((40, 50, 4), np.uint8), "source"),
                       (np.zeros((0, 50, 3), np.uint8), "sides"), (None, "source"), ("image.png", "source")):
        with pytest.raises(ValueError, match=words):
            ht.head_tensors(bad, heads, aligned=False)
    with pytest.raises(ValueError, match="source"):  # a result without an image and without a frame
        PredictionResult(None, heads).get_head_tensors(aligned=False)
    with pytest.raises(ValueError, match="result 1 has neither"):
        ht.head_tensors_batch([res, PredictionResult(None, heads)], aligned=False)
    with pytest.raises(ValueError, match="image_shape"):
        ht.head_tensor_plan((40000, 50), heads, 16, aligned=False)
    with pytest.raises(ValueError, match="head 1: its crop reaches more than 2\\^29 pixels"):
        ht.head_tensor_plan((40, 50), [heads[0], hc.box_head((1 << 30, 0, 10, 10))], 16, aligned=False)
    with pytest.raises(FileNotFoundError):
        ht.head_tensor_plan((40, 50), heads, 16)
    # the tracker's results carry the method too, and a frame result needs no original_image
    from head_detector_amd.tracking import TrackedPredictionResult

    assert TrackedPredictionResult.get_head_tensors is PredictionResult.get_head_tensors
    frame = types.SimpleNamespace()  # stands for a frame: the arguments are looked at before the source's planes
    with pytest.raises(ValueError, match="size"):
        PredictionResult(None, heads, source_frame=frame).get_head_tensors(size=0)
