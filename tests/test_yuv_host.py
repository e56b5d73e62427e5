"""CPU: the host side of VGH_IMG_YUV420_RAW (NV12 / NV21 / I420 video frames converted inside the device letterbox) -- the conversion rule of include/vgh.h
restated twice in NumPy (tests/yuv_ref.py) and once in torch (video.YUV420Frame.to_rgb), the pinned coefficient integers, the C ABI additions and their ctypes
mirror, and the errors the factories and the engine's image argument raise.  Everything is byte equality."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import yuv_ref
from conftest import ROOT
from head_detector_amd import _lib
from head_detector_amd.video import YUV420Frame, yuv_coefficients

# (matrix, full_range) -> (y_offset, cy, crv, cgu, cgv, cbu): literals, so that a change of the formula or of its rounding shows
COEFFICIENTS = {
    ("bt601", False): (16, 76309, 104597, -25675, -53279, 132201),
    ("bt601", True): (0, 65536, 91881, -22553, -46802, 116130),
    ("bt709", False): (16, 76309, 117489, -13975, -34925, 138438),
    ("bt709", True): (0, 65536, 103206, -12276, -30679, 121609),
    ("bt2020", False): (16, 76309, 110014, -12277, -42626, 140363),
    ("bt2020", True): (0, 65536, 96639, -10784, -37444, 123299),
}
SIZES = [(1, 1), (3, 5), (2, 2), (6, 4), (7, 9)]  # (h, w): odd sizes use the ceil chroma column / row


def test_coefficient_integers_are_pinned():
    assert {k: yuv_coefficients(*k) for k in COEFFICIENTS} == COEFFICIENTS
    assert yuv_coefficients() == COEFFICIENTS[("bt709", False)]
    with pytest.raises(ValueError):
        yuv_coefficients("bt470")
    for coef in COEFFICIENTS.values():
        assert 0 <= coef[0] <= 255 and all(abs(c) <= 1 << 20 for c in coef[1:])


@pytest.mark.parametrize("saturating", [False, True])
def test_loop_equals_vectorised_restatement(saturating):
    """Dense planes, pitched planes, and both chroma steps as views of NV12 / NV21 / I420 surfaces with an aligned chroma offset."""
    n = 0
    for (h, w), key in zip(SIZES, list(COEFFICIENTS)[:len(SIZES)]):
        coef = COEFFICIENTS[key]
        y, u, v = yuv_ref.picture(h, w, 10 * h + w, saturating)
        want = yuv_ref.yuv_to_rgb_loop(y, u, v, coef)
        assert np.array_equal(yuv_ref.yuv_to_rgb(y, u, v, coef), want)
        ch, cw = u.shape
        for layout in ("nv12", "nv21", "i420"):
            buf, pitch, off = yuv_ref.surface(layout, y, u, v, pitch=2 * cw + 6, extra_rows=3)
            yy = np.lib.stride_tricks.as_strided(buf, (h, w), (pitch, 1))
            if layout == "i420":
                cp = pitch // 2
                uu = np.lib.stride_tricks.as_strided(buf[off:], (ch, cw), (cp, 1))
                vv = np.lib.stride_tricks.as_strided(buf[off + cp * ch:], (ch, cw), (cp, 1))
            else:
                a = np.lib.stride_tricks.as_strided(buf[off:], (ch, cw), (pitch, 2))
                b = np.lib.stride_tricks.as_strided(buf[off + 1:], (ch, cw), (pitch, 2))
                uu, vv = (a, b) if layout == "nv12" else (b, a)
            assert np.array_equal(uu, u) and np.array_equal(vv, v) and np.array_equal(yy, y)
            assert np.array_equal(yuv_ref.yuv_to_rgb_loop(yy, uu, vv, coef), want) and np.array_equal(yuv_ref.yuv_to_rgb(yy, uu, vv, coef), want)
            n += 1
    assert n == 3 * len(SIZES)
    # extreme values with the largest admissible coefficients: the header's overflow bound holds (the loop asserts it) and both forms agree
    y, u, v = yuv_ref.picture(4, 6, 5, True)
    for sign in (1, -1):
        big = (255 if sign < 0 else 0, sign << 20, sign << 20, sign << 20, sign << 20, -sign << 20)
        assert np.array_equal(yuv_ref.yuv_to_rgb_loop(y, u, v, big), yuv_ref.yuv_to_rgb(y, u, v, big))


@pytest.mark.parametrize("saturating", [False, True])
def test_frame_to_rgb_equals_the_restatement_in_every_layout(saturating):
    """YUV420Frame.to_rgb() on CPU tensors == tests/yuv_ref.py; NV12, NV21 and I420 views of one picture give identical RGB; the factories build views, not copies."""
    for (h, w), (key, coef) in zip(SIZES + [(33, 20)], list(COEFFICIENTS.items())):
        y, u, v = yuv_ref.picture(h, w, 7 * h + w, saturating)
        want = yuv_ref.yuv_to_rgb(y, u, v, coef)
        kw = dict(matrix=key[0], full_range=key[1])
        ch, cw = u.shape
        frames = [YUV420Frame(torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(v), chroma_step=1, **kw)]
        for layout, make in (("nv12", YUV420Frame.from_nv12), ("nv21", YUV420Frame.from_nv21), ("i420", YUV420Frame.from_i420)):
            buf, pitch, off = yuv_ref.surface(layout, y, u, v)  # the default pitch and offset
            t = torch.from_numpy(buf)[:off + (pitch * ch if layout != "i420" else 2 * (pitch // 2) * ch)]
            f = make(t, h, w, **kw)
            assert f.y.data_ptr() == t.data_ptr() and f.chroma_step == (1 if layout == "i420" else 2)  # a view of the surface
            frames.append(f)
            buf, pitch, off = yuv_ref.surface(layout, y, u, v, pitch=2 * cw + 10, extra_rows=5)
            t = torch.from_numpy(buf)
            f = make(t, h, w, pitch=pitch, uv_offset=off, **kw)
            assert f.u.data_ptr() - t.data_ptr() == off + (1 if layout == "nv21" else 0)
            assert (f.y_pitch, f.uv_pitch) == (pitch, pitch // 2 if layout == "i420" else pitch)
            frames.append(f)
        uv = torch.from_numpy(np.stack([u, v], axis=-1).copy())
        frames.append(YUV420Frame.from_nv12((torch.from_numpy(y), uv), h, w, **kw))
        frames.append(YUV420Frame.from_nv21((torch.from_numpy(y), uv.flip(-1).contiguous().view(ch, 2 * cw)), h, w, **kw))
        frames.append(YUV420Frame.from_i420((torch.from_numpy(y), torch.from_numpy(u), torch.from_numpy(v)), h, w, **kw))
        for f in frames:
            assert f.shape == (h, w, 3) and f.coefficients == coef
            got = f.to_rgb()
            assert got.dtype == torch.uint8 and got.device.type == "cpu" and np.array_equal(got.numpy(), want), (h, w, f)


def test_grey_ramp_limited_and_full_range():
    """U = V = 128: limited range maps Y 16 -> 0 and 235 -> 255 (below and above saturate); full range maps Y -> Y."""
    y = torch.arange(256, dtype=torch.uint8).view(16, 16)
    c = torch.full((8, 8), 128, dtype=torch.uint8)
    for matrix in ("bt601", "bt709", "bt2020"):
        full = YUV420Frame(y, c, c, chroma_step=1, matrix=matrix, full_range=True).to_rgb()
        assert torch.equal(full, y.unsqueeze(-1).expand(16, 16, 3))
        lim = YUV420Frame(y, c, c, chroma_step=1, matrix=matrix).to_rgb().view(256, 3)
        assert (lim[:17] == 0).all() and (lim[235:] == 255).all()
        assert (lim[:, 0] == lim[:, 1]).all() and (lim[:, 0] == lim[:, 2]).all()
        assert (lim[1:, 0] >= lim[:-1, 0]).all() and int(lim[17, 0]) == 1 and int(lim[234, 0]) == 254


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vgh.h")).read(), flags=re.S)


def test_header_declares_the_format_and_the_abi_is_otherwise_unchanged():
    code = _code()
    assert re.search(r"#define\s+VGH_IMG_YUV420_RAW\s+3\b", code)
    assert re.search(r"typedef\s+struct\s+vgh_yuv420_image\s*\{[^}]*\}\s*vgh_yuv420_image\s*;", code)
    assert re.search(r"#define\s+VGH_ABI_VERSION\s+8\b", code)
    assert _lib.VGH_IMG_YUV420_RAW == 3 and _lib.RAW_FORMATS == (2, 3)
    assert _lib.ABI_VERSION == 8 == _lib.load().vgh_abi_version()
    assert len(_lib.SYMBOLS) == 86


def test_ctypes_yuv420_image_matches_the_c_layout(tmp_path):
    m = re.search(r"typedef\s+struct\s+vgh_yuv420_image\s*\{([^}]*)\}", _code())
    declared = []  # (c type, name) in order, from the header's text
    for stmt in m.group(1).split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = re.match(r"((?:const\s+)?\w+)\s+(.*)", stmt).groups()
            declared += [(ctype + (" *" if n.strip().startswith("*") else ""), n.strip().lstrip("*")) for n in names.split(",")]
    mirror = {"const uint8_t *": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, mirror[t]) for t, n in declared] == list(_lib.Yuv420Image._fields_)
    fields = [f for f, _ in _lib.Yuv420Image._fields_]
    assert fields == ["y_dev", "u_dev", "v_dev", "h", "w", "y_pitch_bytes", "uv_pitch_bytes", "chroma_step", "y_offset", "cy", "crv", "cgu", "cgv", "cbu"]
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("gcc is needed to check the C side")
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"vgh.h\"\nint main(void) {\n    printf(\"%zu\\n\", sizeof(vgh_yuv420_image));\n"
    prog += "".join(f"    printf(\"%zu\\n\", offsetof(vgh_yuv420_image, {f}));\n" for f in fields) + "    return 0;\n}\n"
    src = tmp_path / "yuv_layout.c"
    src.write_text(prog)
    exe = str(tmp_path / "yuv_layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.Yuv420Image)] + [getattr(_lib.Yuv420Image, f).offset for f in fields]


def test_frame_and_factory_validation():
    y, u, v = (torch.from_numpy(p) for p in yuv_ref.picture(6, 8, 1))
    ok = YUV420Frame(y, u, v, chroma_step=1)
    assert ok.shape == (6, 8, 3) and (ok.y_pitch, ok.uv_pitch) == (8, 4)
    bad = [
        lambda: YUV420Frame(y.float(), u, v, chroma_step=1),                      # dtype
        lambda: YUV420Frame(y, u.to(torch.int8), v, chroma_step=1),
        lambda: YUV420Frame(y, u, v, chroma_step=3),
        lambda: YUV420Frame(y, u, v, chroma_step=2),                              # dense planes are not interleaved views
        lambda: YUV420Frame(y, u[:2], v, chroma_step=1),                          # chroma shape
        lambda: YUV420Frame(y.t().contiguous().t(), u, v, chroma_step=1),         # luma not dense along x
        lambda: YUV420Frame(y, u, torch.zeros(3, 9, dtype=torch.uint8)[:, :4], chroma_step=1),   # two chroma pitches
        lambda: YUV420Frame(y, u, v, chroma_step=1, matrix="bt470"),
        lambda: YUV420Frame(y, u.to("meta"), v, chroma_step=1),                   # planes on two devices
    ]
    surf = torch.zeros(6 * 8 * 3 // 2, dtype=torch.uint8)
    bad += [
        lambda: YUV420Frame.from_nv12(surf, 6, 8, pitch=7),                       # pitch below the width
        lambda: YUV420Frame.from_i420(surf, 6, 9, pitch=9),                       # pitch // 2 below the chroma width
        lambda: YUV420Frame.from_nv12(surf, 6, 8, uv_offset=40),                  # inside the luma plane
        lambda: YUV420Frame.from_nv12(surf[:-1], 6, 8),                           # surface too short
        lambda: YUV420Frame.from_i420(surf, 6, 8, uv_offset=49),                  # V plane runs off the end
        lambda: YUV420Frame.from_nv21(surf.view(6, 12)[:, :8], 4, 8),             # not one contiguous buffer
        lambda: YUV420Frame.from_nv12(surf.to(torch.int16), 6, 8),
        lambda: YUV420Frame.from_nv12((y, u), 6, 8),                              # planes: (y, uv [ch, cw, 2])
        lambda: YUV420Frame.from_i420((y, u), 6, 8),
        lambda: YUV420Frame.from_nv12(surf, 0, 8),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
    assert YUV420Frame.from_nv12(surf, 6, 8).shape == YUV420Frame.from_i420(surf, 6, 8).shape == (6, 8, 3)


def test_images_arg_validation():
    """engine._images_arg without an engine behind it: a mixed list, frames on another device and an oversized batch are refused before the library is called."""
    from head_detector_amd.engine import VGHeadsEngine

    class Stub:
        max_batch, device, stream = 2, torch.device("cuda", 0), None

    y, u, v = (torch.from_numpy(p) for p in yuv_ref.picture(6, 8, 1))
    frame = YUV420Frame(y, u, v, chroma_step=1)
    rgb = frame.to_rgb()
    arg = lambda images: VGHeadsEngine._images_arg(Stub(), images)  # noqa: E731
    with pytest.raises(ValueError, match="not both"):
        arg([frame, rgb])
    with pytest.raises(ValueError, match="not both"):
        arg([rgb, frame])
    with pytest.raises(ValueError, match="frame 0: its planes are on cpu"):
        arg([frame])
    with pytest.raises(ValueError, match="outside 1..max_batch"):
        arg([frame, frame, frame])
    with pytest.raises(ValueError, match="raw image 0"):
        arg([rgb])  # an RGB image on the host is still refused as before


def test_detect_sliced_refuses_a_frame():
    from head_detector_amd.detector import HeadDetector

    y, u, v = (torch.from_numpy(p) for p in yuv_ref.picture(6, 8, 1))
    with pytest.raises(TypeError, match=r"to_rgb\(\)"):
        HeadDetector.detect_sliced(object.__new__(HeadDetector), YUV420Frame(y, u, v, chroma_step=1))
