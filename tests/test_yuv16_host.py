"""CPU: the host side of VGH_IMG_YUV420P16_RAW (10- and 12-bit P010 / I010 video frames converted inside the device letterbox) -- the conversion rule of
include/vgh.h restated twice in NumPy (tests/yuv16_ref.py) and once in torch (video.YUV420Frame16.to_rgb), its tie to the pinned 8-bit rule, the coefficient
integers, the int32 bound, the C ABI additions and their ctypes mirror, the bridge to 8-bit frames, and the errors the class, the factories and the engine's image
argument raise.  Everything is byte equality."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import yuv16_ref
import yuv_ref
from conftest import ROOT
from head_detector_amd import _lib
from head_detector_amd.video import YUV420Frame, YUV420Frame16, yuv_coefficients

MATRICES = ("bt601", "bt709", "bt2020")
# hand-computed: limited range = the 8-bit integers (2^(D+8) * 255 / (219 * 2^(D-8)) = 65536 * 255 / 219); full range: 2^18 * 255 / 1023 = 65344.25 -> 65344,
# 2^20 * 255 / 4095 = 65296.0 (to 0.0002) -> 65296, and the chroma rows likewise
COEFFICIENTS = {
    ("bt709", False, 10): (64, 76309, 117489, -13975, -34925, 138438),
    ("bt709", False, 12): (256, 76309, 117489, -13975, -34925, 138438),
    ("bt601", False, 10): (64, 76309, 104597, -25675, -53279, 132201),
    ("bt2020", False, 12): (256, 76309, 110014, -12277, -42626, 140363),
    ("bt709", True, 10): (0, 65344, 102903, -12240, -30589, 121252),
    ("bt709", True, 12): (0, 65296, 102828, -12232, -30567, 121163),
}
SIZES = [(1, 1), (3, 5), (2, 2), (6, 4), (7, 9)]  # (h, w): odd sizes use the ceil chroma column / row


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vgh.h")).read(), flags=re.S)


def test_header_declares_format_4_within_abi_8():
    code = _code()
    assert re.search(r"#define\s+VGH_IMG_YUV420P16_RAW\s+4\b", code)
    assert re.search(r"typedef\s+struct\s+vgh_yuv420p16_image\s*\{[^}]*\}\s*vgh_yuv420p16_image\s*;", code)
    assert re.search(r"#define\s+VGH_ABI_VERSION\s+8\b", code)
    assert "unknown image format 4" in open(os.path.join(ROOT, "include", "vgh.h")).read()
    assert _lib.VGH_IMG_YUV420P16_RAW == 4 and _lib.RAW_FORMATS == (2, 3) and _lib.DESCRIPTOR_FORMATS == (2, 3, 4)
    assert _lib.ABI_VERSION == 8 == _lib.load().vgh_abi_version()
    assert len(_lib.SYMBOLS) == 86


def test_ctypes_yuv420p16_image_matches_the_c_layout(tmp_path):
    m = re.search(r"typedef\s+struct\s+vgh_yuv420p16_image\s*\{([^}]*)\}", _code())
    declared = []  # (c type, name) in order, from the header's text
    for stmt in m.group(1).split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = re.match(r"((?:const\s+)?\w+)\s+(.*)", stmt).groups()
            declared += [(ctype + (" *" if n.strip().startswith("*") else ""), n.strip().lstrip("*")) for n in names.split(",")]
    mirror = {"const uint16_t *": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, mirror[t]) for t, n in declared] == list(_lib.Yuv420P16Image._fields_)
    fields = [f for f, _ in _lib.Yuv420P16Image._fields_]
    assert fields == ["y_dev", "u_dev", "v_dev", "h", "w", "y_pitch_bytes", "uv_pitch_bytes", "chroma_step", "bit_depth", "shift", "y_offset", "cy", "crv", "cgu", "cgv",
                      "cbu"]
    cc = shutil.which("gcc")
    if cc is None:
        pytest.fail("gcc is needed to check the C side")
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"vgh.h\"\nint main(void) {\n    printf(\"%zu\\n\", sizeof(vgh_yuv420p16_image));\n"
    prog += "".join(f"    printf(\"%zu\\n\", offsetof(vgh_yuv420p16_image, {f}));\n" for f in fields) + "    return 0;\n}\n"
    src = tmp_path / "yuv16_layout.c"
    src.write_text(prog)
    exe = str(tmp_path / "yuv16_layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.Yuv420P16Image)] + [getattr(_lib.Yuv420P16Image, f).offset for f in fields]


def test_coefficient_integers():
    assert {k: yuv_coefficients(*k) for k in COEFFICIENTS} == COEFFICIENTS
    for matrix, full, D in itertools.product(MATRICES, (False, True), (10, 12)):
        coef = yuv_coefficients(matrix, full, D)
        assert coef == yuv16_ref.coefficients(matrix, full, D)
        assert 0 <= coef[0] < 1 << D and 0 <= coef[1] <= 1 << 17 and all(abs(c) <= 1 << 18 for c in coef[2:])  # what the library admits
        if not full:  # limited range: the 8-bit integers, the offset scaled
            eight = yuv_coefficients(matrix, False)
            assert coef[1:] == eight[1:] and coef[0] == eight[0] << (D - 8)
    assert yuv_coefficients("bt709", False, 8) == yuv_coefficients("bt709", False) == (16, 76309, 117489, -13975, -34925, 138438)  # the default is unchanged
    for bad in (9, 16, 0):
        with pytest.raises(ValueError, match="bit_depth"):
            yuv_coefficients("bt709", False, bad)


@pytest.mark.parametrize("D", [10, 12])
def test_limited_range_rule_on_shifted_samples_is_the_8_bit_rule(D):
    """The tie to the pinned rule: on sample8 << (D - 8), limited range, the deep restatement gives the bytes of yuv_ref.yuv_to_rgb on the 8-bit samples."""
    for (h, w), matrix, saturating in zip(SIZES + [(33, 20)], MATRICES * 2, (False, True) * 3):
        y, u, v = yuv_ref.picture(h, w, 10 * h + w, saturating)
        want = yuv_ref.yuv_to_rgb(y, u, v, yuv_coefficients(matrix, False))
        deep = [p.astype(np.uint16) << np.uint16(D - 8) for p in (y, u, v)]
        coef = yuv16_ref.coefficients(matrix, False, D)
        assert np.array_equal(yuv16_ref.yuv16_to_rgb(*deep, coef, D, 0), want)
        msb = [p << np.uint16(16 - D) for p in deep]  # the same samples MSB-aligned
        assert np.array_equal(yuv16_ref.yuv16_to_rgb(*msb, coef, D, 16 - D), want)
        if h * w <= 64:
            assert np.array_equal(yuv16_ref.yuv16_to_rgb_loop(*deep, coef, D, 0), want)


@pytest.mark.parametrize("D", [10, 12])
def test_full_range_grey_ramp(D):
    """Neutral chroma, every luma code: black -> 0, white -> 255, monotone, R = G = B."""
    top = (1 << D) - 1
    y = np.arange(top + 1, dtype=np.uint16).reshape(2, -1)
    c = np.full((1, y.shape[1] // 2), 1 << (D - 1), dtype=np.uint16)
    for matrix in MATRICES:
        ref = yuv16_ref.yuv16_to_rgb(y, c, c, yuv16_ref.coefficients(matrix, True, D), D, 0).reshape(-1, 3)
        got = YUV420Frame16(torch.from_numpy(y.view(np.int16)), torch.from_numpy(c.view(np.int16)), torch.from_numpy(c.view(np.int16)), chroma_step=1, bit_depth=D,
                            matrix=matrix, full_range=True).to_rgb().reshape(-1, 3).numpy()
        assert np.array_equal(got, ref)
        assert (ref[0] == 0).all() and (ref[top] == 255).all()
        assert (np.diff(ref[:, 0].astype(int)) >= 0).all() and set(np.diff(ref[:, 0].astype(int))) <= {0, 1}
        assert (ref[:, 0] == ref[:, 1]).all() and (ref[:, 0] == ref[:, 2]).all()
        lim = yuv16_ref.yuv16_to_rgb(y, c, c, yuv16_ref.coefficients(matrix, False, D), D, 0).reshape(-1, 3)
        k = 1 << (D - 8)
        assert (lim[:16 * k + 1] == 0).all() and (lim[235 * k:] == 255).all() and (np.diff(lim[:, 0].astype(int)) >= 0).all()


def test_int32_bound_at_every_extreme_corner():
    """The header's bound: with the coefficients at their limits (cy = 2^17, |chroma| = 2^18, either sign) and y_offset at either end, every extreme (Y, U, V) at
    both depths keeps every sum inside int32 -- in Python integers, and the loop restatement (which asserts it per pixel) agrees with the int32 vectorised one."""
    worst = 0
    for D in (10, 12):
        top = (1 << D) - 1
        for y_offset, Y, U, V in itertools.product((0, top), (0, top), (0, top), (0, top)):
            for signs in itertools.product((1, -1), repeat=4):
                cy, (crv, cgu, cgv, cbu) = 1 << 17, (s << 18 for s in signs)
                c, d, e = Y - y_offset, U - (1 << (D - 1)), V - (1 << (D - 1))
                rnd = 1 << (D + 7)
                sums = (cy * c + crv * e + rnd, cy * c + cgu * d + cgv * e + rnd, cy * c + cbu * d + rnd)
                worst = max(worst, *(abs(s) for s in sums))
                assert all(-(1 << 31) <= s < (1 << 31) for s in sums), (D, y_offset, Y, U, V, signs)
    assert worst < 3 * (1 << 29) + (1 << 19) < 1 << 31
    for D in (10, 12):
        y, u, v = yuv16_ref.picture16(4, 6, 5, D, saturating=True, shift=16 - D)
        for sign in (1, -1):
            big = ((1 << D) - 1 if sign < 0 else 0, 1 << 17, sign << 18, sign << 18, sign << 18, -sign << 18)
            assert np.array_equal(yuv16_ref.yuv16_to_rgb_loop(y, u, v, big, D, 16 - D), yuv16_ref.yuv16_to_rgb(y, u, v, big, D, 16 - D))


def _views(buf, layout, h, w, pitch, off):
    """NumPy word views (y, u, v) of a surface16 buffer."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    words = buf[:buf.size & ~1].view("<u2")
    st = np.lib.stride_tricks.as_strided
    y = st(words, (h, w), (pitch, 2))
    if layout == "i010":
        cp = pitch // 2
        return y, st(words[off // 2:], (ch, cw), (cp, 2)), st(words[off // 2 + (cp // 2) * ch:], (ch, cw), (cp, 2))
    return y, st(words[off // 2:], (ch, cw), (pitch, 4)), st(words[off // 2 + 1:], (ch, cw), (pitch, 4))


@pytest.mark.parametrize("saturating", [False, True])
@pytest.mark.parametrize("D", [10, 12])
def test_frame_to_rgb_equals_the_restatement(D, saturating):
    """YUV420Frame16.to_rgb() on CPU tensors == tests/yuv16_ref.py: odd sizes, both layouts (dense, and pitched with an aligned chroma offset), both depths, both
    ranges, three matrices; the garbage in a word's unused bits does not change a byte; the factories build views, not copies."""
    combos = list(itertools.product(MATRICES, (False, True)))
    for n, (h, w) in enumerate(SIZES + [(33, 20)]):
        matrix, full = combos[n]
        coef = yuv16_ref.coefficients(matrix, full, D)
        kw = dict(matrix=matrix, full_range=full, bit_depth=D)
        for layout, make, shift in (("p010", YUV420Frame16.from_p010, 16 - D), ("i010", YUV420Frame16.from_i010, 0)):
            y, u, v = yuv16_ref.picture16(h, w, 7 * h + w, D, saturating, shift)
            want = yuv16_ref.yuv16_to_rgb(y, u, v, coef, D, shift)
            keep = np.uint16(((1 << D) - 1) << shift)
            assert np.array_equal(yuv16_ref.yuv16_to_rgb(y & keep, u & keep, v & keep, coef, D, shift), want)  # garbage bits: not a byte changes
            if h * w <= 64:
                assert np.array_equal(yuv16_ref.yuv16_to_rgb_loop(y, u, v, coef, D, shift), want)
            ch, cw = u.shape
            frames = []
            buf, pitch, off = yuv16_ref.surface16(layout, y, u, v)  # the default pitch and offset, a byte buffer
            assert all(np.array_equal(a, b) for a, b in zip(_views(buf, layout, h, w, pitch, off), (y, u, v)))
            t = torch.from_numpy(buf)
            f = make(t, h, w, **kw)
            assert f.y.data_ptr() == t.data_ptr() and f.chroma_step == (2 if layout == "p010" else 1) and f.shift == shift and f.bit_depth == D  # a view
            frames.append(f)
            buf, pitch, off = yuv16_ref.surface16(layout, y, u, v, pitch=4 * cw + 12, extra_rows=5)  # pitched, as int16 words
            t = torch.from_numpy(buf[:buf.size & ~1].view(np.int16))
            f = make(t, h, w, pitch=pitch, uv_offset=off, **kw)
            assert f.u.data_ptr() - t.data_ptr() == off and (2 * f.y_pitch, 2 * f.uv_pitch) == (pitch, pitch if layout == "p010" else pitch // 2)
            frames.append(f)
            i16 = lambda p: torch.from_numpy(np.ascontiguousarray(p).view(np.int16))  # noqa: E731
            if layout == "p010":
                frames.append(make((i16(y), i16(np.stack([u, v], axis=-1))), h, w, **kw))
            else:
                frames.append(make((i16(y), i16(u), i16(v)), h, w, **kw))
                frames.append(YUV420Frame16(i16(y), i16(u), i16(v), chroma_step=1, shift=0, **kw))
            if hasattr(torch, "uint16"):
                frames.append(YUV420Frame16(*(torch.from_numpy(np.ascontiguousarray(p)) for p in (y, u, v)), chroma_step=1, shift=shift, **kw))
            for f in frames:
                assert f.shape == (h, w, 3) and f.coefficients == coef and f.device.type == "cpu"
                got = f.to_rgb()
                assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (h, w, f)


@pytest.mark.parametrize("D", [10, 12])
def test_to_8bit_returns_the_8_bit_planes_of_shifted_samples(D):
    for (h, w), layout in zip(SIZES + [(33, 20)], ("p010", "i010") * 3):
        y, u, v = yuv_ref.picture(h, w, 3 * h + w)
        shift = 16 - D if layout == "p010" else 0
        deep = [(p.astype(np.uint16) << np.uint16(D - 8 + shift)) for p in (y, u, v)]
        buf, pitch, off = yuv16_ref.surface16(layout, *deep, pitch=4 * u.shape[1] + 8, extra_rows=1)
        make = YUV420Frame16.from_p010 if layout == "p010" else YUV420Frame16.from_i010
        f = make(torch.from_numpy(buf), h, w, pitch=pitch, uv_offset=off, bit_depth=D, matrix="bt601")
        e = f.to_8bit()
        assert isinstance(e, YUV420Frame) and e.chroma_step == (2 if layout == "p010" else 1) and (e.matrix, e.full_range) == ("bt601", False)
        for got, want in zip(e.planes, (y, u, v)):
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
        assert torch.equal(e.to_rgb(), f.to_rgb())  # limited range, exact multiples: the same picture
        other = f.to_8bit("i420")
        assert other.chroma_step == 1 and torch.equal(other.u, e.u)
        assert f.to_8bit(out=other) is other
        with pytest.raises(ValueError, match="layout"):
            f.to_8bit("p010")
        with pytest.raises(ValueError, match="out"):
            f.to_8bit(out=YUV420Frame.empty(h + 1, w, "nv12", "cpu"))
    # rounding and the cap: s -> min(255, (s + 2^(D-9)) >> (D-8))
    s = np.arange(1 << D, dtype=np.uint16).reshape(2, -1)
    c = np.zeros((1, s.shape[1] // 2), dtype=np.uint16)
    f = YUV420Frame16(*(torch.from_numpy(p.view(np.int16)) for p in (s, c, c)), chroma_step=1, bit_depth=D, full_range=True)
    want = np.minimum(255, (s.astype(np.int64) + (1 << (D - 9))) >> (D - 8))
    assert np.array_equal(f.to_8bit().y.numpy(), want) and want.max() == 255 and want[0, 1 << (D - 9)] == 1


def test_frame_and_factory_validation():
    words = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16))  # noqa: E731
    y, u, v = (words(p) for p in yuv16_ref.picture16(6, 8, 1, 10))
    ok = YUV420Frame16(y, u, v, chroma_step=1)
    assert ok.shape == (6, 8, 3) and (ok.y_pitch, ok.uv_pitch, ok.bit_depth, ok.shift) == (8, 4, 10, 0) and "10 bits" in repr(ok)
    assert ok.planes[0] is y
    bad = [
        lambda: YUV420Frame16(y.float(), u, v, chroma_step=1),                       # dtype
        lambda: YUV420Frame16(y.to(torch.uint8), u, v, chroma_step=1),
        lambda: YUV420Frame16(y, u.to(torch.int32), v, chroma_step=1),
        lambda: YUV420Frame16(y.numpy().astype(np.uint8), u, v, chroma_step=1),
        lambda: YUV420Frame16(y, u, v, chroma_step=3),
        lambda: YUV420Frame16(y, u, v, chroma_step=2),                               # dense planes are not interleaved views
        lambda: YUV420Frame16(y, u, v, chroma_step=1, bit_depth=8),
        lambda: YUV420Frame16(y, u, v, chroma_step=1, bit_depth=16),
        lambda: YUV420Frame16(y, u, v, chroma_step=1, bit_depth=10, shift=7),
        lambda: YUV420Frame16(y, u, v, chroma_step=1, bit_depth=12, shift=5),
        lambda: YUV420Frame16(y, u, v, chroma_step=1, shift=-1),
        lambda: YUV420Frame16(y, u[:2], v, chroma_step=1),                           # chroma shape
        lambda: YUV420Frame16(y.t().contiguous().t(), u, v, chroma_step=1),          # luma not dense along x
        lambda: YUV420Frame16(y, u, torch.zeros(3, 9, dtype=torch.int16)[:, :4], chroma_step=1),   # two chroma pitches
        lambda: YUV420Frame16(y, u, v, chroma_step=1, matrix="bt470"),
        lambda: YUV420Frame16(y, u.to("meta"), v, chroma_step=1),                    # planes on two devices
    ]
    surf = torch.zeros(6 * 8 * 3, dtype=torch.uint8)  # 6 x 8 words of luma + 3 x 8 of chroma
    bad += [
        lambda: YUV420Frame16.from_p010(surf, 6, 8, pitch=14),                       # pitch below the row
        lambda: YUV420Frame16.from_p010(surf, 6, 8, pitch=17),                       # odd pitch
        lambda: YUV420Frame16.from_i010(surf, 6, 8, pitch=18),                       # chroma rows would be odd
        lambda: YUV420Frame16.from_p010(surf, 6, 8, uv_offset=80),                   # inside the luma plane
        lambda: YUV420Frame16.from_p010(surf, 6, 8, uv_offset=97),                   # odd offset
        lambda: YUV420Frame16.from_p010(surf[:-2], 6, 8),                            # surface too short
        lambda: YUV420Frame16.from_p010(surf[1:], 6, 7),                             # odd address
        lambda: YUV420Frame16.from_i010(surf, 6, 8, uv_offset=98),                   # V plane runs off the end
        lambda: YUV420Frame16.from_p010(surf.view(6, 24)[:, :16], 4, 8),             # not one contiguous buffer
        lambda: YUV420Frame16.from_p010(surf.to(torch.int32), 6, 8),
        lambda: YUV420Frame16.from_p010((y, u), 6, 8),                               # planes: (y, uv [ch, cw, 2])
        lambda: YUV420Frame16.from_i010((y, u), 6, 8),
        lambda: YUV420Frame16.from_p010(surf, 0, 8),
        lambda: YUV420Frame16.from_p010(surf, 6, 8, bit_depth=8),
        lambda: YUV420Frame16.from_i010(surf, 6, 8, bit_depth=14),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
    assert YUV420Frame16.from_p010(surf, 6, 8).shape == YUV420Frame16.from_i010(surf, 6, 8).shape == (6, 8, 3)
    assert YUV420Frame16.from_p010(surf, 6, 8, bit_depth=12).shift == 4 and YUV420Frame16.from_i010(surf, 6, 8, bit_depth=12).shift == 0
    # the 8-bit class keeps refusing 16-bit planes, and a deep frame is not one of its instances
    with pytest.raises(ValueError):
        YUV420Frame(y, u, v, chroma_step=1)
    with pytest.raises(ValueError):
        YUV420Frame.from_nv12(surf.view(torch.int16), 6, 8)
    assert not isinstance(ok, YUV420Frame)


def test_images_arg_validation():
    """engine._images_arg without an engine behind it: lists mixing the three kinds, frames on another device and an oversized batch are refused before the library
    is called."""
    from head_detector_amd.engine import VGHeadsEngine

    class Stub:
        max_batch, device, stream = 3, torch.device("cuda", 0), None

    words = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16))  # noqa: E731
    deep = YUV420Frame16(*(words(p) for p in yuv16_ref.picture16(6, 8, 1, 10)), chroma_step=1)
    eight = YUV420Frame(*(torch.from_numpy(p) for p in yuv_ref.picture(6, 8, 1)), chroma_step=1)
    rgb = deep.to_rgb()
    arg = lambda images: VGHeadsEngine._images_arg(Stub(), images)  # noqa: E731
    for mixed in ([deep, rgb], [rgb, deep], [deep, eight], [eight, deep], [deep, eight, rgb]):
        with pytest.raises(ValueError, match="not both") as err:
            arg(mixed)
        assert "YUV420Frames, YUV420Frame16s or RGB tensors" in str(err.value)
    with pytest.raises(ValueError, match="frame 0: its planes are on cpu"):
        arg([deep])
    with pytest.raises(ValueError, match="outside 1..max_batch"):
        arg([deep] * 4)


def test_results_of_deep_frames_refuse_the_8_bit_consumers_and_detect_sliced_refuses_a_frame():
    from head_detector_amd.detection_result import PredictionResult
    from head_detector_amd.detector import HeadDetector

    words = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16))  # noqa: E731
    deep = YUV420Frame16(*(words(p) for p in yuv16_ref.picture16(6, 8, 1, 12)), chroma_step=1, bit_depth=12)
    with pytest.raises(TypeError, match=r"to_rgb\(\)"):
        HeadDetector.detect_sliced(object.__new__(HeadDetector), deep)
    result = PredictionResult(original_image=None, heads=[], source_frame=deep)
    for call in (result.anonymize_frame, result.draw_overlay, result.get_head_tensors):
        with pytest.raises(ValueError, match=r"source_frame\.to_8bit\(\)"):
            call()
    assert "(6, 8, 3)" in repr(result)
