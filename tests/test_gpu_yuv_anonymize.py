"""Head anonymisation in YUV 4:2:0 planes and the RGB packer on the MI355X: csrc/yuv_anonymize.hip and csrc/yuv_pack.hip (libvghvideo.so) against the
restatement of include/vgh_video.h (tests/yuv_anonymize_ref.py) on the planted cases of tests/yuv_anonymize_cases.py.  Every comparison of bytes is
np.array_equal / torch.equal: there is no tolerance but the round trip's stated bound, and no test asserts a time."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import yuv_anonymize_cases as yc  # noqa: E402
import yuv_anonymize_ref as yref  # noqa: E402
import yuv_ref  # noqa: E402

from head_detector_amd import _lib_video, anonymize, video  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.tracking import TrackedPredictionResult  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _api(case, frame, **kw):
    return video.anonymize_frame(frame, case["heads"], case["method"], case["region"], margin=case["margin"], cells=case["cells"], strength=case["strength"], color=case["color"],
                                 faces=case["faces"], owner=case["owner"], **kw)


def _planes(frame):
    return tuple(p.cpu().numpy() for p in frame.planes)


def _where(got, want):
    for name, g, w in zip("YUV", got, want):
        bad = np.argwhere(g != w)
        if len(bad):
            at = tuple(bad[0])
            return f"plane {name}: {len(bad)} samples differ, the first at (y, x) = {at}: got {g[at]}, want {w[at]}"
    return "equal"


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _rows(boxes, cell, tables, taps, at):
    rows = np.zeros(len(boxes), _lib_video.HEAD_DTYPE)
    for i in range(len(boxes)):
        rows[i] = (*boxes[i], cell[i], len(tables[i]) - 1, at, 0)
        taps += tables[i]
        at += len(tables[i])
    return rows, at


def _c_call(case, src: YUV420Frame, dst: YUV420Frame):
    """The C call on rows made by the restatement's arithmetic (never the product's plan)."""
    lib = _lib_video.load()
    r = yc.rows_of(case)
    n, (H, W) = len(r["luma_boxes"]), case["shape"]
    taps = []
    luma, at = _rows(r["luma_boxes"], r["luma_cell"], r["luma_taps"], taps, 0)
    chroma, at = _rows(r["chroma_boxes"], r["chroma_cell"], r["chroma_taps"], taps, at)
    taps = np.array(taps, dtype=np.int32)
    owner = None
    if case["owner"] is not None or case["region"] in ("mesh", "map"):
        owner = torch.from_numpy(np.ascontiguousarray(yc.owner_of(case, r["luma_boxes"]))).to(src.device)
    job = _lib_video.AnonymizeJob()
    for k, ((s, sp, ss), (d, dp, ds)) in enumerate(zip(src._layout(), dst._layout())):
        p = job.planes[k]
        p.src_dev, p.dst_dev, p.src_pitch, p.dst_pitch, p.src_step, p.dst_step = s.data_ptr(), d.data_ptr(), sp, dp, ss, ds
    c = r["color_yuv"]
    job.height, job.width, job.n_heads, job.method, job.color = H, W, n, _lib_video.METHODS[case["method"]], c[0] | c[1] << 8 | c[2] << 16
    job.region = 2 if owner is not None else {"box": 0, "ellipse": 1}[case["region"]]
    if n:
        job.luma_heads, job.chroma_heads = luma.ctypes.data, chroma.ctypes.data
    job.taps, job.n_taps = taps.ctypes.data, len(taps)
    if owner is not None:
        job.owner_dev = owner.data_ptr()
    need = lib.vghy_anonymize_workspace_bytes(job)
    assert need >= 16 and need % 16 == 0, lib.vghy_last_error()
    workspace = torch.empty(need, dtype=torch.uint8, device=src.device)
    _lib_video.check(lib.vghy_anonymize(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _surface(case, planes=None, layout=None):
    """(host bytes, GPU copy) of the case's surface holding ``planes`` in ``layout``."""
    host = yc.surface_of(case, planes, layout)[0]
    return host, torch.from_numpy(host).to(_dev())


def test_every_planted_case_through_anonymize_frame_out_of_place_and_in_place(gpu_lib):
    ran = 0
    for name, case in yc.cases().items():
        if case["kind"] != "api":
            continue
        want = yc.expected(name, case)
        host, buf = _surface(case)
        src = yc.frame_of(case, buf)
        got = _api(case, src)  # out=None: a new dense frame of the source's layout, matrix and range
        assert isinstance(got, YUV420Frame) and (got.chroma_step, got.matrix, got.full_range, got.shape) == (src.chroma_step, src.matrix, src.full_range, src.shape), name
        assert (got.v.data_ptr() > got.u.data_ptr()) == (src.v.data_ptr() > src.u.data_ptr()), name  # NV12 stays NV12, NV21 stays NV21
        assert _same(_planes(got), want), (name, "out of place", _where(_planes(got), want))
        assert np.array_equal(buf.cpu().numpy(), host), (name, "the source surface changed")
        # in place: the whole surface equals a surface that holds the restatement's planes -- every sentinel byte and every sample nobody owns is unchanged
        back = _api(case, src, out=src)
        assert back is src, name
        want_surface = yc.surface_of(case, want)[0]
        after = buf.cpu().numpy()
        assert np.array_equal(after, want_surface), (name, "in place", int((after != want_surface).sum()), "bytes differ, the first at", int(np.argmax(after != want_surface)))
        assert _same(_planes(src), _planes(got)), name  # in place = out of place
        ran += 1
    assert ran >= 35


def test_every_planted_case_through_the_c_call(gpu_lib):
    for name, case in yc.cases().items():
        want = yc.expected(name, case)
        host, buf = _surface(case)
        src = yc.frame_of(case, buf)
        # out of place into a PITCHED surface full of another seed's sentinels: every sample is written, nothing else
        other = dict(case, seed=case["seed"] + 50, pitched=True)
        blank = yc.surface_of(other, tuple(np.zeros_like(p) for p in want))[0]
        out_buf = torch.from_numpy(blank).to(_dev())
        dst = yc.frame_of(other, out_buf)
        _c_call(case, src, dst)
        assert _same(_planes(dst), want), (name, _where(_planes(dst), want))
        assert np.array_equal(out_buf.cpu().numpy(), yc.surface_of(other, want)[0]), (name, "bytes outside the destination's samples were written")
        assert np.array_equal(buf.cpu().numpy(), host), (name, "the source surface changed")
        _c_call(case, src, src)  # in place
        assert np.array_equal(buf.cpu().numpy(), yc.surface_of(case, want)[0]), (name, "in place")


def test_luma_plane_equals_libvghanon_on_the_stacked_plane(gpu_lib):
    """An independent cross-check: another library, other kernels.  The luma plane of the result is channel 0 of ``anonymize_heads`` on stack([Y, Y, Y])."""
    ran = 0
    for name, case in yc.cases().items():
        if case["kind"] != "api" or case["region"] == "mesh" or case["method"] == "fill":
            continue
        _, buf = _surface(case)
        src = yc.frame_of(case, buf)
        got = _api(case, src)
        stacked = torch.stack([src.y, src.y, src.y], dim=-1).contiguous()
        rgb = anonymize.anonymize_heads(stacked, case["heads"], case["method"], case["region"], margin=case["margin"], cells=case["cells"], strength=case["strength"], owner=case["owner"])
        assert np.array_equal(got.y.cpu().numpy(), rgb[..., 0]) and np.array_equal(rgb[..., 0], rgb[..., 2]), name
        ran += 1
    assert ran >= 20
    # fill: the colour's Y byte
    case = yc.cases()["edges_fill_ellipse"]
    _, buf = _surface(case)
    src = yc.frame_of(case, buf)
    yy = video.rgb_to_yuv(case["color"], src.matrix, src.full_range)[0]
    stacked = torch.stack([src.y, src.y, src.y], dim=-1).contiguous()
    rgb = anonymize.anonymize_heads(stacked, case["heads"], "fill", "ellipse", color=(yy, yy, yy))
    assert np.array_equal(_api(case, src).y.cpu().numpy(), rgb[..., 0])


def test_layout_change_repeated_runs_and_refused_outputs(gpu_lib):
    cases = yc.cases()
    for name in ("edges_blur_box", "overlap_pixelate_ellipse", "owner_fill", "many_heads_blur"):
        case = cases[name]
        want = yc.expected(name, case)
        host, buf = _surface(case)
        src = yc.frame_of(case, buf)
        for layout in yc.LAYOUTS:  # source layout -> every destination layout (NV12 -> I420 among them): the same planes
            out = YUV420Frame.empty(*case["shape"], layout, _dev(), matrix=src.matrix, full_range=src.full_range)
            back = _api(case, src, out=out)
            assert back is out and _same(_planes(out), want), (name, layout, _where(_planes(out), want))
            first = tuple(p.clone() for p in out.planes)
            _api(case, yc.frame_of(case, torch.flip(buf, dims=(0,)).contiguous()), out=out)  # a video loop: another frame through the same out, then the first again
            _api(case, src, out=out)
            assert all(torch.equal(a, b) for a, b in zip(first, out.planes)), (name, layout, "two runs differ")
        assert np.array_equal(buf.cpu().numpy(), host), name
    case = cases["edges_pixelate_box"]
    _, buf = _surface(case)
    src = yc.frame_of(case, buf)
    h, w = case["shape"]
    shifted = YUV420Frame(src.y, src.v, src.u, chroma_step=src.chroma_step)  # the source's memory, but not plane for plane
    for bad, words in ((YUV420Frame.empty(h, w + 1, "nv12", _dev()), "out must be a YUV420Frame"), ("frame", "out must be a YUV420Frame"), (shifted, "overlaps the source frame")):
        with pytest.raises(ValueError, match=words):
            _api(case, src, out=bad)
    same_memory = yc.frame_of(case, buf)  # another object over the same planes counts as in place
    assert _api(case, src, out=same_memory) is same_memory and _same(_planes(src), yc.expected("edges_pixelate_box", case))


def test_from_rgb_equals_the_restatement(gpu_lib):
    rng = np.random.default_rng(5)
    for (h, w), layout, matrix, full in (((97, 131), "nv12", "bt709", False), ((96, 130), "nv21", "bt601", True), ((1, 1), "i420", "bt2020", False), ((2, 2), "nv12", "bt709", True),
                                         ((1, 7), "i420", "bt601", False), ((64, 64), "nv21", "bt2020", True), ((5, 3), "i420", "bt709", False)):
        wide = rng.integers(0, 256, (h, w + 19, 3), dtype=np.uint8)
        if (h, w) == (96, 130):
            wide = ((rng.integers(0, 2, wide.shape)) * 255).astype(np.uint8)  # saturating
        image = wide[:, 7:7 + w]  # a pitched view that starts off a dword
        want = yref.pack(image, yref.coefficients(matrix, full))
        for source in (image, torch.from_numpy(wide).to(_dev())[:, 7:7 + w]):
            got = YUV420Frame.from_rgb(source, layout, matrix, full)
            assert (got.matrix, got.full_range, got.shape, got.chroma_step) == (matrix, full, (h, w, 3), 1 if layout == "i420" else 2)
            assert _same(_planes(got), want), ((h, w), layout, _where(_planes(got), want))
        # out=: a pitched surface of sentinels; its own layout, matrix and range are used and nothing outside the samples is written
        case = dict(shape=(h, w), pitched=True, layout=layout, seed=h + w, content="random", matrix=matrix, full_range=full)
        blank = yc.surface_of(case, tuple(np.zeros_like(p) for p in want))[0]
        buf = torch.from_numpy(blank).to(_dev())
        out = yc.frame_of(case, buf)
        assert YUV420Frame.from_rgb(image, "i420", "bt709", not full, out=out) is out
        assert np.array_equal(buf.cpu().numpy(), yc.surface_of(case, want)[0]), ((h, w), layout)
    # the round trip of an image of constant 2 x 2 blocks: within 2 (limited range) or 1 (full range) of the image in every channel
    blocks = rng.integers(0, 256, (24, 33, 3), dtype=np.uint8)
    blocks[:4, :8] = [[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]] * 4
    image = np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)[:47, :65]
    for matrix in ("bt601", "bt709", "bt2020"):
        for full, bound in ((False, 2), (True, 1)):
            back = YUV420Frame.from_rgb(image, "nv12", matrix, full).to_rgb().cpu().numpy()
            worst = int(np.abs(back.astype(np.int32) - image.astype(np.int32)).max())
            assert worst <= bound, (matrix, full, worst)


def _planted_result(case, frame, cls=PredictionResult, **kw):
    return cls(None, case["heads"], case.get("faces"), source_frame=frame, **kw)


def test_prediction_result_anonymize_frame(gpu_lib):
    cases = yc.cases()
    case = cases["overlap_pixelate_ellipse"]
    want = yc.expected("overlap_pixelate_ellipse", case)
    _, buf = _surface(case)
    frame = yc.frame_of(case, buf)
    res = _planted_result(case, frame)
    kw = dict(margin=case["margin"], cells=case["cells"], strength=case["strength"], color=case["color"])
    got = res.anonymize_frame(case["method"], case["region"], **kw)
    assert got is not frame and _same(_planes(got), want)
    n = len(case["heads"])
    tracked = _planted_result(case, frame, TrackedPredictionResult, track_ids=np.arange(n, dtype=np.int64), hits=np.full(n, 3, np.int64), coasting=np.arange(n) % 2 == 1)
    assert tracked.anonymize_frame(case["method"], case["region"], out=frame, **kw) is frame and _same(_planes(frame), want)  # coasting tracks included, in place
    mesh = cases["mesh_pixelate"]
    _, mbuf = _surface(mesh)
    got = _planted_result(mesh, yc.frame_of(mesh, mbuf)).anonymize_frame("pixelate", "mesh", cells=mesh["cells"])  # the result's own faces
    assert _same(_planes(got), yc.expected("mesh_pixelate", mesh))
    with pytest.raises(ValueError, match=r"anonymize\(\)"):
        PredictionResult(np.zeros((4, 4, 3), np.uint8), []).anonymize_frame()


def test_detector_and_tracker_remember_the_frame_without_an_rgb_copy(gpu_lib, flame_model):
    """A detector with synthetic weights on one NV12 frame: ``rgb="none"`` makes no RGB copy, the result keeps the frame, and the frame route still works."""
    import warnings

    import anonymize_ref as ref

    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.tracking import HeadTracker

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        det = HeadDetector("vgg_heads_m", image_size=160, weights="synthetic", flame_model=flame_model, max_batch=2, seed=4)
    h, w = 90, 120
    y, u, v = yuv_ref.picture(h, w, 60)
    surface, pitch, uv_offset = yuv_ref.surface("nv12", y, u, v, pitch=2 * ((w + 1) // 2) + 10, extra_rows=3)
    buf = torch.from_numpy(surface).to(_dev())
    frame = YUV420Frame.from_nv12(buf, h, w, pitch=pitch, uv_offset=uv_offset)
    scores = det.model.model([frame])[1][0, :, 0]
    conf, low = float(scores[3]), float(scores[12])
    with_rgb = det(frame, confidence_threshold=conf)
    assert with_rgb.source_frame is frame and isinstance(with_rgb.original_image, np.ndarray) and len(with_rgb.heads) >= 1
    res = det(frame, confidence_threshold=conf, rgb="none")
    assert res.original_image is None and res.source_frame is frame
    assert [tuple(hd.bbox) for hd in res.heads] == [tuple(hd.bbox) for hd in with_rgb.heads]
    batch = det.detect_batch([frame, frame], confidence_threshold=conf, rgb="none")
    assert all(r.original_image is None and r.source_frame is frame and len(r.heads) == len(res.heads) for r in batch)
    assert det(with_rgb.original_image, confidence_threshold=conf).source_frame is None  # an RGB input has no frame
    with pytest.raises(ValueError, match="YUV420Frame inputs only"):
        det(with_rgb.original_image, rgb="none")
    # the frame route on the detector's own heads, against the restatement
    boxes = [ref.geometry_box(hd.bbox, 0.1) for hd in res.heads]
    out = res.anonymize_frame("fill", "box", color=(255, 255, 255))
    want = yref.render_frame(y, u, v, boxes, ref.owner_map(h, w, boxes, "box"), "fill", color_yuv=yref.pixel_yuv((255, 255, 255), yref.coefficients("bt709", False)))
    assert _same(_planes(out), want), _where(_planes(out), want)
    assert np.array_equal(buf.cpu().numpy(), surface)
    tracker = HeadTracker(det, max_tracks=64, high_thr=conf, low_thr=low, min_hits=1)
    tr = tracker.update(frame, rgb="none")
    assert tr.original_image is None and tr.source_frame is frame and len(tr.heads) >= 1
    boxes = [ref.geometry_box(hd.bbox, 0.1) for hd in tr.heads]
    assert tr.anonymize_frame("fill", "box", color=(0, 0, 0), out=frame) is frame  # in place, on the decoder's surface
    want = yref.render_frame(y, u, v, boxes, ref.owner_map(h, w, boxes, "box"), "fill", color_yuv=(16, 128, 128))
    assert np.array_equal(buf.cpu().numpy(), yuv_ref.surface("nv12", *want, pitch=pitch, extra_rows=3)[0])
    assert tracker.update_batch([frame], rgb="host")[0].source_frame is frame


def test_a_chroma_pair_at_an_odd_address_on_one_side_and_an_even_one_on_the_other(gpu_lib):
    """5 x 7 (both sides odd), two heads, hand-made rows through the C call.  The interleaved chroma plane of one surface starts at an odd byte, so its (U, V)
    views are not the bytes of an aligned 16-bit pair and go byte by byte, while the other surface's are one 16-bit access: a pair on the source side alone, then
    on the destination side alone, NV12 and NV21 (the lower byte is U, then V), pixelate (the cell sums load) and blur (the row pass loads); every pass stores.
    Whole surfaces, sentinels included."""
    h, w, pitch = 5, 7, 10
    boxes = dict(luma_boxes=[(0, 0, 4, 3), (3, 1, 7, 5)], chroma_boxes=[(0, 0, 2, 2), (1, 0, 4, 3)])
    runs = {"pixelate": yc.raw_case((h, w), boxes["luma_boxes"], boxes["chroma_boxes"], "pixelate", "box", "nv12", luma_cell=[2, 3], chroma_cell=[2, 3], seed=21),
            "blur": yc.raw_case((h, w), boxes["luma_boxes"], boxes["chroma_boxes"], "blur", "box", "nv12", luma_taps=[[32768, 16384], [65536]], chroma_taps=[[21846, 21845], [32768, 8192, 8192]],
                                seed=21)}

    def surface(planes, uv_offset, seed):
        """(bytes, frame maker): sentinel bytes everywhere, the planes planted through CPU views of the layout."""
        host = np.random.default_rng(seed).integers(0, 256, uv_offset + pitch * 3 + 8, dtype=np.uint8)

        def frame(buffer):
            return make(buffer, h, w, pitch=pitch, uv_offset=uv_offset)

        for view, plane in zip(frame(torch.from_numpy(host)).planes, planes):
            view.copy_(torch.from_numpy(np.array(plane)))  # (a copy: the expected planes are read-only)
        return host, frame

    for method, case in runs.items():
        want = yc.expected(f"odd_pair_5x7_{method}", case)
        planes = yc.planes_of(case)
        assert not np.array_equal(want[1], planes[1]) and not np.array_equal(want[2], planes[2]) and want[1].shape == (3, 4), method
        for make in (YUV420Frame.from_nv12, YUV420Frame.from_nv21):
            for src_uv, dst_uv in ((pitch * h + 1, pitch * h), (pitch * h, pitch * h + 1)):
                host, src_frame = surface(planes, src_uv, 5)
                blank, dst_frame = surface(tuple(np.zeros_like(p) for p in want), dst_uv, 6)
                buf, out = torch.from_numpy(host).to(_dev()), torch.from_numpy(blank).to(_dev())
                src, dst = src_frame(buf), dst_frame(out)
                assert min(src.u.data_ptr(), src.v.data_ptr()) % 2 == src_uv % 2 and min(dst.u.data_ptr(), dst.v.data_ptr()) % 2 == dst_uv % 2
                _c_call(case, src, dst)
                assert _same(_planes(dst), want), (method, make.__name__, src_uv, dst_uv, _where(_planes(dst), want))
                assert np.array_equal(out.cpu().numpy(), surface(want, dst_uv, 6)[0]), (method, make.__name__, src_uv, dst_uv, "bytes outside the destination's samples were written")
                assert np.array_equal(buf.cpu().numpy(), host), (method, make.__name__, src_uv, dst_uv, "the source surface changed")
