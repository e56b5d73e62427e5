"""The on-screen display on the MI355X: csrc/osd.hip (libvghosd.so) against the restatement of include/vgh_osd.h (tests/osd_ref.py) on the planted cases of
tests/osd_cases.py, in every layout, in place and out of place, with a workspace full of garbage.  Every comparison of bytes is np.array_equal / torch.equal over
WHOLE surfaces, sentinels included: there is no tolerance, and no test asserts a time."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import osd_cases as oc  # noqa: E402
import osd_ref as ref  # noqa: E402
import yuv_ref  # noqa: E402

from head_detector_amd import _vgho, overlay, video  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

pytestmark = pytest.mark.gpu

GARBAGE = (0x7F7F7F7F, -1)  # int32 views of 0x7f7f7f7f and 0xffffffff
OTHER = {"nv12": "i420", "nv21": "nv12", "i420": "nv21", "rgb": "rgb"}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _c_call(case, src_buf, src_geom, dst_buf, dst_geom, garbage):
    """The C call on rows made by tests/osd_cases.py (never the product's ``Items``), with a workspace that holds ``garbage`` in every word."""
    lib = _vgho.load()
    h, w = case["shape"]
    rows, codes = oc.c_arrays(case["items"], _vgho.ITEM_DTYPE)
    job = _vgho.Job()
    for k, (s, d) in enumerate(zip(src_geom["planes"], dst_geom["planes"])):
        p = job.planes[k]
        p.src_dev, p.dst_dev = src_buf.data_ptr() + s["offset"], dst_buf.data_ptr() + d["offset"]
        p.src_pitch, p.dst_pitch, p.src_step, p.dst_step, p.shift = s["pitch"], d["pitch"], s["step"], d["step"], s["shift"]
    job.height, job.width, job.n_planes, job.n_items = h, w, 3, len(rows)
    if len(rows):
        job.items = rows.ctypes.data
    if len(codes):
        job.codes, job.n_codes = codes.ctypes.data, len(codes)
    need = lib.vgho_workspace_bytes(job)
    assert need >= 16 and need % 16 == 0 and need >= 4 * h * w, lib.vgho_last_error()
    workspace = torch.full((need // 4,), garbage, dtype=torch.int32, device=src_buf.device)
    _vgho.check(lib.vgho_draw(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _first(a, b):
    bad = np.flatnonzero(a != b)
    return f"{len(bad)} bytes differ, the first at {int(bad[0])}: got {a[bad[0]]}, want {b[bad[0]]}" if len(bad) else "equal"


def test_every_planted_case_in_every_layout_in_place_and_out_of_place(gpu_lib):
    ran = 0
    for name, case in oc.cases().items():
        shape, seed = case["shape"], case["seed"]
        K = ref.key_plane(*shape, case["items"])
        for layout in oc.LAYOUTS:
            src, want = oc.expected(name, case, layout)
            for pitched in (True, False):
                host, geom = oc.surface(shape, layout, pitched, src, seed)
                want_surface = oc.surface(shape, layout, pitched, want, seed)[0]  # the same sentinels around the restatement's planes
                owned = np.zeros(geom["size"], dtype=bool)  # the bytes of the samples somebody owns
                for view, s in zip(oc.views(owned, geom), oc.shifts(layout)):
                    view[...] = ref.owner(K, s) >= 0
                for garbage in GARBAGE:  # in place: the whole surface, every sentinel and every sample nobody owns, whatever the workspace held
                    buf = torch.from_numpy(host).to(_dev())
                    _c_call(case, buf, geom, buf, geom, garbage)
                    after = buf.cpu().numpy()
                    assert np.array_equal(after, want_surface), (name, layout, pitched, hex(garbage & 0xFFFFFFFF), "in place", _first(after, want_surface))
                    assert not (after != host)[~owned].any(), (name, layout, pitched, "a byte outside the owned samples changed")
                if not case["items"]:
                    assert np.array_equal(after, host), (name, layout, pitched, "n_items = 0 in place changed the buffer")
                # out of place into another surface full of other sentinels: a pitched source goes to another layout, a dense one to its own layout, pitched
                dl, dp = (OTHER[layout], False) if pitched else (layout, True)
                blank, dgeom = oc.surface(shape, dl, dp, [np.zeros_like(p) for p in want], seed + 50)
                want_out = oc.surface(shape, dl, dp, want, seed + 50)[0]
                buf, out = torch.from_numpy(host).to(_dev()), torch.from_numpy(blank).to(_dev())
                _c_call(case, buf, geom, out, dgeom, GARBAGE[ran % 2])
                got = out.cpu().numpy()
                assert np.array_equal(got, want_out), (name, layout, pitched, "->", dl, dp, _first(got, want_out))
                assert np.array_equal(buf.cpu().numpy(), host), (name, layout, pitched, "the source surface changed")
                ran += 1
    assert ran == len(oc.cases()) * 4 * 2 and ran >= 100


def _items_of(ref_items, colour_of):
    """The product's builder from the restatement's items; ``colour_of`` maps an item's plane bytes to the RGB triple to give."""
    items = overlay.Items()
    for it in ref_items:
        a = it["alpha"] / 256.0
        if it["kind"] == "bar":
            items.bar(it["box"], colour_of(it["color"]), a)
        elif it["kind"] == "rect":
            items.rect(it["box"], colour_of(it["color"]), it["thickness"], a)
        else:
            items.text(it["box"][0], it["box"][1], "".join(ref.CHARS[c] for c in it["codes"]), colour_of(it["color"]), it["scale"], a)
    return items


def _yuv_items(ref_items, matrix, full_range):
    return [dict(it, color=video.rgb_to_yuv(it["color"], matrix, full_range)) for it in ref_items]


def test_render_frames_and_images_through_the_python_surface(gpu_lib):
    cases = oc.cases()
    for name, layout, matrix, full in (("stack", "nv12", "bt709", False), ("text", "nv21", "bt601", True), ("odd", "i420", "bt2020", False), ("many_heads", "nv12", "bt709", True),
                                      ("tiny_1x1", "i420", "bt709", False), ("no_items", "nv21", "bt709", False)):
        case = cases[name]
        h, w = case["shape"]
        y, u, v = yuv_ref.picture(h, w, case["seed"])
        pitch = 2 * ((w + 1) // 2) + 10
        surface, pitch, uv_offset = yuv_ref.surface(layout, y, u, v, pitch=pitch, extra_rows=3)
        buf = torch.from_numpy(surface).to(_dev())
        make = {"nv12": YUV420Frame.from_nv12, "nv21": YUV420Frame.from_nv21, "i420": YUV420Frame.from_i420}[layout]
        frame = make(buf, h, w, pitch=pitch, uv_offset=uv_offset, matrix=matrix, full_range=full)
        items = _items_of(case["items"], lambda c: c)  # the case's bytes as RGB: the frame converts them
        want = ref.render([y, u, v], (0, 1, 1), h, w, _yuv_items(case["items"], matrix, full))
        got = overlay.render(frame, items)  # out=None: a new dense frame of the source's layout, matrix and range
        assert isinstance(got, YUV420Frame) and got is not frame and (got.chroma_step, got.matrix, got.full_range, got.shape) == (frame.chroma_step, matrix, full, frame.shape), name
        assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(got.planes, want)), name
        assert np.array_equal(buf.cpu().numpy(), surface), (name, "the source surface changed")
        again = overlay.render(frame, items)  # two identical calls give identical bytes
        assert all(torch.equal(p, q) for p, q in zip(got.planes, again.planes)), name
        for other in ("nv12", "i420"):  # another layout out (NV12 in, I420 out among them)
            out = YUV420Frame.empty(h, w, other, _dev(), matrix=matrix, full_range=full)
            assert overlay.render(frame, items, out=out) is out and all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(out.planes, want)), (name, other)
        assert overlay.render(frame, items, out=frame) is frame  # in place, on the decoder's surface
        assert np.array_equal(buf.cpu().numpy(), yuv_ref.surface(layout, *want, pitch=pitch, extra_rows=3)[0]), (name, "in place")
        shifted = YUV420Frame(frame.y, frame.v, frame.u, chroma_step=frame.chroma_step)  # the source's memory, but not plane for plane
        for bad, words in ((YUV420Frame.empty(h, w + 1, "nv12", _dev()), "out must be a YUV420Frame"), ("frame", "out must be a YUV420Frame")) + (((shifted, "overlaps the source frame"),) if h > 2 else ()):
            with pytest.raises(ValueError, match=words):
                overlay.render(frame, items, out=bad)
    # RGB: a NumPy image (uploaded, a GPU tensor comes back), a pitched GPU view, out= and in place
    for name in ("edges", "text", "many_heads"):
        case = cases[name]
        h, w = case["shape"]
        src, want = oc.expected(name, case, "rgb")
        image, want_image = np.stack(src, axis=-1), np.stack(want, axis=-1)
        items = _items_of(case["items"], lambda c: c)
        got = overlay.render(image, items)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want_image), name
        wide = np.random.default_rng(1).integers(0, 256, (h, w + 7, 3), dtype=np.uint8)
        wide[:, 3:3 + w] = image
        dev_wide = torch.from_numpy(wide).to(_dev())
        view = dev_wide[:, 3:3 + w]
        got = overlay.render(view, items)
        assert got.data_ptr() != view.data_ptr() and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want_image) and np.array_equal(dev_wide.cpu().numpy(), wide), name
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device=_dev())
        assert overlay.render(view, items, out=out) is out and np.array_equal(out.cpu().numpy(), want_image), name
        assert overlay.render(view, items, out=view) is view  # in place in the pitched view: the bytes beside it stay
        wide[:, 3:3 + w] = want_image
        assert np.array_equal(dev_wide.cpu().numpy(), wide), name
        with pytest.raises(ValueError, match="overlaps"):
            overlay.render(view, items, out=dev_wide[:, 2:2 + w])


def test_rgb_and_luma_agree_on_ownership(gpu_lib):
    """An RGB image whose three channels are the Y plane, drawn with grey items (c, c, c), and the full-range frame drawn with the same items: a grey's Y byte is
    c itself, so the set of changed positions is the same in the image and in the luma plane."""
    cases = oc.cases()
    for name in ("stack", "text", "edges", "odd"):
        case = cases[name]
        h, w = case["shape"]
        y, u, v = yuv_ref.picture(h, w, case["seed"] + 9)
        items = _items_of(case["items"], lambda c: (c[0], c[0], c[0]))
        assert all(video.rgb_to_yuv((c, c, c), "bt709", True) == (c, 128, 128) for c in (0, 1, 127, 200, 255))
        frame = YUV420Frame.from_i420((torch.from_numpy(y).to(_dev()), torch.from_numpy(u).to(_dev()), torch.from_numpy(v).to(_dev())), h, w, matrix="bt709", full_range=True)
        luma = overlay.render(frame, items).y.cpu().numpy()
        image = overlay.render(np.stack([y, y, y], axis=-1), items).cpu().numpy()
        assert np.array_equal(image[..., 0], luma) and np.array_equal(image[..., 1], luma) and np.array_equal(image[..., 2], luma), name
        assert np.array_equal((image != y[..., None]).any(axis=-1), luma != y) and (luma != y).any(), name


def test_draw_overlay_on_a_detectors_and_a_trackers_result(gpu_lib, flame_model):
    """A detector with synthetic weights on one NV12 frame with ``rgb="none"``: the overlay is drawn into the frame's own planes, equals the restatement applied to
    ``head_overlay_plan``'s items, and a tracked head's label carries its track id."""
    import warnings

    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.tracking import HeadTracker, TrackedPredictionResult

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

    def restated(plan):
        rows, codes = plan.rows(), plan.codes()
        items = []
        for r in rows:
            box, c, a = (int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])), video.rgb_to_yuv(tuple(int(x) for x in r["color"]), "bt709", False), int(r["alpha"])
            if r["kind"] == _vgho.BAR:
                items.append(ref.bar(box, c, a))
            elif r["kind"] == _vgho.RECT:
                items.append(ref.rect(box, c, int(r["thickness"]), a))
            else:
                items.append(ref.text(box[0], box[1], codes[r["code_offset"]:r["code_offset"] + r["length"]].tolist(), c, int(r["scale"]), a))
        return ref.render([y, u, v], (0, 1, 1), h, w, items)

    res = det(frame, confidence_threshold=conf, rgb="none")
    assert res.original_image is None and res.source_frame is frame and len(res.heads) >= 1
    got = res.draw_overlay(labels="id+score", text_scale=1)
    want = restated(overlay.head_overlay_plan((h, w), res.heads, labels="id+score", text_scale=1))
    assert got is not frame and all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(got.planes, want)) and not np.array_equal(want[0], y)
    assert np.array_equal(buf.cpu().numpy(), surface)
    host = res.draw_overlay(labels="id+score", text_scale=1, to_host=True)
    assert all(isinstance(p, np.ndarray) and np.array_equal(p, q) for p, q in zip(host, want))
    # a result with an RGB original_image draws into that
    with_rgb = det(frame, confidence_threshold=conf)
    drawn = with_rgb.draw_overlay(labels="score", colors=(255, 0, 0))  # (the frame is the target where there is one)
    assert isinstance(drawn, YUV420Frame)
    rgb_only = det(with_rgb.original_image, confidence_threshold=conf)
    picture = rgb_only.draw_overlay(labels="score", colors=(255, 0, 0), to_host=True)
    plan = overlay.head_overlay_plan((h, w), rgb_only.heads, labels="score", colors=(255, 0, 0))
    rows, codes = plan.rows(), plan.codes()
    items = [ref.rect(tuple(int(r[k]) for k in ("x0", "y0", "x1", "y1")), tuple(r["color"]), int(r["thickness"]), int(r["alpha"])) if r["kind"] == _vgho.RECT else
             ref.bar(tuple(int(r[k]) for k in ("x0", "y0", "x1", "y1")), tuple(r["color"]), int(r["alpha"])) if r["kind"] == _vgho.BAR else
             ref.text(int(r["x0"]), int(r["y0"]), codes[r["code_offset"]:r["code_offset"] + r["length"]].tolist(), tuple(r["color"]), int(r["scale"]), int(r["alpha"])) for r in rows]
    src = [np.ascontiguousarray(with_rgb.original_image[..., c]) for c in range(3)]
    assert isinstance(picture, np.ndarray) and np.array_equal(picture, np.stack(ref.render(src, (0, 0, 0), h, w, items), axis=-1))
    # the tracker: ids and coasting come from the result itself, in place on the decoder's surface
    tracker = HeadTracker(det, max_tracks=64, high_thr=conf, low_thr=low, min_hits=1)
    tracker.update(frame, rgb="none")
    tr = tracker.update(frame, rgb="none")
    assert isinstance(tr, TrackedPredictionResult) and tr.original_image is None and len(tr.heads) >= 1
    plan = overlay.head_overlay_plan((h, w), tr.heads, labels="id", track_ids=tr.track_ids, coasting=tr.coasting)
    labels = [r for r in plan.rows() if r["kind"] == _vgho.TEXT]
    texts = ["".join(overlay.CHARS[c] for c in plan.codes()[r["code_offset"]:r["code_offset"] + r["length"]]) for r in labels]
    assert texts == [f"#{int(i)}" for i in tr.track_ids]
    want = restated(plan)
    assert tr.draw_overlay(labels="id", out=frame) is frame
    assert np.array_equal(buf.cpu().numpy(), yuv_ref.surface("nv12", *want, pitch=pitch, extra_rows=3)[0])


def test_a_chroma_pair_at_an_odd_address_on_one_side_and_an_even_one_on_the_other(gpu_lib):
    """5 x 7 (both sides odd), one item of each kind, through the C call.  The interleaved chroma plane of one surface starts at an odd byte, so its (U, V) views are
    not the bytes of an aligned 16-bit pair and go byte by byte, while the other surface's are one 16-bit access: a pair on the source side alone, then on the
    destination side alone, NV12 and NV21 (the lower byte is U, then V), and the odd surface in place.  Whole surfaces, sentinels included."""
    h, w, pitch = 5, 7, 10
    items = [ref.bar((0, 0, 4, 3), (200, 40, 90), 128), ref.rect((2, 1, 7, 5), (13, 250, 7), 1, 256), ref.text(1, -1, [2], (90, 91, 230), 1, 200)]
    case = dict(shape=(h, w), items=items)
    src = oc.content((h, w), "nv12", 31)
    want = ref.render(src, (0, 1, 1), h, w, items)
    assert not np.array_equal(want[1], src[1]) and not np.array_equal(want[2], src[2]) and want[1].shape == (3, 4)

    def surface(planes, uv, v_first, seed):
        first = [dict(offset=uv + k, pitch=pitch, step=2, shift=1, h=3, w=4) for k in range(2)]
        geom = dict(size=uv + pitch * 3 + 8, planes=[dict(offset=0, pitch=pitch, step=1, shift=0, h=h, w=w)] + (first[::-1] if v_first else first))
        buffer = np.random.default_rng(seed).integers(0, 256, geom["size"], dtype=np.uint8)
        for view, plane in zip(oc.views(buffer, geom), planes):
            view[...] = plane
        return buffer, geom

    for v_first in (False, True):
        for src_uv, dst_uv in ((pitch * h + 1, pitch * h), (pitch * h, pitch * h + 1)):
            host, geom = surface(src, src_uv, v_first, 5)
            blank, dgeom = surface([np.zeros_like(p) for p in want], dst_uv, v_first, 6)
            buf, out = torch.from_numpy(host).to(_dev()), torch.from_numpy(blank).to(_dev())
            assert buf.data_ptr() % 2 == 0 and out.data_ptr() % 2 == 0  # so the parity of a plane's offset is the parity of its address
            _c_call(case, buf, geom, out, dgeom, GARBAGE[0])
            got, want_out = out.cpu().numpy(), surface(want, dst_uv, v_first, 6)[0]
            assert np.array_equal(got, want_out), (v_first, src_uv, dst_uv, _first(got, want_out))
            assert np.array_equal(buf.cpu().numpy(), host), (v_first, src_uv, dst_uv, "the source surface changed")
        host, geom = surface(src, pitch * h + 1, v_first, 5)  # in place at the odd address: bytes on both sides
        buf = torch.from_numpy(host).to(_dev())
        _c_call(case, buf, geom, buf, geom, GARBAGE[1])
        after, want_surface = buf.cpu().numpy(), surface(want, pitch * h + 1, v_first, 5)[0]
        assert np.array_equal(after, want_surface), (v_first, "in place", _first(after, want_surface))
