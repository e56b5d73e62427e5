"""Head anonymisation on the MI355X: csrc/anonymize.hip (libvghanon.so) against the restatement of include/vgh_anon.h (tests/anonymize_ref.py) on the planted
cases of tests/anonymize_cases.py.  Every comparison is np.array_equal / torch.equal: there is no tolerance anywhere, and no test asserts a time."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_cases as ac  # noqa: E402
import anonymize_ref as ref  # noqa: E402
from draw_fixture import fixture_heads, fixture_image, load_fixture  # noqa: E402

from head_detector_amd import _lib_anon, anonymize, visibility  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.tracking import TrackedPredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu
C = _lib_anon.C


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _api(case, image, **kw):
    return anonymize.anonymize_heads(image, case["heads"], case["method"], case["region"], margin=case["margin"], cells=case["cells"], strength=case["strength"], color=case["color"],
                                     faces=case["faces"], owner=case["owner"], **kw)


def _where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return f"{len(bad)} pixels differ, the first at (y, x) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}" if len(bad) else "equal"


def _c_call(case, src: torch.Tensor) -> np.ndarray:
    """The C call on rows made by the restatement's arithmetic (never the product's plan); ``src`` is the pitched GPU view."""
    lib = _lib_anon.load()
    boxes, cell, tables = ac.rows_of(case)
    n, (H, W) = len(boxes), src.shape[:2]
    rows = np.zeros(n, _lib_anon.HEAD_DTYPE)
    taps, at = [], 0
    for i in range(n):
        rows[i] = (*boxes[i], cell[i], len(tables[i]) - 1, at, 0)
        taps += tables[i]
        at += len(tables[i])
    taps = np.array(taps, dtype=np.int32)
    owner = None
    if case["owner"] is not None or case["region"] in ("mesh", "map"):
        owner = torch.from_numpy(np.ascontiguousarray(ac.owner_of(case, boxes))).to(src.device)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=src.device)
    color = case["color"]
    job = _lib_anon.Job(src_dev=src.data_ptr(), dst_dev=out.data_ptr(), src_pitch_bytes=src.stride(0), height=H, width=W, n_heads=n, method=_lib_anon.METHODS[case["method"]],
                        region=2 if owner is not None else {"box": 0, "ellipse": 1}[case["region"]], color=color[0] | color[1] << 8 | color[2] << 16,
                        heads=rows.ctypes.data if n else None, taps=taps.ctypes.data, n_taps=len(taps), reserved=0, owner_dev=None if owner is None else owner.data_ptr())
    need = lib.vghan_workspace_bytes(job)
    assert need >= 16 and need % 16 == 0, lib.vghan_last_error()
    workspace = torch.empty(need, dtype=torch.uint8, device=src.device)
    _lib_anon.check(lib.vghan_anonymize(job, workspace.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_every_planted_case_through_anonymize_heads(gpu_lib):
    ran = 0
    for name, case in ac.cases().items():
        if case["kind"] != "api":
            continue
        want = ac.expected(name, case)
        host = ac.view_of(case["buffer"], case["width"])
        keep = case["buffer"].copy()
        got = _api(case, host)  # a pitched NumPy view: uploaded once
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, "host image", _where(got, want))
        assert np.array_equal(case["buffer"], keep), name
        buf = torch.from_numpy(case["buffer"]).to(_dev())
        src = ac.view_of(buf, case["width"])  # a pitched GPU view that starts off a dword
        assert src.stride(0) > 3 * src.shape[1] and src.data_ptr() % 4
        got = _api(case, src)
        assert np.array_equal(got, want), (name, "device image", _where(got, want))
        assert torch.equal(buf.cpu(), torch.from_numpy(keep)), name  # the source, and the buffer around it, untouched
        ran += 1
    assert ran >= 30


def test_every_planted_case_through_the_c_call(gpu_lib):
    for name, case in ac.cases().items():
        want = ac.expected(name, case)
        buf = torch.from_numpy(case["buffer"]).to(_dev())
        got = _c_call(case, ac.view_of(buf, case["width"]))
        assert np.array_equal(got, want), (name, _where(got, want))
        assert torch.equal(buf.cpu(), torch.from_numpy(case["buffer"])), name


def test_out_device_results_and_repeated_runs(gpu_lib):
    cases = ac.cases()
    for name in ("overlap_blur_ellipse", "edges_pixelate_box", "owner_fill", "mesh_blur"):
        case = cases[name]
        want = torch.from_numpy(np.array(ac.expected(name, case)))
        buf = torch.from_numpy(case["buffer"]).to(_dev())
        src = ac.view_of(buf, case["width"])
        first = _api(case, src, to_host=False)
        assert isinstance(first, torch.Tensor) and first.is_cuda and first.dtype == torch.uint8 and first.is_contiguous() and torch.equal(first.cpu(), want), name
        out = torch.full(tuple(want.shape), 0xAB, dtype=torch.uint8, device=_dev())
        again = _api(case, src, out=out, to_host=False)
        assert again.data_ptr() == out.data_ptr() and torch.equal(out, first), name  # written in place; two runs are identical
        host = _api(case, src, out=out)
        assert isinstance(host, np.ndarray) and np.array_equal(host, want.numpy()) and torch.equal(out, first), name
        assert torch.equal(buf.cpu(), torch.from_numpy(case["buffer"])), name
        # a video loop: another image through the same out, then the first one again (the staging block and the workspace are reused)
        other = torch.flip(buf, dims=(0,)).contiguous()
        _api(case, ac.view_of(other, case["width"]), out=out, to_host=False)
        _api(case, src, out=out, to_host=False)
        assert torch.equal(out, first), name
    # out= that overlaps the source, or of another shape, dtype or place, is refused
    case = cases["one_head"]
    buf = torch.from_numpy(case["buffer"]).to(_dev())
    whole = buf[:, :ac.W]  # pitched: `out` must be dense
    dense = buf.reshape(-1)[:ac.H * ac.W * 3].view(ac.H, ac.W, 3)  # dense, but inside the source's buffer
    for bad, words in ((whole, "contiguous"), (dense, "overlaps the source"), (torch.empty((ac.H, ac.W + 1, 3), dtype=torch.uint8, device=_dev()), "contiguous GPU uint8"),
                       (torch.empty((ac.H, ac.W, 3), dtype=torch.int8, device=_dev()), "contiguous GPU uint8"), (torch.empty((ac.H, ac.W, 3), dtype=torch.uint8), "contiguous GPU uint8")):
        with pytest.raises(ValueError, match=words):
            _api(case, ac.view_of(buf, case["width"]), out=bad)
    assert torch.equal(buf.cpu(), torch.from_numpy(case["buffer"]))
    # owner= as a GPU tensor is the same as NumPy
    case = cases["owner_pixelate"]
    dev_owner = dict(case, owner=torch.from_numpy(case["owner"]).to(_dev()))
    assert np.array_equal(_api(dev_owner, ac.view_of(case["buffer"], case["width"])), ac.expected("owner_pixelate", case))


def _fixture_want(image, heads, method, region, faces=None, **kw):
    """The restatement on the draw fixture's heads with the public defaults (margin 0.1, cells 8, strength 0.1)."""
    H, W = image.shape[:2]
    if region == "mesh":
        import visibility_ref as vr

        boxes = [ref.mesh_box(h.vertices_3d, faces, H, W) for h in heads]
        owner = vr.compose(np.stack([h.vertices_3d for h in heads]), faces, H, W, "order", -1.0)["head_index"]
    else:
        boxes = [ref.geometry_box(h.bbox, 0.1) for h in heads]
        owner = ref.owner_map(H, W, boxes, region)
    return ref.render(image, boxes, owner, method, cell=[ref.cell_side(b, 8) for b in boxes], tap_tables=[ref.taps(*ref.blur_radius(b, 0.1)) for b in boxes], **kw)


def test_prediction_result_anonymize(gpu_lib):
    g = load_fixture()
    image, heads, faces = fixture_image(g, "A"), fixture_heads(g, "A"), g["triangles"]
    keep = image.copy()
    res = PredictionResult(image, heads, faces)
    default = res.anonymize()
    assert np.array_equal(default, anonymize.anonymize_heads(image, heads)) and np.array_equal(default, _fixture_want(image, heads, "pixelate", "ellipse"))
    assert not np.array_equal(default, image) and np.array_equal(image, keep)
    for method, region, kw in (("blur", "box", {}), ("fill", "ellipse", dict(color=(12, 34, 56))), ("pixelate", "mesh", {}), ("blur", "mesh", {})):
        got = res.anonymize(method, region, **kw)
        assert np.array_equal(got, anonymize.anonymize_heads(image, heads, method, region, faces=faces, **kw)), (method, region)
        want = _fixture_want(image, heads, method, region, faces, **kw)
        assert np.array_equal(got, want), (method, region, _where(got, want))
    # the mesh region is the silhouette get_visibility sees: nothing changes outside it
    vis = res.get_visibility().head_index
    got = res.anonymize("fill", "mesh", color=(1, 2, 3))
    assert np.array_equal(got[vis < 0], image[vis < 0]) and (got[vis >= 0] == (1, 2, 3)).all() and (vis >= 0).any()
    assert np.array_equal(res.anonymize("fill", "mesh", color=(1, 2, 3), faces=faces[:50]), anonymize.anonymize_heads(image, heads, "fill", "mesh", color=(1, 2, 3), faces=faces[:50]))
    # a tracked result, coasting tracks included, with the frame on the device (rgb="device")
    frame = torch.from_numpy(image).to(_dev())
    n = len(heads)
    tracked = TrackedPredictionResult(frame, heads, faces, track_ids=np.arange(n, dtype=np.int64), hits=np.full(n, 3, np.int64), coasting=np.arange(n) % 2 == 1)
    on_dev = tracked.anonymize(to_host=False)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and torch.equal(on_dev.cpu(), torch.from_numpy(default)) and torch.equal(frame.cpu(), torch.from_numpy(keep))
    assert np.array_equal(tracked.anonymize("blur", "mesh"), res.anonymize("blur", "mesh"))
    assert np.array_equal(PredictionResult(image, []).anonymize(), image) and np.array_equal(PredictionResult(image, [], faces).anonymize("blur", "mesh"), image)
