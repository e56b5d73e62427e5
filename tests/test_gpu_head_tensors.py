"""Head tensors on the MI355X: csrc/head_tensors.hip (libvghcrop.so) through ``head_tensors``, ``head_tensors_batch`` and ``PredictionResult.get_head_tensors``,
bit for bit against the NumPy restatement of include/vgh_crop.h (tests/head_tensors_ref.py) on every planted case (tests/head_tensors_cases.py), for every dtype,
both layouts and both channel orders.  There is no tolerance anywhere in this file: float results are compared as their raw bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_tensors_cases as hc  # noqa: E402
import head_tensors_ref as ref  # noqa: E402

from head_detector_amd import _lib_crop, head_tensors as ht  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = hc.cases()
COMBOS = [(dtype, layout, order) for dtype in ("uint8", "float32", "float16", "bfloat16") for layout in ("nchw", "nhwc") for order in ("rgb", "bgr")]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _same(got: torch.Tensor, want: np.ndarray, what):
    raw = ref.raw(got)
    assert raw.dtype == want.dtype and raw.shape == want.shape, (what, raw.dtype, raw.shape, want.dtype, want.shape)
    assert torch.equal(torch.from_numpy(raw.view(np.uint8).copy()), torch.from_numpy(want.view(np.uint8).copy())), (what, int((raw != want).sum()))  # the raw patterns


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_planted_case_equals_the_restatement_bitwise(gpu_lib, name):
    c = CASES[name]
    made = [hc.on_device(source, _dev()) for source, _ in c["pairs"]]
    sources, buffers = [m[0] for m in made], [m[1] for m in made]
    expected = {order: hc.expected_sums(c, order) for order in ("rgb", "bgr")}  # computed once per order, shared by the dtypes and layouts
    plan = hc.plan_of(c)
    for dtype, layout, order in COMBOS:
        s, ks = expected[order]
        want = ref.finish(s, ks, dtype, layout, **c["norm"])
        got = hc.run(c, _dev(), dtype, layout, order, sources=sources)
        assert got.tensor.is_cuda and got.tensor.dtype == hc.DTYPES[dtype] and got.tensor.is_contiguous()
        _same(got.tensor, want, (name, dtype, layout, order))
        assert np.array_equal(got.matrices, plan[3]) and np.array_equal(got.supersample, plan[1]) and np.array_equal(got.image_index, plan[2])
    for (source, _), buffer in zip(c["pairs"], buffers):  # the sources, and the sentinel bytes around them, are what they were
        assert np.array_equal(buffer.cpu().numpy(), source["buffer"]), name


def test_a_frame_equals_its_rgb_image_bitwise(gpu_lib):
    for name in ("nv12_limited", "nv21_full", "i420_limited", "i420_full_saturating", "nv12_saturating"):
        c = CASES[name]
        frame, _ = hc.on_device(c["pairs"][0][0], _dev())
        assert isinstance(frame, YUV420Frame)
        rgb = frame.to_rgb()
        assert np.array_equal(rgb.cpu().numpy(), hc.rgb_of(c["pairs"][0][0]))
        for dtype, layout, order in (("uint8", "nhwc", "rgb"), ("float32", "nchw", "bgr"), ("bfloat16", "nchw", "rgb"), ("float16", "nhwc", "bgr")):
            a = hc.run(c, _dev(), dtype, layout, order, sources=[frame])
            b = hc.run(c, _dev(), dtype, layout, order, sources=[rgb])
            assert torch.equal(a.tensor.view(torch.uint8), b.tensor.view(torch.uint8)), (name, dtype, layout, order)
        # a result made from a frame without an RGB copy (rgb="none"): the frame is the source
        heads = c["pairs"][0][1]
        via = PredictionResult(None, heads, source_frame=frame).get_head_tensors(c["size"], aligned=False, supersample=c["supersample"], dtype=torch.uint8, layout="nhwc")
        direct = ht.head_tensors(rgb, heads, c["size"], aligned=False, supersample=c["supersample"], dtype=torch.uint8, layout="nhwc")
        assert torch.equal(via.tensor, direct.tensor)


def test_identity_crops_equal_get_aligned_heads(gpu_lib):
    """Un-rotated heads (abs(yaw) >= 60) whose rect lies inside the image: uint8 NHWC with K = 1 and S = side is the crop get_aligned_heads returns, byte for byte."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (hc.H, hc.W, 3), dtype=np.uint8)
    heads = [hc.mesh_head(60.0, 48.0, 25.0, 33.0, yaw=75.0, seed=1), hc.mesh_head(30.0, 30.0, 12.0, -120.0, yaw=-61.0, seed=2), hc.mesh_head(90.0, 60.0, 28.0, 5.0, yaw=89.0, seed=3)]
    res = PredictionResult(img, heads, head_indices=hc.HIDX)
    crops = res.get_aligned_heads()
    plan = ht.head_tensor_plan(img.shape, heads, 16, head_indices=hc.HIDX)
    checked = 0
    for k, crop in enumerate(crops):
        side = int(plan.sides[k])
        assert crop.shape == (side, side, 3) and side >= 16, (k, crop.shape, side)  # the rect lies inside the image: the slice kept all of it
        one = PredictionResult(img, [heads[k]], head_indices=hc.HIDX).get_head_tensors(side, supersample=1, dtype=torch.uint8, layout="nhwc")
        assert one.supersample.tolist() == [1] and np.array_equal(one.tensor[0].cpu().numpy(), crop), k
        assert np.array_equal(one.to_image([[0, 0], [side - 1, side - 1]], 0)[1] - one.to_image([[0, 0]], 0)[0], [side - 1, side - 1])
        checked += 1
    assert checked == 3


def test_batch_equals_the_concatenation_of_single_calls(gpu_lib):
    c = CASES["two_sources"]
    sources = [hc.on_device(source, _dev())[0] for source, _ in c["pairs"]]
    for dtype, layout, order in (("float32", "nchw", "rgb"), ("bfloat16", "nhwc", "bgr"), ("uint8", "nchw", "bgr")):
        whole = hc.run(c, _dev(), dtype, layout, order, sources=sources)
        singles = [hc.run(dict(c, pairs=[pair]), _dev(), dtype, layout, order, sources=[s]) for pair, s in zip(c["pairs"], sources)]
        assert [int(t.tensor.shape[0]) for t in singles] == [2, 0, 1, 1] and whole.tensor.shape[0] == 4
        assert torch.equal(whole.tensor.view(torch.uint8), torch.cat([t.tensor for t in singles]).view(torch.uint8))
        assert whole.image_index.tolist() == [0, 0, 2, 3] and np.array_equal(whole.matrices, np.concatenate([t.matrices for t in singles]))
        assert all(t.image_index.tolist() == [0] * len(t.image_index) for t in singles)
    empty = ht.head_tensors_batch([], 16, aligned=False)
    assert tuple(empty.tensor.shape) == (0, 3, 16, 16) and empty.tensor.is_cuda and empty.image_index.shape == (0,)


def test_out_is_written_and_nothing_around_it(gpu_lib):
    c = CASES["S17_K2_ragged"]
    for dtype, layout in (("float16", "nchw"), ("uint8", "nhwc"), ("float32", "nhwc")):
        s, ks = hc.expected_sums(c)
        want = ref.finish(s, ks, dtype, layout, **c["norm"])
        shape, n = want.shape, want.size
        whole = torch.full((n + 64,), 77, dtype=hc.DTYPES[dtype], device=_dev())
        before = whole.clone()
        out = whole[31:31 + n].view(shape)  # (an odd offset: aligned to the element, not to more)
        got = hc.run(c, _dev(), dtype, layout, out=out)
        assert got.tensor.data_ptr() == out.data_ptr()
        _same(out, want, (dtype, layout))
        assert torch.equal(whole[:31], before[:31]) and torch.equal(whole[31 + n:], before[31 + n:])
    with pytest.raises(ValueError, match="out"):
        hc.run(c, _dev(), "float32", "nchw", out=torch.zeros(2, 3, 17, 17, device=_dev()).permute(0, 1, 3, 2))
    none = ht.head_tensors(hc.on_device(c["pairs"][0][0], _dev())[0], [], 17, aligned=False, out=torch.zeros(0, 3, 17, 17, device=_dev()))
    assert tuple(none.tensor.shape) == (0, 3, 17, 17)


def test_two_calls_back_to_back_on_one_stream(gpu_lib):
    """A small call, a large one (the staging block regrows while the first call's work may still be queued) and the small one again, nothing waited for between."""
    names = ("S1_K8", "many_heads", "S1_K8")
    made = {name: [hc.on_device(source, _dev())[0] for source, _ in CASES[name]["pairs"]] for name in set(names)}
    want = {name: ref.finish(*hc.expected_sums(CASES[name]), "float32", "nchw", **CASES[name]["norm"]) for name in set(names)}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = [hc.run(CASES[name], _dev(), "float32", "nchw", sources=made[name]) for name in names]
    stream.synchronize()
    for name, g in zip(names, got):
        _same(g.tensor, want[name], name)


def test_an_invalid_job_is_refused_and_queues_nothing(gpu_lib):
    lib = _lib_crop.load()
    src = torch.zeros(8, 8, 3, dtype=torch.uint8, device=_dev())
    dst = torch.full((48,), 9, dtype=torch.uint8, device=_dev())
    source = (_lib_crop.Source * 1)()
    source[0].kind, source[0].h, source[0].w, source[0].rgb_dev, source[0].rgb_pitch_bytes = 0, 8, 8, src.data_ptr(), 24
    rows = np.zeros(1, _lib_crop.HEAD_DTYPE)
    rows["xp"], rows["yq"], rows["supersample"] = 1 << 32, 1 << 32, 1
    job = _lib_crop.Job()
    job.sources, job.heads, job.n_sources, job.n_heads, job.size, job.dtype, job.layout = _lib_crop.C.addressof(source), rows.ctypes.data, 1, 1, 4, 0, 1
    job.dst_dev, job.dst_bytes = dst.data_ptr(), 47
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.vghc_head_tensors(job, stream) == -1 and b"needs 48 bytes" in lib.vghc_last_error()  # VGHC_ERR_INVALID
    job.dst_bytes, rows["x0"] = 48, 1 << 62
    assert lib.vghc_head_tensors(job, stream) == -1 and b"reaches 2^62" in lib.vghc_last_error()
    rows["x0"], rows["supersample"] = 0, 9
    assert lib.vghc_head_tensors(job, stream) == -1 and b"supersample 9" in lib.vghc_last_error()
    torch.cuda.synchronize()
    assert (dst == 9).all()  # nothing was queued
    rows["supersample"] = 1
    assert lib.vghc_head_tensors(job, stream) == 0  # and the same job, valid, writes: the 4 x 4 corner of a black image
    torch.cuda.synchronize()
    assert (dst == 0).all()
    with pytest.raises(_lib_crop.VghError, match="libvghcrop error -1"):
        _lib_crop.check(-1)


def test_head_tensors_of_video_frames_through_the_facade(gpu_lib, flame_model):
    """detect_batch(frames, rgb="none") followed by ONE head_tensors_batch call: one batch for the next model, cut out of the frames' own planes, equal to the
    restatement driven by the same heads.  With synthetic weights the boxes are meaningless: the assertion is equality, not plausibility."""
    import yuv_ref

    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.video import yuv_coefficients

    det = HeadDetector("vgg_heads_m", 320, flame_model=flame_model, weights="synthetic", seed=4, max_batch=2)
    pictures = [yuv_ref.picture(h, w, seed) for h, w, seed in ((300, 320, 1), (275, 411, 2))]
    frames = [YUV420Frame.from_nv12(torch.from_numpy(yuv_ref.surface("nv12", *p)[0]).to(_dev()), p[0].shape[0], p[0].shape[1]) for p in pictures]
    image, _ = det._preprocess(frames[0].to_rgb().cpu().numpy())
    conf = float(det._process(image)[1][0, 6, 0])
    results = det.detect_batch(frames, confidence_threshold=conf, rgb="none")
    assert len(results) == 2 and all(r.original_image is None and r.source_frame is f for r, f in zip(results, frames)) and sum(len(r.heads) for r in results) >= 2
    got = ht.head_tensors_batch(results, 16, aligned=False, dtype=torch.float16)
    n = sum(len(r.heads) for r in results)
    assert tuple(got.tensor.shape) == (n, 3, 16, 16) and got.image_index.tolist() == [0] * len(results[0].heads) + [1] * len(results[1].heads)
    rgb = [yuv_ref.yuv_to_rgb(*p, yuv_coefficients("bt709", False)) for p in pictures]
    plans = [ht.head_tensor_plan(im.shape, r.heads, 16, aligned=False) for im, r in zip(rgb, results)]
    s = ref.sums(rgb, np.concatenate([p.coefficients for p in plans]), got.supersample, got.image_index, 16)
    _same(got.tensor, ref.finish(s, got.supersample, "float16", "nchw"), "facade")
    one = results[0].get_head_tensors(16, aligned=False, dtype=torch.float16)
    assert torch.equal(one.tensor.view(torch.int16), got.tensor[:len(results[0].heads)].view(torch.int16))
    with pytest.raises(FileNotFoundError):
        results[0].get_head_tensors(16)
