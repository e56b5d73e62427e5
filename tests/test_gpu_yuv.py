"""GPU (-m gpu): VGH_IMG_YUV420_RAW -- NV12 / NV21 / I420 video frames converted to RGB inside the batched device letterbox -- against what defines it: the
conversion rule of include/vgh.h restated in NumPy (tests/yuv_ref.py), then VGH_IMG_U8_RAW on those RGB arrays.  Everything is compared byte for byte."""
import ctypes as C
import os
import struct
import subprocess
import warnings

import numpy as np
import pytest
import torch

import yuv_ref
from head_detector_amd import _lib
from head_detector_amd.letterbox import geometry
from head_detector_amd.video import YUV420Frame, yuv_coefficients

pytestmark = pytest.mark.gpu

S = 160
FACTORY = {"nv12": YUV420Frame.from_nv12, "nv21": YUV420Frame.from_nv21, "i420": YUV420Frame.from_i420}
# every layout in both ranges and with two matrices each way round: 12 frames of one picture = 3 batches of 4
COMBOS = [(layout, matrix, full) for layout in ("nv12", "nv21", "i420") for matrix, full in (("bt709", False), ("bt601", True), ("bt601", False), ("bt2020", True))]


def _dev():
    return torch.device("cuda", 0)


def _frame(layout, h, w, seed, saturating=False, matrix="bt709", full_range=False, pitched=True):
    """-> (YUV420Frame on the GPU: views of ONE uploaded surface with pitched luma and chroma rows and an aligned chroma offset; its RGB restatement, NumPy)."""
    y, u, v = yuv_ref.picture(h, w, seed, saturating)
    cw = u.shape[1]
    buf, pitch, off = yuv_ref.surface(layout, y, u, v, pitch=2 * cw + 10, extra_rows=3) if pitched else yuv_ref.surface(layout, y, u, v)
    frame = FACTORY[layout](torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, matrix=matrix, full_range=full_range)
    return frame, yuv_ref.yuv_to_rgb(y, u, v, yuv_coefficients(matrix, full_range))


def _same(a, b):
    assert torch.equal(a.counts, b.counts)
    assert a.num_heads == b.num_heads
    for f in ("boxes", "scores", "flame_params", "head_image", "vertices_3d", "head_pose"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


@pytest.fixture(scope="module")
def engine_m(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine

    eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=4, seed=11)
    yield eng
    eng.close()


def _canvas_after(eng, images):
    eng.forward_candidates(images)
    eng.join()
    torch.cuda.synchronize()
    return eng.raw_canvas()[: len(images)].clone(), eng.raw_unpad()[: len(images)].clone()


# (h, w): every tap replicated; odd in both axes (the ceil chroma column and row); downscale; tall with the pad on x; scale 1
@pytest.mark.parametrize("h,w", [(2, 2), (1, 1), (47, 61), (360, 640), (250, 33), (160, 160)])
def test_yuv_canvas_equals_raw_canvas_of_the_restated_rgb(engine_m, h, w):
    eng = engine_m
    assert eng.arena_batch >= 4
    for saturating in (False, True):
        for at in range(0, len(COMBOS), 4):
            frames, rgbs = [], []
            for layout, matrix, full in COMBOS[at:at + 4]:
                f, rgb = _frame(layout, h, w, seed=1000 * h + w, saturating=saturating, matrix=matrix, full_range=full)
                assert f.y_pitch > w and f.uv_pitch > f.chroma_step * ((w + 1) // 2)
                assert torch.equal(f.to_rgb().cpu(), torch.from_numpy(rgb))  # to_rgb on the device is the same rule
                frames.append(f)
                rgbs.append(rgb)
            want, want_unpad = _canvas_after(eng, [torch.from_numpy(r).to(_dev()) for r in rgbs])
            got, got_unpad = _canvas_after(eng, frames)
            for i, combo in enumerate(COMBOS[at:at + 4]):
                assert torch.equal(got[i], want[i]), (combo, saturating, int((got[i] != want[i]).sum()))
            assert torch.equal(got_unpad, want_unpad)
            nh, nw, gx, gy, gs = geometry(h, w, S)
            assert torch.equal(got_unpad[0].cpu(), torch.tensor([gx, gy, gs], dtype=torch.float32))
    # the three layouts of one picture with one matrix: one canvas
    trio = [_frame(layout, h, w, seed=5, pitched=False)[0] for layout in ("nv12", "nv21", "i420")]
    got, _ = _canvas_after(eng, trio)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


def _mixed(seed):
    """A batch of frames of different sizes and layouts -> (frames, their RGB restatements as GPU tensors)."""
    spec = [("nv12", 90, 120, "bt709", False), ("i420", 201, 77, "bt601", True), ("nv21", 47, 61, "bt2020", False), ("nv12", 360, 640, "bt601", False)]
    pairs = [_frame(layout, h, w, seed + i, matrix=m, full_range=fr) for i, (layout, h, w, m, fr) in enumerate(spec)]
    return [f for f, _ in pairs], [torch.from_numpy(r).to(_dev()) for _, r in pairs]


def test_yuv_detect_equals_raw_detect_of_the_restated_rgb(gpu_lib, flame_model):
    """Every detection output -- boxes, scores, parameters, counts, head list, vertices, head pose, the un-pad table -- of vgh_detect(VGH_IMG_YUV420_RAW) equals
    that of vgh_detect(VGH_IMG_U8_RAW) on the restated RGB images: a mixed-size batch in one arena chunk and in two (arena_batch 2 for 4 frames), B = 1, overlap
    mode on and off, and the two formats alternating on one engine (they share the staging slots)."""
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    frames, rgbs = _mixed(seed=40)
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=len(frames) * 100)
    for arena in (None, 2):
        eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=len(frames), seed=7, arena_batch=arena)
        try:
            assert (eng.arena_batch < len(frames)) == (arena is not None)
            _, sc, _ = eng.model(rgbs)
            conf = float(sc[:, 4, 0].min())
            for overlap in (False, True):
                eng.set_overlap(overlap)
                for n in (len(frames), 1):
                    old = eng.detect(rgbs[:n], confidence_threshold=conf, flame=fl)
                    unpad_old = eng.raw_unpad()[:n].clone()
                    new = eng.detect(frames[:n], confidence_threshold=conf, flame=fl)
                    torch.cuda.synchronize()
                    assert old.num_heads >= n
                    _same(new, old)
                    assert torch.equal(eng.raw_unpad()[:n], unpad_old)
            eng.set_overlap(False)
        finally:
            eng.close()


def test_yuv_descriptors_are_validated_before_anything_runs(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine

    eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=4, seed=2)
    try:
        det = eng._det
        scratch = lambda which: gpu_lib.vgh_detector_scratch(det, which)  # noqa: E731
        assert not scratch(_lib.SCRATCH_CANVAS) and not scratch(_lib.SCRATCH_UNPAD)
        frame, rgb = _frame("nv12", 60, 80, seed=3)
        coef = yuv_coefficients()

        def desc(**over):
            d = dict(y_dev=frame.y.data_ptr(), u_dev=frame.u.data_ptr(), v_dev=frame.v.data_ptr(), h=60, w=80, y_pitch_bytes=frame.y_pitch, uv_pitch_bytes=frame.uv_pitch,
                     chroma_step=2, y_offset=coef[0], cy=coef[1], crv=coef[2], cgu=coef[3], cgv=coef[4], cbu=coef[5])
            d.update(over)
            return _lib.Yuv420Image(**d)

        def call(*descs):
            arr = (_lib.Yuv420Image * len(descs))(*descs)
            rc = gpu_lib.vgh_detector_candidates(det, C.addressof(arr), _lib.VGH_IMG_YUV420_RAW, len(descs), eng._sp())
            return rc, gpu_lib.vgh_last_error().decode()

        ok = desc()
        cases = [((ok, desc(y_dev=None)), 1, "null plane"), ((desc(u_dev=None), ok), 0, "null plane"), ((ok, ok, desc(v_dev=None)), 2, "null plane"),
                 ((ok, desc(y_pitch_bytes=79)), 1, "y_pitch_bytes"), ((desc(uv_pitch_bytes=79),), 0, "uv_pitch_bytes"),
                 ((desc(chroma_step=1, uv_pitch_bytes=39),), 0, "uv_pitch_bytes"), ((desc(w=81, y_pitch_bytes=81, uv_pitch_bytes=81),), 0, "uv_pitch_bytes"),
                 ((ok, desc(chroma_step=0)), 1, "chroma_step"), ((ok, ok, ok, desc(chroma_step=3)), 3, "chroma_step"),
                 ((desc(y_offset=-1),), 0, "y_offset"), ((ok, desc(y_offset=256)), 1, "y_offset"),
                 ((desc(cy=(1 << 20) + 1),), 0, "coefficient cy"), ((ok, desc(cgv=-(1 << 20) - 1)), 1, "coefficient cgv"), ((desc(cbu=1 << 30),), 0, "coefficient cbu"),
                 ((desc(h=0),), 0, "empty"),
                 ((ok, desc(h=1, w=4000, y_pitch_bytes=4000, uv_pitch_bytes=4000)), 1, "elongated")]
        for descs, index, words in cases:
            rc, msg = call(*descs)
            assert rc == -1 and f"image {index}" in msg and words in msg, msg  # VGH_ERR_INVALID
        assert not scratch(_lib.SCRATCH_CANVAS)  # a rejected call allocates nothing
        for entry in (gpu_lib.vgh_net_forward, gpu_lib.vgh_net_capture):
            rc = entry(eng._net, frame.y.data_ptr(), _lib.VGH_IMG_YUV420_RAW, 1, eng._sp())
            assert rc == -1 and b"not a canvas" in gpu_lib.vgh_last_error()
        op_ms = (C.c_float * len(eng.program.ops))()
        rc = gpu_lib.vgh_net_profile(eng._net, frame.y.data_ptr(), _lib.VGH_IMG_YUV420_RAW, 1, eng._sp(), op_ms)
        assert rc == -1 and b"not a canvas" in gpu_lib.vgh_last_error()
        with pytest.raises(ValueError, match="not both"):
            eng.detect([frame, torch.from_numpy(rgb).to(_dev())])
        # the largest admissible coefficients are accepted, and a following valid call works
        rc, msg = call(desc(cy=1 << 20, crv=-(1 << 20), cgu=1 << 20, cgv=1 << 20, cbu=-(1 << 20), y_offset=255))
        assert rc == 0, msg
        rc, msg = call(ok)
        assert rc == 0, msg
        assert scratch(_lib.SCRATCH_CANVAS) and scratch(_lib.SCRATCH_UNPAD)
        eng.join()
        torch.cuda.synchronize()
        want, _ = _canvas_after(eng, [torch.from_numpy(rgb).to(_dev())])
        got, _ = _canvas_after(eng, [frame])
        assert torch.equal(got, want)
    finally:
        eng.close()


def _heads_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.bbox == y.bbox and x.score == y.score
        for k in ("shape", "expression", "jaw", "rotation", "eyeballs", "neck", "translation", "scale"):
            assert torch.equal(getattr(x.flame_params, k), getattr(y.flame_params, k)), k
        assert np.array_equal(x.vertices_3d, y.vertices_3d)
        assert x.head_pose == y.head_pose


@pytest.fixture(scope="module")
def detector(gpu_lib, flame_model):
    from head_detector_amd.detector import HeadDetector

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hd = HeadDetector("vgg_heads_m", image_size=S, weights="synthetic", flame_model=flame_model, max_batch=3, seed=4)
    frames = [_frame(layout, 90, 120, seed=60 + i)[0] for i, layout in enumerate(("nv12", "i420", "nv21"))]
    scores = hd.model.model(frames)[1][:, :, 0]
    return hd, frames, float(scores[:, 3].min()), float(scores[:, 12].min())


def test_head_detector_on_frames_returns_the_heads_of_their_rgb(detector):
    hd, frames, conf, _ = detector
    rgbs = [f.to_rgb().cpu().numpy() for f in frames]
    one = hd(frames[0], confidence_threshold=conf)
    ref = hd(rgbs[0], confidence_threshold=conf)
    assert len(ref.heads) >= 1
    _heads_equal(one.heads, ref.heads)
    assert isinstance(one.original_image, np.ndarray) and np.array_equal(one.original_image, rgbs[0])
    batch = hd.detect_batch(frames, confidence_threshold=conf)
    ref_batch = hd.detect_batch(rgbs, confidence_threshold=conf)
    for got, want, rgb in zip(batch, ref_batch, rgbs):
        assert len(want.heads) >= 1
        _heads_equal(got.heads, want.heads)
        assert np.array_equal(got.original_image, rgb)
    # rgb="device": the original stays on the GPU, and the device helpers take it as it is
    dev = hd(frames[0], confidence_threshold=conf, rgb="device")
    assert isinstance(dev.original_image, torch.Tensor) and dev.original_image.is_cuda and torch.equal(dev.original_image.cpu(), torch.from_numpy(rgbs[0]))
    _heads_equal(dev.heads, ref.heads)
    drawn = dev.draw("bbox", to_host=False)
    assert isinstance(drawn, torch.Tensor) and drawn.is_cuda and np.array_equal(drawn.cpu().numpy(), ref.draw("bbox"))
    assert hd.detect_batch(frames[:2], confidence_threshold=conf, rgb="device")[1].original_image.is_cuda
    with pytest.raises(ValueError, match="not both"):
        hd.detect_batch([frames[0], rgbs[1]], confidence_threshold=conf)
    with pytest.raises(ValueError, match="YUV420Frame inputs only"):
        hd(rgbs[0], rgb="device")
    with pytest.raises(TypeError, match=r"to_rgb\(\)"):
        hd.detect_sliced(frames[0])


def test_head_tracker_on_frames_gives_the_track_ids_of_their_rgb(detector):
    from head_detector_amd.tracking import HeadTracker

    hd, frames, high, low = detector
    rule = dict(high_thr=high, low_thr=low, min_hits=1)
    on_frames, on_rgb = HeadTracker(hd, max_tracks=64, **rule), HeadTracker(hd, max_tracks=64, **rule)
    seen = 0
    for f in frames:  # three frames of one size
        got, want = on_frames.update(f), on_rgb.update(f.to_rgb().cpu().numpy())
        assert np.array_equal(got.track_ids, want.track_ids) and np.array_equal(got.hits, want.hits) and np.array_equal(got.coasting, want.coasting)
        _heads_equal(got.heads, want.heads)
        assert np.array_equal(got.original_image, want.original_image)
        seen += len(got.track_ids)
    assert seen >= 3
    both = HeadTracker(hd, max_tracks=64, **rule).update_batch(frames, rgb="device")
    assert all(r.original_image.is_cuda for r in both)
    assert np.array_equal(both[2].track_ids, got.track_ids)


def test_c_only_client_on_an_nv12_frame(gpu_lib, flame_model, tmp_path):
    """tests/c_abi_yuv_smoke.c (plain gcc, no Python): a .vghpack, one NV12 surface uploaded as it is, vgh_ctx_detect with VGH_IMG_YUV420_RAW -- its canvas and its
    outputs equal the Python engine's on the same frame byte for byte."""
    from conftest import ROOT
    from head_detector_amd import arch, pack
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    variant, h, w = "vgg_heads_m", 101, 135
    sd = arch.random_state_dict(variant, 13)
    P = arch.build_program(variant, sd, S)
    path = str(tmp_path / "m160.vghpack")
    pack.write_pack(path, P, flame_model, {}, 1)
    y, u, v = yuv_ref.picture(h, w, 77)
    buf, pitch, off = yuv_ref.surface("nv12", y, u, v, pitch=160, extra_rows=11)
    coef = yuv_coefficients("bt601", False)
    with open(tmp_path / "frame.bin", "wb") as f:
        f.write(struct.pack("<iiqqq6i", h, w, pitch, off, buf.size, *coef))
        f.write(buf.tobytes())
    frame = YUV420Frame.from_nv12(torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, matrix="bt601")
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=100)
    eng = VGHeadsEngine(variant, state_dict=sd, image_size=S, max_batch=1, use_tuning=False)
    try:
        _, sc, _ = eng.model([frame])
        conf = float(sc[0, 6, 0])
        det = eng.detect([frame], confidence_threshold=conf, flame=fl)
        n_py = det.num_heads
        assert n_py >= 1
        canvas = eng.raw_canvas()[0].cpu().numpy()
        exe = str(tmp_path / "c_abi_yuv_smoke")
        libdir = os.path.join(ROOT, "head_detector_amd")
        cc = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
              os.path.join(ROOT, "tests", "c_abi_yuv_smoke.c"), "-o", exe, "-L" + libdir, "-lvgh", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
              "-Wl,-rpath,/opt/rocm/lib"]
        subprocess.run(cc, check=True, capture_output=True, text=True)
        r = subprocess.run([exe, path, str(tmp_path / "frame.bin"), repr(conf), str(tmp_path / "c")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
        rd = lambda name, dt: np.fromfile(str(tmp_path / f"c.{name}"), dtype=dt)  # noqa: E731
        assert np.array_equal(rd("canvas", np.uint8).reshape(S, S, 3), canvas)
        assert np.array_equal(canvas, eng.raw_canvas()[0].cpu().numpy())
        n = int(rd("counts", np.int32)[0])
        assert n == int(det.counts[0]) and int(rd("n_heads", np.int32)[0]) == n_py
        kk = eng.keep_k
        assert np.array_equal(rd("boxes", np.float32).reshape(kk, 4)[:n], det.boxes[0, :n].cpu().numpy())
        assert np.array_equal(rd("scores", np.float32)[:n], det.scores[0, :n].cpu().numpy())
        assert np.array_equal(rd("flame", np.float32).reshape(kk, 413)[:n], det.flame_params[0, :n].cpu().numpy())
        V = fl.num_vertices
        assert np.array_equal(rd("head_image", np.int32)[:n_py], det.head_image.cpu().numpy().astype(np.int32))
        assert np.array_equal(rd("proj", np.float32).reshape(-1, V, 3)[:n_py], det.vertices_3d.cpu().numpy())
        assert np.array_equal(rd("rpy", np.float32).reshape(-1, 3)[:n_py], det.head_pose.cpu().numpy())
        assert np.array_equal(rd("unpad", np.float32), np.array(geometry(h, w, S)[2:], dtype=np.float32))
    finally:
        eng.close()
