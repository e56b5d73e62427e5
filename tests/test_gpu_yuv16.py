"""GPU (-m gpu): VGH_IMG_YUV420P16_RAW -- 10- and 12-bit P010 / I010 video frames converted to RGB bytes inside the batched device letterbox -- against what
defines it: the conversion rule of include/vgh.h restated in NumPy (tests/yuv16_ref.py), then VGH_IMG_U8_RAW on those RGB arrays.  Everything is compared byte
for byte."""
import ctypes as C
import os
import struct
import subprocess
import warnings

import numpy as np
import pytest
import torch

import yuv16_ref
import yuv_ref
from head_detector_amd import _lib
from head_detector_amd.letterbox import geometry
from head_detector_amd.video import YUV420Frame, YUV420Frame16, yuv_coefficients

pytestmark = pytest.mark.gpu

S = 160
FACTORY = {"p010": YUV420Frame16.from_p010, "i010": YUV420Frame16.from_i010}
# both layouts at both depths, in both ranges and with the three matrices: 8 frames of one picture = 2 batches of 4
COMBOS = [("p010", 10, "bt709", False), ("i010", 10, "bt601", True), ("p010", 12, "bt2020", True), ("i010", 12, "bt601", False),
          ("i010", 10, "bt2020", False), ("p010", 10, "bt709", True), ("i010", 12, "bt709", True), ("p010", 12, "bt601", False)]


def _dev():
    return torch.device("cuda", 0)


def _frame(layout, h, w, seed, D=10, saturating=False, matrix="bt709", full_range=False, pitched=True):
    """-> (YUV420Frame16 on the GPU: views of ONE uploaded surface with pitched luma and chroma rows, an aligned chroma offset, sentinel bytes between the samples
    and garbage in every word's unused bits; its RGB restatement, NumPy)."""
    shift = 16 - D if layout == "p010" else 0
    y, u, v = yuv16_ref.picture16(h, w, seed, D, saturating, shift)
    cw = u.shape[1]
    buf, pitch, off = yuv16_ref.surface16(layout, y, u, v, pitch=4 * cw + 20, extra_rows=3) if pitched else yuv16_ref.surface16(layout, y, u, v)
    frame = FACTORY[layout](torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, bit_depth=D, matrix=matrix, full_range=full_range)
    return frame, yuv16_ref.yuv16_to_rgb(y, u, v, yuv16_ref.coefficients(matrix, full_range, D), D, shift)


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
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (47, 61), (250, 33), (160, 160), (360, 640)])
def test_deep_canvas_equals_raw_canvas_of_the_restated_rgb(engine_m, h, w):
    eng = engine_m
    assert eng.arena_batch >= 4
    for saturating in (False, True):
        for at in range(0, len(COMBOS), 4):
            frames, rgbs = [], []
            for layout, D, matrix, full in COMBOS[at:at + 4]:
                f, rgb = _frame(layout, h, w, seed=1000 * h + w, D=D, saturating=saturating, matrix=matrix, full_range=full)
                assert 2 * f.y_pitch > 2 * w and f.uv_pitch > f.chroma_step * ((w + 1) // 2)
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
    # one picture's samples in both layouts (MSB-aligned with garbage below, LSB-aligned with garbage above): one canvas
    y, u, v = yuv16_ref.picture16(h, w, 5, 10, False, 0)
    low = np.uint16(1023)
    pair = []
    for layout, shift in (("p010", 6), ("i010", 0)):
        noise = yuv16_ref.picture16(h, w, 6, 10, False, shift)
        keep = np.uint16(1023 << shift)
        planes = [((p & low) << np.uint16(shift)) | (n & ~keep) for p, n in zip((y, u, v), noise)]
        buf, pitch, off = yuv16_ref.surface16(layout, *planes)
        pair.append(FACTORY[layout](torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off))
    got, _ = _canvas_after(eng, pair)
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("h,w", [(47, 61), (360, 640)])
def test_p010_of_shifted_nv12_samples_gives_the_canvas_of_the_nv12_frame(engine_m, h, w):
    """The tie to the 8-bit yardstick: a P010 frame whose words are an NV12 picture's samples << 8, limited range, through VGH_IMG_YUV420P16_RAW == that NV12 frame
    through VGH_IMG_YUV420_RAW."""
    eng = engine_m
    for matrix in ("bt709", "bt601", "bt2020"):
        y, u, v = yuv_ref.picture(h, w, 31 * h + w)
        buf, pitch, off = yuv_ref.surface("nv12", y, u, v, pitch=2 * u.shape[1] + 10, extra_rows=3)
        nv12 = YUV420Frame.from_nv12(torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, matrix=matrix)
        deep = [p.astype(np.uint16) << np.uint16(8) for p in (y, u, v)]
        buf, pitch, off = yuv16_ref.surface16("p010", *deep, pitch=4 * u.shape[1] + 20, extra_rows=3)
        p010 = YUV420Frame16.from_p010(torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, matrix=matrix)
        want, want_unpad = _canvas_after(eng, [nv12])
        got, got_unpad = _canvas_after(eng, [p010])
        assert torch.equal(got, want) and torch.equal(got_unpad, want_unpad)


def _mixed(seed):
    """A batch of deep frames of different sizes, layouts and depths -> (frames, their RGB restatements as GPU tensors)."""
    spec = [("p010", 10, 90, 120, "bt709", False), ("i010", 12, 201, 77, "bt601", True), ("p010", 12, 47, 61, "bt2020", False), ("i010", 10, 360, 640, "bt601", False)]
    pairs = [_frame(layout, h, w, seed + i, D=D, matrix=m, full_range=fr) for i, (layout, D, h, w, m, fr) in enumerate(spec)]
    return [f for f, _ in pairs], [torch.from_numpy(r).to(_dev()) for _, r in pairs]


def test_deep_detect_equals_raw_detect_of_the_restated_rgb(gpu_lib, flame_model):
    """Every detection output -- boxes, scores, parameters, counts, head list, vertices, head pose, the un-pad table -- of vgh_detect(VGH_IMG_YUV420P16_RAW) equals
    that of vgh_detect(VGH_IMG_U8_RAW) on the restated RGB images: a mixed-size batch in one arena chunk and in two (arena_batch 2 for 4 frames), B = 1, overlap
    mode on and off, and the three raw formats alternating on one engine (they share the staging slots and the canvas)."""
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    frames, rgbs = _mixed(seed=40)
    eight = [YUV420Frame.from_rgb(r, layout) for r, layout in zip(rgbs, ("nv12", "i420", "nv21", "nv12"))]  # 8-bit frames between the calls
    eight_rgb = [f.to_rgb() for f in eight]
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
                    canvas = eng.raw_canvas().data_ptr()
                    mid = eng.detect(eight[:n], confidence_threshold=conf, flame=fl)
                    new = eng.detect(frames[:n], confidence_threshold=conf, flame=fl)
                    torch.cuda.synchronize()
                    assert old.num_heads >= n
                    _same(new, old)
                    assert torch.equal(eng.raw_unpad()[:n], unpad_old)
                    assert eng.raw_canvas().data_ptr() == canvas  # one canvas for the three formats
                    _same(mid, eng.detect(eight_rgb[:n], confidence_threshold=conf, flame=fl))
            eng.set_overlap(False)
        finally:
            eng.close()


def test_deep_descriptors_are_validated_before_anything_runs(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine

    eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=4, seed=2)
    try:
        det = eng._det
        scratch = lambda which: gpu_lib.vgh_detector_scratch(det, which)  # noqa: E731
        assert not scratch(_lib.SCRATCH_CANVAS) and not scratch(_lib.SCRATCH_UNPAD)
        frame, rgb = _frame("p010", 60, 80, seed=3)
        coef = yuv_coefficients(bit_depth=10)

        def desc(**over):
            d = dict(y_dev=frame.y.data_ptr(), u_dev=frame.u.data_ptr(), v_dev=frame.v.data_ptr(), h=60, w=80, y_pitch_bytes=2 * frame.y_pitch,
                     uv_pitch_bytes=2 * frame.uv_pitch, chroma_step=4, bit_depth=10, shift=6, y_offset=coef[0], cy=coef[1], crv=coef[2], cgu=coef[3], cgv=coef[4], cbu=coef[5])
            d.update(over)
            return _lib.Yuv420P16Image(**d)

        def call(*descs):
            arr = (_lib.Yuv420P16Image * len(descs))(*descs)
            rc = gpu_lib.vgh_detector_candidates(det, C.addressof(arr), _lib.VGH_IMG_YUV420P16_RAW, len(descs), eng._sp())
            return rc, gpu_lib.vgh_last_error().decode()

        ok = desc()
        yp = frame.y.data_ptr()
        cases = [((ok, desc(y_dev=None)), 1, "null plane"), ((desc(u_dev=None), ok), 0, "null plane"), ((ok, ok, desc(v_dev=None)), 2, "null plane"),
                 ((ok, desc(y_dev=yp + 1)), 1, "odd plane pointer"), ((desc(v_dev=frame.u.data_ptr() + 1),), 0, "odd plane pointer"),
                 ((ok, desc(y_pitch_bytes=158)), 1, "y_pitch_bytes"), ((desc(y_pitch_bytes=161),), 0, "y_pitch_bytes"),
                 ((desc(uv_pitch_bytes=158),), 0, "uv_pitch_bytes"), ((desc(uv_pitch_bytes=161),), 0, "uv_pitch_bytes"),
                 ((desc(chroma_step=2, uv_pitch_bytes=78),), 0, "uv_pitch_bytes"), ((desc(w=81, y_pitch_bytes=162, uv_pitch_bytes=162),), 0, "uv_pitch_bytes"),
                 ((ok, desc(chroma_step=0)), 1, "chroma_step"), ((ok, ok, ok, desc(chroma_step=3)), 3, "chroma_step"), ((desc(chroma_step=1),), 0, "chroma_step"),
                 ((desc(chroma_step=8),), 0, "chroma_step"),
                 ((desc(bit_depth=8),), 0, "bit_depth"), ((ok, desc(bit_depth=16)), 1, "bit_depth"), ((desc(bit_depth=11),), 0, "bit_depth"),
                 ((desc(shift=7),), 0, "shift"), ((desc(shift=-1),), 0, "shift"), ((ok, desc(bit_depth=12, shift=5)), 1, "shift"),
                 ((desc(y_offset=-1),), 0, "y_offset"), ((ok, desc(y_offset=1024)), 1, "y_offset"), ((desc(bit_depth=12, shift=4, y_offset=4096),), 0, "y_offset"),
                 ((desc(cy=(1 << 17) + 1),), 0, "coefficient cy"), ((desc(cy=-1),), 0, "coefficient cy"), ((ok, desc(cgv=-(1 << 18) - 1)), 1, "coefficient cgv"),
                 ((desc(cbu=1 << 30),), 0, "coefficient cbu"), ((desc(crv=(1 << 18) + 1),), 0, "coefficient crv"), ((desc(cgu=-(1 << 19)),), 0, "coefficient cgu"),
                 ((desc(h=0),), 0, "empty"),
                 ((ok, desc(h=1, w=4000, y_pitch_bytes=8000, uv_pitch_bytes=8000)), 1, "elongated")]
        for descs, index, words in cases:
            rc, msg = call(*descs)
            assert rc == -1 and f"image {index}" in msg and words in msg, msg  # VGH_ERR_INVALID
        assert not scratch(_lib.SCRATCH_CANVAS)  # a rejected call allocates nothing
        for entry in (gpu_lib.vgh_net_forward, gpu_lib.vgh_net_capture):
            rc = entry(eng._net, frame.y.data_ptr(), _lib.VGH_IMG_YUV420P16_RAW, 1, eng._sp())
            assert rc == -1 and b"not a canvas" in gpu_lib.vgh_last_error()
        op_ms = (C.c_float * len(eng.program.ops))()
        rc = gpu_lib.vgh_net_profile(eng._net, frame.y.data_ptr(), _lib.VGH_IMG_YUV420P16_RAW, 1, eng._sp(), op_ms)
        assert rc == -1 and b"not a canvas" in gpu_lib.vgh_last_error()
        rc = gpu_lib.vgh_detector_candidates(det, frame.y.data_ptr(), 5, 1, eng._sp())
        assert rc == -1 and b"unknown image format 5" in gpu_lib.vgh_last_error()
        with pytest.raises(ValueError, match="not both"):
            eng.detect([frame, torch.from_numpy(rgb).to(_dev())])
        # the largest admissible coefficients are accepted (samples 0: only the bounds are exercised, the bytes are whatever the rule gives), and a following valid
        # call works
        rc, msg = call(desc(cy=1 << 17, crv=-(1 << 18), cgu=1 << 18, cgv=1 << 18, cbu=-(1 << 18), y_offset=1023))
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
    frames = [_frame(layout, 90, 120, seed=60 + i, D=D)[0] for i, (layout, D) in enumerate((("p010", 10), ("i010", 10), ("p010", 12)))]
    scores = hd.model.model(frames)[1][:, :, 0]
    return hd, frames, float(scores[:, 3].min()), float(scores[:, 12].min())


def test_head_detector_on_deep_frames_returns_the_heads_of_their_rgb(detector):
    hd, frames, conf, _ = detector
    rgbs = [f.to_rgb().cpu().numpy() for f in frames]
    one = hd(frames[0], confidence_threshold=conf)
    ref = hd(rgbs[0], confidence_threshold=conf)
    assert len(ref.heads) >= 1
    _heads_equal(one.heads, ref.heads)
    assert isinstance(one.original_image, np.ndarray) and np.array_equal(one.original_image, rgbs[0]) and one.source_frame is frames[0]
    batch = hd.detect_batch(frames, confidence_threshold=conf)
    ref_batch = hd.detect_batch(rgbs, confidence_threshold=conf)
    for got, want, rgb, f in zip(batch, ref_batch, rgbs, frames):
        assert len(want.heads) >= 1
        _heads_equal(got.heads, want.heads)
        assert np.array_equal(got.original_image, rgb) and got.source_frame is f
    # rgb="device": the original stays on the GPU, and the device helpers take it as it is
    dev = hd(frames[0], confidence_threshold=conf, rgb="device")
    assert isinstance(dev.original_image, torch.Tensor) and dev.original_image.is_cuda and torch.equal(dev.original_image.cpu(), torch.from_numpy(rgbs[0]))
    _heads_equal(dev.heads, ref.heads)
    drawn = dev.draw("bbox", to_host=False)
    assert isinstance(drawn, torch.Tensor) and drawn.is_cuda and np.array_equal(drawn.cpu().numpy(), ref.draw("bbox"))
    assert hd.detect_batch(frames[:2], confidence_threshold=conf, rgb="device")[1].original_image.is_cuda
    # rgb="none": no RGB copy; the three consumers that work in 8-bit planes refuse the deep frame and name the bridge, which then serves them
    bare = hd(frames[0], confidence_threshold=conf, rgb="none")
    assert bare.original_image is None and bare.source_frame is frames[0]
    _heads_equal(bare.heads, ref.heads)
    for call in (bare.anonymize_frame, bare.draw_overlay, lambda: bare.get_head_tensors(32, aligned=False)):
        with pytest.raises(ValueError, match=r"source_frame\.to_8bit\(\)"):
            call()
    with pytest.raises(ValueError, match=r"source_frame\.to_8bit\(\)"):
        one.anonymize_frame()
    narrow = frames[0].to_8bit()
    assert isinstance(narrow, YUV420Frame) and narrow.device == frames[0].device and narrow.chroma_step == 2
    samples = ((frames[0].y.to(torch.int32) & 0xFFFF) >> 6) & 1023  # P010 at 10 bits
    assert torch.equal(narrow.y, ((samples + 2) >> 2).clamp(max=255).to(torch.uint8))
    from head_detector_amd.video import anonymize_frame

    hidden = anonymize_frame(narrow, bare.heads, "fill", "box")
    assert isinstance(hidden, YUV420Frame) and not torch.equal(hidden.y, narrow.y)
    with pytest.raises(ValueError, match="not both"):
        hd.detect_batch([frames[0], rgbs[1]], confidence_threshold=conf)
    with pytest.raises(ValueError, match="not both"):
        hd.detect_batch([frames[0], narrow], confidence_threshold=conf)
    with pytest.raises(TypeError, match=r"to_rgb\(\)"):
        hd.detect_sliced(frames[0])


def test_head_tracker_on_deep_frames_gives_the_track_ids_of_their_rgb(detector):
    from head_detector_amd.tracking import HeadTracker

    hd, frames, high, low = detector
    rule = dict(high_thr=high, low_thr=low, min_hits=1)
    on_frames, on_rgb = HeadTracker(hd, max_tracks=64, **rule), HeadTracker(hd, max_tracks=64, **rule)
    seen = 0
    for f in frames:  # three frames of one size
        got, want = on_frames.update(f), on_rgb.update(f.to_rgb().cpu().numpy())
        assert np.array_equal(got.track_ids, want.track_ids) and np.array_equal(got.hits, want.hits) and np.array_equal(got.coasting, want.coasting)
        _heads_equal(got.heads, want.heads)
        assert np.array_equal(got.original_image, want.original_image) and got.source_frame is f
        seen += len(got.track_ids)
    assert seen >= 3
    both = HeadTracker(hd, max_tracks=64, **rule).update_batch(frames, rgb="device")
    assert all(r.original_image.is_cuda for r in both)
    assert np.array_equal(both[2].track_ids, got.track_ids)


def test_c_only_client_on_a_p010_frame(gpu_lib, flame_model, tmp_path):
    """tests/c_abi_yuv16_smoke.c (plain gcc, no Python): a .vghpack, one P010 surface uploaded as it is, vgh_ctx_detect with VGH_IMG_YUV420P16_RAW -- its canvas and
    its outputs equal the Python engine's on the same frame byte for byte."""
    from conftest import ROOT
    from head_detector_amd import arch, pack
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    variant, h, w = "vgg_heads_m", 101, 135
    sd = arch.random_state_dict(variant, 13)
    P = arch.build_program(variant, sd, S)
    path = str(tmp_path / "m160.vghpack")
    pack.write_pack(path, P, flame_model, {}, 1)
    y, u, v = yuv16_ref.picture16(h, w, 77, 10, False, 6)
    buf, pitch, off = yuv16_ref.surface16("p010", y, u, v, pitch=320, extra_rows=11)
    coef = yuv_coefficients("bt601", False, 10)
    with open(tmp_path / "frame.bin", "wb") as f:
        f.write(struct.pack("<iiqqq8i", h, w, pitch, off, buf.size, 10, 6, *coef))
        f.write(buf.tobytes())
    frame = YUV420Frame16.from_p010(torch.from_numpy(buf).to(_dev()), h, w, pitch=pitch, uv_offset=off, matrix="bt601")
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=100)
    eng = VGHeadsEngine(variant, state_dict=sd, image_size=S, max_batch=1, use_tuning=False)
    try:
        _, sc, _ = eng.model([frame])
        conf = float(sc[0, 6, 0])
        det = eng.detect([frame], confidence_threshold=conf, flame=fl)
        n_py = det.num_heads
        assert n_py >= 1
        canvas = eng.raw_canvas()[0].cpu().numpy()
        exe = str(tmp_path / "c_abi_yuv16_smoke")
        libdir = os.path.join(ROOT, "head_detector_amd")
        cc = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
              os.path.join(ROOT, "tests", "c_abi_yuv16_smoke.c"), "-o", exe, "-L" + libdir, "-lvgh", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
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
