"""GPU (-m gpu): VGH_IMG_U8_RAW -- images of any size letterboxed inside vgh_detect (one batched launch per arena chunk, tables built in the
library) -- against the per-image route it replaces: letterbox.letterbox() of every image, vgh_detect on the u8 canvas batch, the host's
un-pad table.  Everything is compared bit for bit."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from head_detector_amd import _lib
from head_detector_amd.letterbox import PAD_VALUE, geometry, letterbox

pytestmark = pytest.mark.gpu

S = 320


def _dev():
    return torch.device("cuda", 0)


def _sources(seed=0):
    """The kinds of photographs a caller hands over: landscape, portrait, square, up- and downscaled, odd sizes, RGBA, padded rows.
    -> list of (name, GPU uint8 tensor [h, w, C] (possibly a strided view), dense numpy copy)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for name, (h, w, c) in [("landscape", (480, 640, 3)), ("portrait", (640, 480, 3)), ("square", (500, 500, 3)), ("upscale", (97, 131, 3)),
                            ("downscale", (3000, 4000, 3)), ("odd", (333, 517, 3)), ("rgba", (211, 307, 4))]:
        t = torch.randint(0, 256, (h, w, c), dtype=torch.uint8, generator=g)
        out.append((name, t.to(_dev()), t.numpy()))
    wide = torch.randint(0, 256, (251, 401, 3), dtype=torch.uint8, generator=g).to(_dev())
    view = wide[:, :389]  # rows 401 * 3 bytes apart, 389 * 3 used
    assert view.stride(0) > view.shape[1] * view.shape[2]
    out.append(("pitched", view, view.cpu().numpy()))
    return out


def _old_route(images_np, dev):
    """detect_batch before VGH_IMG_U8_RAW: letterbox() per image -> u8 canvas batch + the host-built un-pad table."""
    canv, unpad = [], []
    for im in images_np:
        c, (px, py), sc = letterbox(im, S, dev)
        canv.append(c)
        unpad.append([px, py, sc])
    return torch.stack(canv).contiguous(), torch.tensor(unpad, dtype=torch.float32, device=dev)


def _same(a, b):
    assert torch.equal(a.counts, b.counts)
    assert a.num_heads == b.num_heads
    for f in ("boxes", "scores", "flame_params"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("head_image", "vertices_3d", "head_pose"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


@pytest.fixture(scope="module")
def engine_m(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine

    eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=8, seed=11)
    yield eng
    eng.close()


def test_raw_canvas_equals_letterbox_of_every_image(engine_m):
    """The detector's canvas (VGH_SCRATCH_CANVAS) after a RAW call holds letterbox.letterbox() of each image, bit for bit: every kind of source alone,
    then all of them in one batch; the un-pad table (VGH_SCRATCH_UNPAD) is letterbox.geometry()'s (pad_x, pad_y, scale)."""
    eng = engine_m
    src = _sources()
    assert len(src) <= eng.arena_batch
    for batch in [[s] for s in src] + [src]:
        eng.forward_candidates([t for _, t, _ in batch])
        eng.join()
        torch.cuda.synchronize()
        canvas, unpad = eng.raw_canvas(), eng.raw_unpad()
        for i, (name, _, im) in enumerate(batch):
            want, (px, py), sc = letterbox(im, S, _dev())
            assert torch.equal(canvas[i], want), (name, int((canvas[i] != want).sum()))
            nh, nw, gx, gy, gs = geometry(im.shape[0], im.shape[1], S)
            assert (gx, gy, gs) == (px, py, sc)
            assert torch.equal(unpad[i].cpu(), torch.tensor([gx, gy, gs], dtype=torch.float32)), name
            border = canvas[i, gy + nh:].reshape(-1, 3) if gy + nh < S else canvas[i, :, gx + nw:].reshape(-1, 3)
            if border.numel():
                assert (border.cpu() == torch.tensor(PAD_VALUE, dtype=torch.uint8)).all()


def test_raw_descriptors_are_validated_before_anything_runs(gpu_lib):
    from head_detector_amd.engine import VGHeadsEngine

    eng = VGHeadsEngine("vgg_heads_m", image_size=S, max_batch=4, seed=2)
    try:
        det = eng._det
        scratch = lambda which: gpu_lib.vgh_detector_scratch(det, which)  # noqa: E731
        assert not scratch(_lib.SCRATCH_CANVAS) and not scratch(_lib.SCRATCH_UNPAD)  # nothing before the first RAW call
        good = torch.randint(0, 256, (60, 80, 3), dtype=torch.uint8, device=_dev())

        def call(*descs):
            arr = (_lib.RawImage * len(descs))(*descs)
            rc = gpu_lib.vgh_detector_candidates(det, C.addressof(arr), _lib.VGH_IMG_U8_RAW, len(descs), eng._sp())
            return rc, gpu_lib.vgh_last_error().decode()

        ok = _lib.RawImage(good.data_ptr(), 60, 80, 3, 240)
        for descs, index, words in [((ok, _lib.RawImage(None, 60, 80, 3, 240)), 1, "null"),
                                    ((_lib.RawImage(good.data_ptr(), 60, 80, 2, 240), ok), 0, "channels"),
                                    ((ok, ok, _lib.RawImage(good.data_ptr(), 60, 80, 3, 239)), 2, "pitch"),
                                    ((_lib.RawImage(good.data_ptr(), 1, 4000, 3, 12000),), 0, "elongated")]:
            rc, msg = call(*descs)
            assert rc == -1 and f"image {index}" in msg and words in msg, msg  # VGH_ERR_INVALID
        assert not scratch(_lib.SCRATCH_CANVAS)  # a rejected call allocates nothing
        rc = gpu_lib.vgh_net_forward(eng._net, good.data_ptr(), _lib.VGH_IMG_U8_RAW, 1, eng._sp())
        assert rc == -1 and b"not a canvas" in gpu_lib.vgh_last_error()
        with pytest.raises(ValueError):
            eng.detect([good.cpu()])  # raw images live on the device
        rc, msg = call(ok)
        assert rc == 0, msg
        assert scratch(_lib.SCRATCH_CANVAS) and scratch(_lib.SCRATCH_UNPAD)
        torch.cuda.synchronize()
    finally:
        eng.close()


@pytest.mark.parametrize("variant", ["vgg_heads_m", "vgg_heads_l"])
def test_raw_detect_equals_letterbox_then_canvas_route(gpu_lib, flame_model, variant):
    """vgh_detect(VGH_IMG_U8_RAW) == letterbox() per image + vgh_detect(VGH_IMG_U8_NHWC) + the host un-pad table, every output bit for bit:
    one arena chunk (lazy FLAME gather), several chunks (arena_batch 3 for 8 images), overlap mode on and off."""
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    src = _sources(seed=5)
    raw = [t for _, t, _ in src]
    canvas, unpad = _old_route([im for _, _, im in src], _dev())
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=len(src) * 100)
    for arena in (None, 3):
        eng = VGHeadsEngine(variant, image_size=S, max_batch=len(src), seed=7, arena_batch=arena)
        try:
            assert (eng.arena_batch < len(src)) == (arena is not None)
            _, sc, _ = eng.model(canvas)
            conf = float(sc[:, 4, 0].min())
            for overlap in (False, True):
                eng.set_overlap(overlap)
                old = eng.detect(canvas, confidence_threshold=conf, flame=fl, unpad=unpad)
                new = eng.detect(raw, confidence_threshold=conf, flame=fl)
                torch.cuda.synchronize()
                assert old.num_heads >= len(src)
                _same(new, old)
                assert torch.equal(eng.raw_unpad()[: len(src)], unpad)
            # the un-padding the table does is letterbox.geometry()'s: a caller-supplied table still wins
            mine = torch.tensor([[1.0, 2.0, 0.5]], device=_dev()).expand(len(src), 3).contiguous()
            a = eng.detect(raw, confidence_threshold=conf, flame=fl, unpad=mine)
            b = eng.detect(canvas, confidence_threshold=conf, flame=fl, unpad=mine)
            torch.cuda.synchronize()
            _same(a, b)
            eng.set_overlap(False)
        finally:
            eng.close()


def test_detect_batch_equals_the_per_image_route(gpu_lib, flame_model):
    """HeadDetector.detect_batch (now VGH_IMG_U8_RAW) returns the heads the per-image route returned: letterbox() + engine.detect(U8_NHWC) + the same
    host-side un-pad of the boxes, bit for bit."""
    import warnings

    from head_detector_amd.detector import HeadDetector
    from head_detector_amd.head_info import Bbox, FlameParams

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hd = HeadDetector("vgg_heads_m", image_size=S, weights="synthetic", flame_model=flame_model, max_batch=4, seed=4)
    imgs = [im for name, _, im in _sources(seed=9) if name in ("landscape", "portrait", "upscale", "rgba")]
    canvas, unpad = _old_route(imgs, hd._device)
    _, sc, _ = hd.model.model(canvas)
    conf = float(sc[:, 3, 0].min())
    got = hd.detect_batch(imgs, confidence_threshold=conf)
    det = hd.model.detect(canvas, confidence_threshold=conf, flame=hd._flame, unpad=unpad)
    counts, boxes, scores = det.counts.cpu().numpy(), det.boxes.cpu().numpy(), det.scores.cpu().numpy()
    params, verts, rpy = det.flame_params.cpu(), det.vertices_3d.cpu().numpy(), det.head_pose.cpu().numpy().astype(np.float64)
    assert det.num_heads >= len(imgs)
    at = 0
    for b, im in enumerate(imgs):
        _, _, px, py, scale = geometry(im.shape[0], im.shape[1], S)
        heads = got[b].heads
        assert len(heads) == int(counts[b])
        for i, h in enumerate(heads):
            bb = boxes[b, i].clip(0, S)
            bb[[0, 2]] -= px
            bb[[1, 3]] -= py
            bb = np.rint(bb / scale).astype(int)
            assert h.bbox == Bbox(x=bb[0], y=bb[1], w=bb[2] - bb[0], h=bb[3] - bb[1])
            assert h.score == scores[b, i]
            fp = FlameParams.from_3dmm(params[b, i].unsqueeze(0))
            fp.scale = fp.scale / scale
            for k in ("shape", "expression", "jaw", "rotation", "eyeballs", "neck", "translation", "scale"):
                assert torch.equal(getattr(h.flame_params, k), getattr(fp, k)), k
            assert np.array_equal(h.vertices_3d, verts[at])
            assert (h.head_pose.roll, h.head_pose.pitch, h.head_pose.yaw) == tuple(float(v) for v in rpy[at])
            at += 1


def test_c_only_client_on_raw_images(gpu_lib, flame_model, tmp_path):
    """tests/c_abi_raw_smoke.c (plain gcc, no Python, no tables): a .vghpack, raw images of different sizes uploaded as they are, vgh_ctx_detect with
    VGH_IMG_U8_RAW and VGH_SCRATCH_UNPAD -- its outputs equal the Python engine's RAW path byte for byte, its un-pad table letterbox.geometry()'s."""
    from conftest import ROOT
    from head_detector_amd import arch, pack
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer

    variant, B = "vgg_heads_m", 3
    sd = arch.random_state_dict(variant, 13)
    P = arch.build_program(variant, sd, S)
    names = {i: "256x128_w64x64_k1_r3" for i, op in enumerate(P.ops) if op["kind"] == 1 and op["cout_pad"] % 128 == 0 and i % 2 == 0}
    path = str(tmp_path / "m320.vghpack")
    pack.write_pack(path, P, flame_model, names, B)
    src = [s for s in _sources(seed=21) if s[0] in ("pitched", "rgba", "portrait")]
    with open(tmp_path / "images.bin", "wb") as f:
        for _, t, _ in src:
            h, w, c = t.shape
            pitch = t.stride(0)
            rows = torch.as_strided(t, (h, pitch), (pitch, 1)).cpu().numpy()  # the rows with their padding, as they lie on the device
            f.write(struct.pack("<iiiq", h, w, c, pitch))
            f.write(rows.tobytes())
    fl = FLAMELayer(model=flame_model, device=_dev(), max_heads=B * 100)
    eng = VGHeadsEngine(variant, state_dict=sd, image_size=S, max_batch=B, use_tuning=False)
    try:
        for i, n in names.items():
            eng.set_cfg(i, eng.cfg_names().index(n))
        raw = [t for _, t, _ in src]
        _, sc, _ = eng.model(raw)
        conf = float(sc[:, 6, 0].min())
        det = eng.detect(raw, confidence_threshold=conf, flame=fl)
        n_py = det.num_heads
        assert n_py >= B
        exe = str(tmp_path / "c_abi_raw_smoke")
        libdir = os.path.join(ROOT, "head_detector_amd")
        cc = ["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
              os.path.join(ROOT, "tests", "c_abi_raw_smoke.c"), "-o", exe, "-L" + libdir, "-lvgh", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
              "-Wl,-rpath,/opt/rocm/lib"]
        subprocess.run(cc, check=True, capture_output=True, text=True)
        r = subprocess.run([exe, path, str(tmp_path / "images.bin"), str(B), repr(conf), str(tmp_path / "c")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
        rd = lambda name, dt: np.fromfile(str(tmp_path / f"c.{name}"), dtype=dt)  # noqa: E731
        counts = rd("counts", np.int32)
        assert np.array_equal(counts, det.counts.cpu().numpy()) and int(rd("n_heads", np.int32)[0]) == n_py
        kk = eng.keep_k
        cb, cs, cf = rd("boxes", np.float32).reshape(B, kk, 4), rd("scores", np.float32).reshape(B, kk), rd("flame", np.float32).reshape(B, kk, 413)
        for i in range(B):
            n = int(counts[i])
            assert np.array_equal(cb[i, :n], det.boxes[i, :n].cpu().numpy()) and np.array_equal(cs[i, :n], det.scores[i, :n].cpu().numpy())
            assert np.array_equal(cf[i, :n], det.flame_params[i, :n].cpu().numpy())
        V = fl.num_vertices
        assert np.array_equal(rd("head_image", np.int32)[:n_py], det.head_image.cpu().numpy().astype(np.int32))
        assert np.array_equal(rd("proj", np.float32).reshape(-1, V, 3)[:n_py], det.vertices_3d.cpu().numpy())
        assert np.array_equal(rd("rpy", np.float32).reshape(-1, 3)[:n_py], det.head_pose.cpu().numpy())
        want = np.array([geometry(t.shape[0], t.shape[1], S)[2:] for _, t, _ in src], dtype=np.float32)
        assert np.array_equal(rd("unpad", np.float32).reshape(B, 3), want)
    finally:
        eng.close()
