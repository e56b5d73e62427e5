"""Letterbox stage and whole vgh_detect time: per-image route vs VGH_IMG_U8_RAW, on photographs of mixed real-world sizes already on the device.

    per-image route: letterbox.letterbox() of every image (numpy tables, 4 table uploads, 1 vgh_letterbox launch each) into a canvas batch
                     + the host-built un-pad table, then vgh_detect(VGH_IMG_U8_NHWC)
    RAW:             vgh_detect(VGH_IMG_U8_RAW): per arena chunk ONE staging upload and ONE batched letterbox launch, then the network

HIP events on the caller's stream bracket each call (median over --iters); the letterbox stage of the per-image route is bracketed on its own.
Inside vgh_detect the RAW letterbox cannot be bracketed from here: its device time comes from a `rocprofv3 --kernel-trace --stats` run of this
tool (kernel letterbox_batch_kernel vs letterbox_kernel).  Also prints the bytes the batched kernel must move (canvas writes + the source rows and
columns its taps touch), so that kernel time turns into bytes/s.

    python tools/raw_letterbox_bench.py [--variant vgg_heads_l] [--batch 64] [--iters 20] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from head_detector_amd.engine import VGHeadsEngine  # noqa: E402
from head_detector_amd.flame import FLAMELayer  # noqa: E402
from head_detector_amd.letterbox import axis_tables, geometry, letterbox  # noqa: E402
from head_detector_amd.synthetic import synthetic_flame_model  # noqa: E402

# (h, w) of common camera / video frames, 480p .. 4K, landscape and portrait
SIZES = [(480, 640), (480, 854), (720, 1280), (1080, 1920), (1440, 2560), (2160, 3840), (3024, 4032), (3000, 4000), (1080, 1080), (768, 1024),
         (640, 480), (1280, 720), (1920, 1080), (4032, 3024), (1200, 1600), (960, 1280)]


def source_bytes(h, w, c, S):
    """Bytes of the source rows x columns the 8x8 taps of the letterbox touch (each once)."""
    nh, nw, _, _, _ = geometry(h, w, S)
    rows = set()
    for o in axis_tables(h, nh)[0]:
        rows.update(min(max(int(o) - 3 + k, 0), h - 1) for k in range(8))
    cols = set()
    for o in axis_tables(w, nw)[0]:
        cols.update(min(max(int(o) - 3 + k, 0), w - 1) for k in range(8))
    return len(rows) * len(cols) * 3  # 3 of the C channels are read


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="vgg_heads_l")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raw_letterbox_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    S, B = a.size, a.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = [SIZES[i % len(SIZES)] for i in range(B)]
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=gen) for h, w in shapes]
    fl = FLAMELayer(model=synthetic_flame_model(seed=3), device=dev, max_heads=B * 100)
    eng = VGHeadsEngine(a.variant, image_size=S, max_batch=B, seed=1)
    canvas = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def per_image_route():
        ev[0].record(cur)
        unpad = []
        for i, im in enumerate(images):
            _, (px, py), sc = letterbox(im, S, dev, out=canvas[i])
            unpad.append([px, py, sc])
        ev[1].record(cur)
        det = eng.detect(canvas, confidence_threshold=conf, flame=fl, unpad=torch.tensor(unpad, dtype=torch.float32, device=dev))
        ev[2].record(cur)
        return det

    def raw_route():
        ev[0].record(cur)
        det = eng.detect(images, confidence_threshold=conf, flame=fl)
        ev[2].record(cur)
        return det

    letterbox(images[0], S, dev, out=canvas[0])
    _, sc, _ = eng.model(torch.stack([letterbox(im, S, dev)[0] for im in images[:B]]))
    conf = float(sc[:, 3, 0].min())
    # the two routes agree (bit for bit; tests/test_gpu_raw_images.py pins it)
    d_old, d_new = per_image_route(), raw_route()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_old.counts, d_new.counts) and torch.equal(d_old.boxes, d_new.boxes) and torch.equal(d_old.vertices_3d, d_new.vertices_3d))
    res = {"variant": a.variant, "image_size": S, "batch": B, "arena_batch": eng.arena_batch, "heads": d_new.num_heads, "outputs_identical": same,
           "source_mpix_mean": float(np.mean([h * w for h, w in shapes]) / 1e6)}
    for name, fn in (("per_image", per_image_route), ("raw", raw_route)) * 2:  # alternated twice: the second round is reported
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        whole, stage, host = [], [], []
        for _ in range(a.iters):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t) * 1e3)
            whole.append(ev[0].elapsed_time(ev[2]))
            if name == "per_image":
                stage.append(ev[0].elapsed_time(ev[1]))
        res[f"{name}_detect_ms"] = float(np.median(whole))
        res[f"{name}_host_ms"] = float(np.median(host))
        if stage:
            res["per_image_letterbox_stage_ms"] = float(np.median(stage))
    src = sum(source_bytes(h, w, 3, S) for h, w in shapes)
    res["batched_kernel_bytes"] = {"canvas_write": B * S * S * 3, "source_read": src, "total": B * S * S * 3 + src}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
