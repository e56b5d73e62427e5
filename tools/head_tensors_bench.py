"""Head tensors (head_detector_amd/head_tensors.py, libvghcrop.so) beside the route that existed before them, alternating in one process:

    new    head_tensors / head_tensors_batch: ONE staging upload and ONE launch for every head of the call, float16 planar [n, 3, S, S]
    old    get_aligned_heads(to_host=False), then per head torch.nn.functional.interpolate (bilinear) and the normalisation in torch, then torch.stack;
           for a video frame YUV420Frame.to_rgb() comes first

    photo   a seeded 3000 x 4000 image on the device with 1 / 16 / 100 heads of about 200 x 240 pixels, S = 112 and 224
    frames  64 dense NV12 1080p frames on the device with 4 such heads each, ONE head_tensors_batch call (old: 64 to_rgb + 64 get_aligned_heads + 256 interpolate)

ms = median of HIP-event times around one whole call (host planning included: the events bracket it on the stream), sources device-resident; `launch_ms` = events
around vghc_head_tensors alone (the ONE staging upload + the ONE head_tensors_kernel launch), the rest of `new_ms` being the float64 planning on the host.  `bytes` = the least
each call must move, from the shapes: every head's rect read once (3 bytes a pixel of an image, 1.5 of a 4:2:0 frame) and the float16 result written once.  The
two routes do NOT compute the same numbers (the old one does not supersample: `max_abs_diff` shows how far apart they are).

    python tools/head_tensors_bench.py [--iters 20] [--warmup 3] [--frames 64] [--out profiles/head_tensors.txt]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from head_detector_amd import aligned, head_tensors as ht  # noqa: E402
from head_detector_amd.head_info import RPY, Bbox  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

V = 600
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def heads_on(rng, n, H, W):
    """Heads of about 200 x 240 pixels, rolled up to +-45 degrees about their own centre, wholly inside the image."""
    s = 640 / max(H, W)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(320, W - 320), rng.uniform(320, H - 320)
        ang, rad = rng.uniform(0, 2 * np.pi, V), np.sqrt(rng.uniform(0, 1, V))
        v = np.stack([cx + 100 * rad * np.cos(ang), cy + 120 * rad * np.sin(ang), rng.normal(0, 20, V)], axis=1).astype(np.float32)
        t = torch.tensor([[cx * s + (640 - int(W * s)), cy * s + (640 - int(H * s)), 0.0]], dtype=torch.float32)
        out.append(types.SimpleNamespace(vertices_3d=v, flame_params=types.SimpleNamespace(translation=t), head_pose=RPY(roll=rng.uniform(-45, 45), pitch=0.0, yaw=rng.uniform(-55, 55)),
                                         bbox=Bbox(int(cx - 100), int(cy - 120), 200, 240)))
    return out


def old_route(sources_and_heads, hidx, S, mean, std):
    out = []
    for source, heads in sources_and_heads:
        image = source.to_rgb() if isinstance(source, YUV420Frame) else source
        for crop in aligned.get_aligned_heads(image, heads, hidx, to_host=False):
            if crop.numel() == 0:
                out.append(torch.zeros(3, S, S, dtype=torch.float16, device=image.device))
                continue
            t = torch.nn.functional.interpolate(crop.permute(2, 0, 1)[None].float(), size=(S, S), mode="bilinear", align_corners=False)[0]
            out.append(((t / 255.0 - mean) / std).half())
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_tensors_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    hidx = np.sort(rng.choice(V, 200, replace=False))
    mean, std = torch.tensor(MEAN, device=dev).view(3, 1, 1), torch.tensor(STD, device=dev).view(3, 1, 1)
    H, W = 3000, 4000
    photo = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    jobs = []
    for n in (1, 16, 100):
        heads = heads_on(np.random.default_rng(n), n, H, W)
        for S in (112, 224):
            jobs.append((f"photo {H}x{W}", n, S, [(photo, heads)], 3.0))
    fh, fw = 1080, 1920
    surface = torch.from_numpy(rng.integers(16, 236, (a.frames, fh * fw * 3 // 2), dtype=np.uint8)).to(dev)
    frames = [(YUV420Frame.from_nv12(surface[k], fh, fw), heads_on(np.random.default_rng(1000 + k), 4, fh, fw)) for k in range(a.frames)]
    for S in (112, 224):
        jobs.append((f"{a.frames} NV12 frames {fh}x{fw}", 4 * a.frames, S, frames, 1.5))
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    lib = ht._lib_crop.load()
    real = lib.vghc_head_tensors

    class Timed:  # brackets the library call with events without changing the product's code path
        def vghc_head_tensors(self, *args):
            ev[4].record(cur)
            rc = real(*args)
            ev[5].record(cur)
            return rc

        def __getattr__(self, name):
            return getattr(lib, name)

    ht._lib_crop.load = lambda: Timed()
    lines = []
    for what, n, S, pairs, bytes_per_pixel in jobs:
        results = [types.SimpleNamespace(source_frame=s if isinstance(s, YUV420Frame) else None, original_image=None if isinstance(s, YUV420Frame) else s, heads=heads,
                                         head_indices=hidx) for s, heads in pairs]
        t_new, t_old, t_launch = [], [], []
        for it in range(a.warmup + a.iters):  # alternating: both routes see the same neighbours on the machine
            ev[0].record(cur)
            new = ht.head_tensors_batch(results, S, dtype=torch.float16)
            ev[1].record(cur)
            ev[2].record(cur)
            old = old_route(pairs, hidx, S, mean, std)
            ev[3].record(cur)
            torch.cuda.synchronize()
            if it >= a.warmup:
                t_new.append(ev[0].elapsed_time(ev[1])), t_old.append(ev[2].elapsed_time(ev[3])), t_launch.append(ev[4].elapsed_time(ev[5]))
        assert tuple(new.tensor.shape) == tuple(old.shape) == (n, 3, S, S)
        plans = [ht.head_tensor_plan(s.shape, heads, S, head_indices=hidx) for s, heads in pairs]
        rect_px = int(sum(int(side) ** 2 for p in plans for side in p.sides))
        least = {"rect_read": int(rect_px * bytes_per_pixel), "result_write": n * 3 * S * S * 2}
        row = {"source": what, "heads": n, "S": S, "supersample": sorted({int(k) for p in plans for k in p.supersample}), "new_ms": float(np.median(t_new)), "new_ms_min": float(np.min(t_new)), "launch_ms": float(np.median(t_launch)),
               "old_ms": float(np.median(t_old)), "old_ms_min": float(np.min(t_old)), "old_over_new": float(np.median(t_old) / np.median(t_new)), "least_bytes": least,
               "launch_GB/s": sum(least.values()) / (float(np.median(t_launch)) * 1e-3) / 1e9, "max_abs_diff": float((new.tensor.float() - old.float()).abs().max())}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/head_tensors_bench.py --iters {a.iters} --warmup {a.warmup} --frames {a.frames}: float16 planar head tensors, device-resident sources; ms = median of HIP-event "
                    "times around one whole call (host planning included); new = head_tensors_batch (one upload, one launch); old = get_aligned_heads(to_host=False) + per-head "
                    "interpolate + normalisation (frames: to_rgb() first); least_bytes = every head's rect read once + the result written once, from the shapes\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
