"""PredictionResult.get_aligned_heads on a 12 MP photograph with 1, 16 and 100 heads: where the time of a call goes.

    plan      aligned.aligned_head_plan: the per-head float64 geometry (host clock)
    tables    aligned.warp_tables of every crop + the ctypes descriptors (host clock)
    launch    HIP events around vghv_warp_crops: the ONE staging upload (descriptors + tile list + tables) and the ONE warp_crops_kernel launch.
              The kernel alone comes from a `rocprofv3 --kernel-trace --stats` run of this tool (kernel warp_crops_kernel).
    call      the whole get_aligned_heads(to_host=True): image upload (36 MB), plan, tables, launch, download of the packed crops; host clock around
              work that ends in a device synchronise.  `call_dev` is the same with the image already on the device and to_host=False.

Also prints the bytes the kernel must move -- the crop bytes it writes plus the four taps (12 bytes) it reads per pixel -- so that time turns into
bytes/s.  Medians over --iters after --warmup; the three head counts are measured twice, alternating, and the second round is reported.

    python tools/aligned_heads_bench.py [--iters 30] [--warmup 5] [--heads 1,16,100] [--out profiles/aligned_heads.txt]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from head_detector_amd import _lib_view, aligned  # noqa: E402
from head_detector_amd.head_info import RPY  # noqa: E402

H, W, V = 3000, 4000, 5023


def heads_on_photo(rng, n):
    """Heads the size a crowd photograph has them (radius 60 .. 220 px), rolled up to +-45 degrees about a centre near the head, one in six in profile (no warp)."""
    s = 640 / max(H, W)
    out = []
    for k in range(n):
        cx, cy, r = rng.uniform(200, W - 200), rng.uniform(200, H - 200), rng.uniform(60, 220)
        ang, rad = rng.uniform(0, 2 * np.pi, V), np.sqrt(rng.uniform(0, 1, V))
        v = np.stack([cx + 0.8 * r * rad * np.cos(ang), cy + r * rad * np.sin(ang), rng.normal(0, 20, V)], axis=1).astype(np.float32)
        t = torch.tensor([[(cx + rng.uniform(-20, 20)) * s + (640 - int(W * s)), (cy + rng.uniform(-20, 20)) * s + (640 - int(H * s)), 0.0]], dtype=torch.float32)
        yaw = rng.uniform(60, 90) if k % 6 == 5 else rng.uniform(-55, 55)
        out.append(types.SimpleNamespace(vertices_3d=v, flame_params=types.SimpleNamespace(translation=t), head_pose=RPY(roll=rng.uniform(-45, 45), pitch=0.0, yaw=yaw)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--heads", default="1,16,100", help="head counts, comma separated (one count for a rocprofv3 run: its stats then belong to that count)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aligned_heads_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    image_dev = torch.from_numpy(image).to(dev)
    hidx = np.sort(rng.choice(V, 1800, replace=False))
    cases = {n: heads_on_photo(np.random.default_rng(n), n) for n in (int(v) for v in a.heads.split(","))}
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lib = _lib_view.load()
    real = lib.vghv_warp_crops

    class Timed:  # brackets the library call with events without changing the product's code path
        def vghv_warp_crops(self, *args):
            ev[0].record(cur)
            rc = real(*args)
            ev[1].record(cur)
            return rc

        def __getattr__(self, name):
            return getattr(lib, name)

    lines = []
    for rnd in range(2):
        for n, heads in cases.items():
            plans = aligned.aligned_head_plan(image.shape, heads, hidx)
            px = sum(p.shape[0] * p.shape[1] for p in plans)
            t_plan, t_tab, t_launch, t_call, t_dev = [], [], [], [], []
            for it in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                plans = aligned.aligned_head_plan(image.shape, heads, hidx)
                t1 = time.perf_counter()
                for p in plans:
                    if p.shape[0] and p.shape[1]:
                        aligned.warp_tables(p.matrix, p.region)
                t2 = time.perf_counter()
                aligned._lib_view.load = lambda: Timed()
                try:
                    crops = aligned.get_aligned_heads(image_dev, heads, hidx, to_host=False)
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                finally:
                    aligned._lib_view.load = lambda: lib
                launch = ev[0].elapsed_time(ev[1])
                t4 = time.perf_counter()
                host = aligned.get_aligned_heads(image, heads, hidx, to_host=True)
                torch.cuda.synchronize()
                t5 = time.perf_counter()
                if it >= a.warmup:
                    t_plan.append((t1 - t0) * 1e3), t_tab.append((t2 - t1) * 1e3), t_launch.append(launch), t_dev.append((t3 - t2) * 1e3), t_call.append((t5 - t4) * 1e3)
            assert len(crops) == len(host) == n and all(np.array_equal(c.cpu().numpy(), h) for c, h in zip(crops, host))
            med = {"heads": n, "crop_mpix": px / 1e6, "plan_ms": float(np.median(t_plan)), "tables_ms": float(np.median(t_tab)), "launch_ms": float(np.median(t_launch)),
                   "launch_ms_min": float(np.min(t_launch)), "call_dev_ms": float(np.median(t_dev)), "call_ms": float(np.median(t_call)),
                   "kernel_bytes": {"crop_write": 3 * px, "taps_read": 12 * px, "total": 15 * px}}
            med["launch_gb_per_s"] = med["kernel_bytes"]["total"] / (med["launch_ms"] * 1e-3) / 1e9
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/aligned_heads_bench.py --iters {a.iters} --warmup {a.warmup}: {H} x {W} image; ms are medians; launch = staging upload + warp_crops_kernel (HIP events)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
