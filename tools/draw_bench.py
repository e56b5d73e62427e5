"""PredictionResult.draw("full") on a 12 MP photograph that is already on the device, with 1, 16 and 100 heads: where the time of a call goes.

    plan      draw.draw_plan: truncation, range checks, boxes, radius and circle table (host clock)
    launch    HIP events around vghv_draw_heads: the ONE staging upload (points, boxes, topology), the clear of the key plane, the three stamp
              kernels and the resolve kernel.  The kernels one by one come from a `rocprofv3 --kernel-trace --stats` run of this tool
              (stamp_boxes_kernel, stamp_wire_kernel, stamp_dots_kernel, resolve_kernel and the fill kernel of hipMemsetAsync).
    call_dev  the whole draw(to_host=False): plan, argument checks and copies into the pinned block, launch; host clock around work that ends in a
              device synchronise.

The yardstick of the resolve pass is printed beside it: the bytes it moves (4 B of key + 3 B of source + 3 B of destination per pixel) divided by
the bandwidth of a torch device-to-device copy of the same image measured in the same run (bytes read + bytes written over its HIP-event time).
Medians over --iters after --warmup; the head counts are measured twice, alternating, and the second round is reported.

The meshes are synthetic: 5023 vertices on a jittered grid, 4816 triangles over neighbouring vertices (edges of about 1/70 of the head), 2470 dots:
the primitive counts of the reference's "full" view.

    python tools/draw_bench.py [--iters 30] [--warmup 5] [--heads 1,16,100] [--out profiles/draw_heads.txt]
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

from head_detector_amd import _lib_view, draw  # noqa: E402
from head_detector_amd.head_info import Bbox  # noqa: E402

H, W, V, T, K, COLS = 3000, 4000, 5023, 4816, 2470, 71


def topology(rng):
    i = rng.integers(0, V - COLS - 1, T)
    tri = np.stack([i, i + 1, i + COLS + rng.integers(-1, 2, T)], axis=1).astype(np.int32)
    return tri, np.sort(rng.choice(V, K, replace=False))


def heads_on_photo(rng, n):
    """Heads the size a crowd photograph has them (120 .. 440 px across), inside the image, overlapping freely."""
    k = np.arange(V)
    row, col = k // COLS, k % COLS
    col = np.where(row % 2 == 1, COLS - 1 - col, col)
    out = []
    for _ in range(n):
        size, cx, cy = rng.uniform(120, 440), rng.uniform(250, W - 250), rng.uniform(300, H - 300)
        u = (col + rng.uniform(-0.4, 0.4, V)) / (COLS - 1) - 0.5
        v = (row + rng.uniform(-0.4, 0.4, V)) / (COLS - 1) - 0.5
        xyz = np.stack([cx + size * u, cy + 1.2 * size * v, rng.normal(0, 20, V)], axis=1).astype(np.float32)
        x0, y0, x1, y1 = (int(q) for q in (xyz[:, 0].min(), xyz[:, 1].min(), xyz[:, 0].max(), xyz[:, 1].max()))
        out.append(types.SimpleNamespace(vertices_3d=xyz, bbox=Bbox(x0, y0, x1 - x0, y1 - y0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--heads", default="1,16,100", help="head counts, comma separated (one count for a rocprofv3 run: its stats then belong to that count)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("draw_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    image_dev = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    tri, hidx = topology(rng)
    assets = dict(triangles=tri, head_indices=hidx)
    cases = {n: heads_on_photo(np.random.default_rng(n), n) for n in (int(v) for v in a.heads.split(","))}
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    lib = _lib_view.load()
    real = lib.vghv_draw_heads

    class Timed:  # brackets the library call with events without changing the product's code path
        def vghv_draw_heads(self, *args):
            ev[0].record(cur)
            rc = real(*args)
            ev[1].record(cur)
            return rc

        def __getattr__(self, name):
            return getattr(lib, name)

    lines = []
    scratch = torch.empty_like(image_dev)
    for rnd in range(2):
        for n, heads in cases.items():
            t_plan, t_launch, t_dev, t_copy = [], [], [], []
            for it in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                draw.draw_plan(image_dev.shape, heads, "full", **assets)
                t1 = time.perf_counter()
                draw._lib_view.load = lambda: Timed()
                try:
                    out = draw.draw_heads(image_dev, heads, "full", to_host=False, **assets)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                finally:
                    draw._lib_view.load = lambda: lib
                ev[2].record(cur)
                scratch.copy_(image_dev)
                ev[3].record(cur)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t_plan.append((t1 - t0) * 1e3), t_launch.append(ev[0].elapsed_time(ev[1])), t_dev.append((t2 - t1) * 1e3), t_copy.append(ev[2].elapsed_time(ev[3]))
            painted = int((out != image_dev).any(dim=2).sum())
            copy_ms = float(np.median(t_copy))
            copy_gbs = 2 * 3 * H * W / (copy_ms * 1e-3) / 1e9
            med = {"heads": n, "segments": n * T * 3, "dots": n * K, "painted_pixels": painted, "plan_ms": float(np.median(t_plan)), "launch_ms": float(np.median(t_launch)),
                   "launch_ms_min": float(np.min(t_launch)), "call_dev_ms": float(np.median(t_dev)), "d2d_copy_ms": copy_ms, "d2d_copy_gb_per_s": copy_gbs,
                   "resolve_bytes": 10 * H * W, "resolve_yardstick_ms": 10 * H * W / (copy_gbs * 1e9) * 1e3}
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/draw_bench.py --iters {a.iters} --warmup {a.warmup}: draw(\"full\", to_host=False) on a {H} x {W} image on the device; ms are medians; "
                    "launch = staging upload + key-plane clear + stamp kernels + resolve (HIP events); resolve_yardstick_ms = resolve_bytes / d2d_copy_gb_per_s\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
