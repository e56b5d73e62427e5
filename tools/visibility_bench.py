"""visibility.rasterize_heads(to_host=False) on a 12 MP canvas with 1, 16 and 100 heads whose vertices are already on the device, both occlusion modes,
with and without barycentric weights, beside the nearest thing this package had before: render_mesh on the same vertices (it paints a picture through
the same tile-major fold; nothing else here answers "which head owns this pixel").

    launch    HIP events around vghvis_rasterize_triangles: the fill of the background, the clears, the ONE staging upload (topology, tile lists) and the
              kernels (fill_kernel, boxes_kernel, tiles_kernel).  The kernels one by one and the NUMBER OF LAUNCHES come from a
              `rocprofv3 --kernel-trace --stats` run of this tool with one head count (--heads 100 --iters 3 --warmup 1 --no-render).
    call_dev  the whole rasterize_heads(to_host=False): allocating the outputs, the per-head bounds (one reduction on the device and its 4 n floats
              back), checks, launch; host clock around work that ends in a device synchronise.
    render_ms HIP events around vghv_render_meshes inside render_mesh(to_host=False) on the same vertices and topology, alternated with the new call in
              the same process: normals, shading and a blended picture instead of buffers, so a yardstick for scale and not an equal job.

Medians over --iters after --warmup; the head counts are measured twice, alternating, and the second round is reported.  The meshes are closed
ellipsoids of FLAME's size (5 002 vertices, 10 000 triangles), 100 .. 300 px across.

    python tools/visibility_bench.py [--iters 20] [--warmup 3] [--heads 1,16,100] [--out profiles/visibility.txt]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shade_ref as sr  # noqa: E402  (the ellipsoid generator of the tests)

from head_detector_amd import _lib_view, _lib_vis, mesh_render, visibility  # noqa: E402

H, W = 3000, 4000


class Timed:
    """Brackets one library call with events without changing the product's code path."""

    def __init__(self, lib, name, ev0, ev1, stream):
        self._lib, self._name, self._ev, self._stream = lib, name, (ev0, ev1), stream

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def timed(*args):
            self._ev[0].record(self._stream)
            rc = fn(*args)
            self._ev[1].record(self._stream)
            return rc

        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heads", default="1,16,100", help="head counts, comma separated (one count for a rocprofv3 run: its stats then belong to that count)")
    ap.add_argument("--no-render", action="store_true", help="leave the yardstick out (for a kernel trace of the new call alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("visibility_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    image_dev = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    unit, tri = sr.ellipsoid()
    cases = {}
    for n in (int(v) for v in a.heads.split(",")):
        verts = sr.ellipsoid_heads(np.random.default_rng(n), n, H, W, 100.0, 300.0, unit, spread=0.95)
        cases[n] = ([types.SimpleNamespace(vertices_3d=v) for v in verts], torch.from_numpy(verts).to(dev))
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    vis_lib, view_lib = _lib_vis.load(), _lib_view.load()
    vis_timed = Timed(vis_lib, "vghvis_rasterize_triangles", ev[0], ev[1], cur)
    view_timed = Timed(view_lib, "vghv_render_meshes", ev[2], ev[3], cur)
    variants = [(mode, bary) for mode in ("order", "depth") for bary in (True, False)]
    lines = []
    for rnd in range(2):
        for n, (heads, verts_dev) in cases.items():
            t_launch, t_dev, t_render = {v: [] for v in variants}, {v: [] for v in variants}, []
            res = {}
            for it in range(a.warmup + a.iters):
                for mode, bary in variants:
                    t1 = time.perf_counter()
                    visibility._lib_vis.load = lambda: vis_timed
                    try:
                        res[mode] = visibility.rasterize_heads(verts_dev, tri, H, W, occlusion=mode, z_sign=-1.0, barycentric=bary, to_host=False)
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                    finally:
                        visibility._lib_vis.load = lambda: vis_lib
                    if it >= a.warmup:
                        t_launch[(mode, bary)].append(ev[0].elapsed_time(ev[1])), t_dev[(mode, bary)].append((t2 - t1) * 1e3)
                if not a.no_render:
                    mesh_render._lib_view.load = lambda: view_timed
                    try:
                        mesh_render.render_mesh(image_dev, heads, tri, to_host=False)
                        torch.cuda.synchronize()
                    finally:
                        mesh_render._lib_view.load = lambda: view_lib
                    if it >= a.warmup:
                        t_render.append(ev[2].elapsed_time(ev[3]))
            bounds = mesh_render.pixel_bounds(verts_dev, tri, H, W)
            pairs = int(sum((b[2] // 16 - b[0] // 16 + 1) * (b[3] // 16 - b[1] // 16 + 1) for b in bounds if b[2] >= b[0] and b[3] >= b[1]))
            med = {"heads": n, "triangles": n * tri.shape[0], "tile_head_pairs": pairs, "covered_pixels": int(res["order"].covered_pixels.sum()),
                   "owned_pixels": int(res["order"].visible_pixels.sum())}
            for mode, bary in variants:
                key = f"{mode}{'' if bary else '_nobary'}"
                med[f"{key}_launch_ms"] = float(np.median(t_launch[(mode, bary)]))
                med[f"{key}_call_dev_ms"] = float(np.median(t_dev[(mode, bary)]))
            med["order_launch_ms_min"] = float(np.min(t_launch[("order", True)]))
            if t_render:
                med.update(render_ms=float(np.median(t_render)), render_over_order_launch=float(np.median(t_render) / np.median(t_launch[("order", True)])))
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/visibility_bench.py --iters {a.iters} --warmup {a.warmup}: rasterize_heads(to_host=False) on a {H} x {W} canvas, vertices on the device; ms are "
                    "medians; launch = background fill + clears + staging upload + boxes and tiles kernels (HIP events); render_ms = vghv_render_meshes on the same vertices\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
