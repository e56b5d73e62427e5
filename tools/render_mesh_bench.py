"""PredictionResult.render_mesh(to_host=False) on a 12 MP photograph that is already on the device, with 1, 16 and 100 heads, beside the only other way
this package has to paint n meshes on the device: PNCCProcessor.render (vgh_pncc_render: two launches per head, the second over the whole image).

    launch    HIP events around vghv_render_meshes: the image copy, the ONE staging upload (topology, incidence lists, tile lists) and the kernels
              (normals_kernel, boxes_kernel, tiles_kernel).  The kernels one by one and the NUMBER OF LAUNCHES come from a
              `rocprofv3 --kernel-trace --stats` run of this tool with one head count (--heads 100 --iters 3 --warmup 1).
    call_dev  the whole render_mesh(to_host=False): stacking and uploading the vertices, the per-head bounds (one reduction on the device and its 4 n
              floats back), checks, launch; host clock around work that ends in a device synchronise.
    pncc_ms   HIP events around PNCCProcessor.render on the same vertices and topology (vertices already on the device), alternated with the new call
              in the same process.  It paints opaque colour codes on black, the new call lights and blends over the photograph: the comparison is of
              "n meshes rasterised on the device", not of equal pictures.

Medians over --iters after --warmup; the head counts are measured twice, alternating, and the second round is reported.  The meshes are closed
ellipsoids of FLAME's size (5 002 vertices, 10 000 triangles), 100 .. 300 px across.

    python tools/render_mesh_bench.py [--iters 20] [--warmup 3] [--heads 1,16,100] [--out profiles/render_mesh.txt]
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

from head_detector_amd import _lib_view, mesh_render  # noqa: E402
from head_detector_amd.pncc import MeshAssets, PNCCProcessor  # noqa: E402

H, W = 3000, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heads", default="1,16,100", help="head counts, comma separated (one count for a rocprofv3 run: its stats then belong to that count)")
    ap.add_argument("--no-pncc", action="store_true", help="leave the yardstick out (for a kernel trace of the new call alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_mesh_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    image_dev = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    unit, tri = sr.ellipsoid()
    V = unit.shape[0]
    pncc = PNCCProcessor(MeshAssets(tri, unit, np.arange(V)))  # every triangle kept, colour codes of the unit sphere
    cases = {}
    for n in (int(v) for v in a.heads.split(",")):
        verts = sr.ellipsoid_heads(np.random.default_rng(n), n, H, W, 100.0, 300.0, unit, spread=0.95)
        cases[n] = ([types.SimpleNamespace(vertices_3d=v) for v in verts], torch.from_numpy(verts).to(dev))
    cur = torch.cuda.current_stream(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    lib = _lib_view.load()
    real = lib.vghv_render_meshes

    class Timed:  # brackets the library call with events without changing the product's code path
        def vghv_render_meshes(self, *args):
            ev[0].record(cur)
            rc = real(*args)
            ev[1].record(cur)
            return rc

        def __getattr__(self, name):
            return getattr(lib, name)

    lines = []
    for rnd in range(2):
        for n, (heads, verts_dev) in cases.items():
            t_launch, t_dev, t_pncc = [], [], []
            for it in range(a.warmup + a.iters):
                t1 = time.perf_counter()
                mesh_render._lib_view.load = lambda: Timed()
                try:
                    out = mesh_render.render_mesh(image_dev, heads, tri, to_host=False)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                finally:
                    mesh_render._lib_view.load = lambda: lib
                if not a.no_pncc:
                    ev[2].record(cur)
                    pncc.render((H, W, 3), verts_dev)
                    ev[3].record(cur)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t_launch.append(ev[0].elapsed_time(ev[1])), t_dev.append((t2 - t1) * 1e3)
                    if not a.no_pncc:
                        t_pncc.append(ev[2].elapsed_time(ev[3]))
            painted = int((out != image_dev).any(dim=2).sum())
            bounds = mesh_render.pixel_bounds(verts_dev, tri, H, W)
            pairs = int(sum((b[2] // 16 - b[0] // 16 + 1) * (b[3] // 16 - b[1] // 16 + 1) for b in bounds if b[2] >= b[0] and b[3] >= b[1]))
            med = {"heads": n, "triangles": n * tri.shape[0], "tile_head_pairs": pairs, "painted_pixels": painted, "launch_ms": float(np.median(t_launch)),
                   "launch_ms_min": float(np.min(t_launch)), "call_dev_ms": float(np.median(t_dev))}
            if t_pncc:
                med.update(pncc_ms=float(np.median(t_pncc)), pncc_over_launch=float(np.median(t_pncc) / np.median(t_launch)))
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/render_mesh_bench.py --iters {a.iters} --warmup {a.warmup}: render_mesh(to_host=False) on a {H} x {W} image on the device; ms are medians; "
                    "launch = image copy + staging upload + normals, boxes and tiles kernels (HIP events); pncc_ms = PNCCProcessor.render on the same vertices\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
