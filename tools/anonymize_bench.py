"""Head anonymisation: ``anonymize.anonymize_heads`` on a seeded 12-megapixel image (3000 x 4000) with 1, 16 and 100 heads, three methods x box / ellipse / mesh,
on device-resident inputs, beside the NumPy restatement (tests/anonymize_ref.py) on this machine's CPU.

    ms            median of HIP-event times around one call (the plan, the workspace allocation, the upload of the head rows and every launch are inside)
    bytes         what the stages of that call must move, computed from the shapes (see ``stage_bytes``); GB/s = their sum over ms, an end-to-end figure
    cpu_ms        one run of the restatement; the device result is compared BITWISE with it.  The restatement blurs the whole image once per tap table, which
                  takes minutes at this size, so for "blur" it runs only with --cpu-blur (otherwise cpu_ms is null and the check is the test suite's)

Heads are 200 x 240 pixel boxes on a jittered grid, so that neighbours overlap; a head's mesh is a 9 x 9 grid sheet bulging over its box's ellipse.

    python tools/anonymize_bench.py [--iters 20] [--warmup 3] [--cpu-blur] [--out profiles/anonymize.txt]
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

import anonymize_ref as ref  # noqa: E402

from head_detector_amd import anonymize, visibility  # noqa: E402
from head_detector_amd.head_info import Bbox  # noqa: E402

H, W = 3000, 4000
SIDE = 9


def sheet_triangles():
    tri = []
    for j in range(SIDE - 1):
        for i in range(SIDE - 1):
            a = j * SIDE + i
            tri += [(a, a + 1, a + SIDE), (a + 1, a + SIDE + 1, a + SIDE)]
    return np.array(tri, dtype=np.int32)


def make_heads(n, seed):
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n * W / H)))
    rows = int(np.ceil(n / cols))
    u, v = np.meshgrid(np.linspace(-1, 1, SIDE), np.linspace(-1, 1, SIDE))
    heads = []
    for k in range(n):
        cx = (k % cols + 0.5) * W / cols + rng.integers(-60, 61)
        cy = (k // cols + 0.5) * H / rows + rng.integers(-60, 61)
        x, y, w, h = int(cx - 100), int(cy - 120), 200, 240
        # the square [-1, 1]^2 mapped onto the disc, scaled to the box: a sheet whose silhouette is the box's ellipse
        px, py = cx + 100 * u * np.sqrt(1 - v * v / 2), cy + 120 * v * np.sqrt(1 - u * u / 2)
        pz = 80 * (1 - (u * u + v * v) / 2)
        heads.append(types.SimpleNamespace(bbox=Bbox(x, y, w, h), vertices_3d=np.stack([px, py, pz], axis=-1).reshape(-1, 3).astype(np.float32)))
    return heads


def stage_bytes(boxes, owner, method, radii):
    """Bytes each stage must move for these geometry boxes (clipped to the image) and this owner map."""
    out = {"resolve": H * W * (3 + 4 + 3)}
    clipped = [(max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)) for x0, y0, x1, y1 in boxes]
    area = [max(0, x1 - x0) * max(0, y1 - y0) for x0, y0, x1, y1 in clipped]
    out["owner"] = 4 * H * W + 4 * sum(area)  # the clear and one atomic per pixel of every clipped box (a caller's map: produced elsewhere)
    if method == "pixelate":
        out["cells"] = 3 * sum(area)
        out["resolve"] += 4 * int((owner >= 0).sum())
    if method == "blur":
        rows = [max(0, min(y1 + r, H) - max(y0 - r, 0)) * max(0, x1 - x0) for (x0, y0, x1, y1), r in zip(clipped, radii)]
        out["blur_rows"] = (3 + 6) * sum(rows)
        out["blur_cols"] = 6 * sum(rows) + 4 * int((owner >= 0).sum())
        out["resolve"] += 4 * int((owner >= 0).sum())
    return out


def median_ms(fn, stream, warmup, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for it in range(warmup + iters):
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        ev[1].synchronize()
        if it >= warmup:
            out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-blur", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anonymize_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    image = np.random.default_rng(12).integers(0, 256, (H, W, 3), dtype=np.uint8)
    src = torch.from_numpy(image).to(dev)
    out = torch.empty_like(src)
    faces = sheet_triangles()
    lines = []
    for n in (1, 16, 100):
        heads = make_heads(n, seed=n)
        silhouettes = visibility.head_visibility(heads, faces, H, W, occlusion="order", barycentric=False).head_index
        for region in ("box", "ellipse", "mesh"):
            if region == "mesh":
                boxes, owner = [ref.mesh_box(h.vertices_3d, faces, H, W) for h in heads], silhouettes
            else:
                boxes = [ref.geometry_box(h.bbox, 0.1) for h in heads]
                t0 = time.perf_counter()
                owner = ref.owner_map(H, W, boxes, region)
                owner_cpu_ms = (time.perf_counter() - t0) * 1e3
            for method in ("fill", "pixelate", "blur"):
                def call():
                    anonymize.anonymize_heads(src, heads, method, region, faces=faces, color=(16, 16, 16), out=out, to_host=False)

                call()
                torch.cuda.synchronize()
                tables = [ref.taps(*ref.blur_radius(b, 0.1)) for b in boxes]
                line = {"heads": n, "region": region, "method": method, "cpu_ms": None, "bitwise_equal": None}
                if method != "blur" or a.cpu_blur:
                    t0 = time.perf_counter()
                    want = ref.render(image, boxes, owner, method, cell=[ref.cell_side(b, 8) for b in boxes], tap_tables=tables, color=(16, 16, 16))
                    line["cpu_ms"] = (time.perf_counter() - t0) * 1e3 + (owner_cpu_ms if region != "mesh" else 0.0)
                    line["bitwise_equal"] = bool(np.array_equal(out.cpu().numpy(), want))
                    assert line["bitwise_equal"], f"{n} heads, {region}, {method}: the device differs from the restatement"
                line["ms"] = median_ms(call, stream, a.warmup, a.iters)
                line["bytes"] = stage_bytes(boxes, owner, method, [len(t) - 1 for t in tables])
                line["GB/s"] = sum(line["bytes"].values()) / line["ms"] / 1e6
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/anonymize_bench.py --iters {a.iters} --warmup {a.warmup}{' --cpu-blur' if a.cpu_blur else ''}: anonymize_heads on a seeded {H} x {W} image, device-resident "
                    "source and destination; ms = median of HIP-event times around one whole call (region=mesh includes the visibility pass); bytes = what each stage must "
                    "move, from the shapes; cpu_ms = one run of the NumPy restatement on the CPU\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
