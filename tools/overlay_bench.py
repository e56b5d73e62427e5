"""Boxes and track labels in the planes of a video frame: ``overlay.draw_heads`` on seeded NV12 surfaces at 1920 x 1080 and 3840 x 2160 with 1, 16 and 100
tracked heads of 200 x 240 pixels and ``"id+score"`` labels, IN PLACE, ALTERNATED in one process with the only route to an annotated stream that existed before
it: ``frame.to_rgb()`` + ``draw("bbox", to_host=False)`` + ``YUV420Frame.from_rgb``.  That route draws the reference's boxes and NO labels: the two routes do
not paint the same picture, the old one paints less.

    ms       median of HIP-event times around one whole call of each route (the Python plan, the workspace allocation, the staging upload and every launch
             inside), after warm-up; the routes take turns inside every iteration, each being the first after the synchronise in turn.  ``render_only`` is the
             in-place call on items planned beforehand: what is left of a call without ``head_overlay_plan``
    bytes    what the passes of each route must move at least, computed from the shapes (``overlay_bytes`` / ``rgb_bytes``); the torch passes of ``to_rgb`` move
             more than the one read and one write counted for them

Nothing here is a pass criterion and no test asserts a time.  The in-place result is compared bitwise with the out-of-place one before anything is timed.

    python tools/overlay_bench.py [--iters 20] [--warmup 3] [--out profiles/overlay.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from head_detector_amd import draw, overlay  # noqa: E402
from head_detector_amd.head_info import Bbox, HeadMetadata  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

SIZES = ((1080, 1920), (2160, 3840))
ROUTES = ("in_place", "render_only", "rgb_round_trip")


def make_heads(n, H, W, seed):
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n * W / H)))
    rows = int(np.ceil(n / cols))
    heads = []
    for k in range(n):
        cx = (k % cols + 0.5) * W / cols + rng.integers(-60, 61)
        cy = (k // cols + 0.5) * H / rows + rng.integers(-60, 61)
        heads.append(HeadMetadata(Bbox(int(cx - 100), int(cy - 120), 200, 240), float(rng.uniform(0.3, 1.0)), None, np.zeros((1, 3), np.float32), None))  # (draw() reads vertices)
    return heads, rng.permutation(4 * n)[:n].astype(np.int64)


def overlay_bytes(items, H, W):
    """Least bytes of ``overlay.render`` in place, an upper bound per item (every position of its grown, clipped box counted as covered and owned): the staging
    upload, the key clear (4 g), the paint (4 g), the two write passes' key reads (4 g each) and the samples read and written (2 * 1.5 g)."""
    rows = items.rows()
    g = tiles = 0
    for x0, y0, x1, y1 in zip(rows["x0"].tolist(), rows["y0"].tolist(), rows["x1"].tolist(), rows["y1"].tolist()):
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if cx1 <= cx0 or cy1 <= cy0:
            continue
        gx0, gy0, gx1, gy1 = cx0 & ~1, cy0 & ~1, min((cx1 + 1) & ~1, W), min((cy1 + 1) & ~1, H)
        g += (gx1 - gx0) * (gy1 - gy0)
        tiles += -(-(gx1 - gx0) // 16) * -(-(gy1 - gy0) // 16)
    return {"upload": 44 * len(rows) + len(items.codes()) + 308 + 8 * tiles, "clear": 4 * g, "paint": 4 * g, "write": 8 * g + 3 * g}


def rgb_bytes(heads, H, W):
    """Least bytes of the RGB round trip: one read of the planes and one write of the image for ``to_rgb``, the copy of the image and the box outlines for
    ``draw("bbox")``, one read of the image and one write of the planes for ``from_rgb``."""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    planes = H * W + 2 * CH * CW
    return {"to_rgb": planes + 3 * H * W, "draw": 2 * 3 * H * W + sum(3 * 2 * 2 * (h.bbox.w + h.bbox.h) for h in heads), "from_rgb": 3 * H * W + planes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for H, W in SIZES:
        surface = torch.from_numpy(np.random.default_rng(H).integers(0, 256, W * H * 3 // 2, dtype=np.uint8)).to(dev)
        keep = surface.clone()
        frame = YUV420Frame.from_nv12(surface, H, W, pitch=W)
        out_frame = YUV420Frame.empty(H, W, "nv12", dev)
        packed = YUV420Frame.empty(H, W, "nv12", dev)
        for n in (1, 16, 100):
            heads, ids = make_heads(n, H, W, seed=n)
            kw = dict(labels="id+score", track_ids=ids)
            planned = overlay.head_overlay_plan((H, W), heads, **kw)
            routes = {
                "in_place": lambda: overlay.draw_heads(frame, heads, out=frame, **kw),
                "render_only": lambda: overlay.render(frame, planned, out=frame),  # the same call without head_overlay_plan: the colour conversion, the rows and the library
                "rgb_round_trip": lambda: YUV420Frame.from_rgb(draw.draw_heads(frame.to_rgb(), heads, "bbox", to_host=False), out=packed),
            }
            # in place = out of place, on the untouched surface, before anything is timed
            surface.copy_(keep)
            overlay.draw_heads(frame, heads, out=out_frame, **kw)
            routes["in_place"]()
            torch.cuda.synchronize()
            same = all(torch.equal(p, q) for p, q in zip(frame.planes, out_frame.planes))
            assert same, f"{H} x {W}, {n} heads: in place differs from out of place"
            changed = int((surface != keep).sum())
            surface.copy_(keep)
            ev = {r: [torch.cuda.Event(enable_timing=True) for _ in range(2)] for r in ROUTES}
            ms = {r: [] for r in ROUTES}
            for it in range(a.warmup + a.iters):
                for r in ROUTES[it % 3:] + ROUTES[:it % 3]:  # the routes take turns, and take turns at being the first after the synchronise
                    ev[r][0].record(stream)
                    routes[r]()
                    ev[r][1].record(stream)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    for r in ROUTES:
                        ms[r].append(ev[r][0].elapsed_time(ev[r][1]))
            items = overlay.head_overlay_plan((H, W), heads, **kw)
            line = {"frame": f"{W}x{H}", "heads": n, "items": len(items), "labels": "id+score", "in_place_equals_out_of_place": same, "bytes_changed": changed}
            for r in ROUTES:
                line[f"{r}_ms"] = round(float(np.median(ms[r])), 4)
            line["in_place_bytes"] = overlay_bytes(items, H, W)
            line["rgb_round_trip_bytes"] = rgb_bytes(heads, H, W)
            for r in ("in_place", "rgb_round_trip"):
                line[f"{r}_MB"] = round(sum(line[f"{r}_bytes"].values()) / 1e6, 3)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/overlay_bench.py --iters {a.iters} --warmup {a.warmup}: overlay.draw_heads (boxes + 'id+score' label bars and text, API-default thickness and scale) "
                    "IN PLACE on seeded dense NV12 surfaces, device-resident, tracked heads of 200 x 240 pixels; *_ms = median of HIP-event times around one whole call of each "
                    "route, the routes alternating inside every iteration; render_only = overlay.render in place on items planned beforehand; rgb_round_trip = frame.to_rgb() + draw('bbox', to_host=False) + YUV420Frame.from_rgb back to NV12, "
                    "which draws boxes and NO labels; *_bytes = the least each pass must move, from the shapes\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
