"""Heads hidden in the planes of a video frame: ``video.anonymize_frame`` on seeded NV12 surfaces at 1920 x 1080 and 3840 x 2160 with 1, 16 and 100 heads of
200 x 240 pixels, three methods x box / ellipse, in place and out of place, ALTERNATED in one process with the route that existed before it -- the RGB copy
``frame.to_rgb()`` + ``anonymize.anonymize_heads`` on that copy -- and with that route plus ``YUV420Frame.from_rgb``, the full round trip back to NV12.

    ms       median of HIP-event times around one whole call of each route (plans, workspace allocation, the upload of the head rows and every launch inside),
             after warm-up; the four routes take turns inside every iteration, each being the first after the synchronise in turn, so that what else the machine does
             and the idle queue's wake-up fall on all of them alike.  With boxes of this size a call is short: much of it is the host half (the Python plan)
    bytes    what the stages of each route must move at least, computed from the shapes (``frame_bytes`` / ``rgb_bytes``); the torch passes of ``to_rgb`` move
             more than the one read and one write counted for them

Nothing here is a pass criterion and no test asserts a time.  The in-place result is compared bitwise with the out-of-place one before anything is timed.

    python tools/yuv_anonymize_bench.py [--iters 20] [--warmup 3] [--out profiles/yuv_anonymize.txt]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from head_detector_amd import anonymize, video  # noqa: E402
from head_detector_amd.head_info import Bbox  # noqa: E402
from head_detector_amd.video import YUV420Frame  # noqa: E402

SIZES = ((1080, 1920), (2160, 3840))
ROUTES = ("in_place", "out_of_place", "rgb_route", "rgb_round_trip")


def make_heads(n, H, W, seed):
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n * W / H)))
    rows = int(np.ceil(n / cols))
    heads = []
    for k in range(n):
        cx = (k % cols + 0.5) * W / cols + rng.integers(-60, 61)
        cy = (k // cols + 0.5) * H / rows + rng.integers(-60, 61)
        heads.append(types.SimpleNamespace(bbox=Bbox(int(cx - 100), int(cy - 120), 200, 240)))
    return heads


def _clipped(boxes, W, H, radii=None):
    """(sum of the clipped areas, sum of the areas extended by r rows up and down and clamped)."""
    area = rows = 0
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if cx1 <= cx0 or cy1 <= cy0:
            continue
        area += (cx1 - cx0) * (cy1 - cy0)
        r = radii[i] if radii is not None else 0
        rows += (min(cy1 + r, H) - max(cy0 - r, 0)) * (cx1 - cx0)
    return area, rows


def frame_bytes(plan_rows, chroma_rows, H, W, method, in_place):
    """Least bytes per stage of ``anonymize_frame``: the clear and the painting of the owner plane, the value passes, the write pass (an upper bound: every sample
    of every clipped box counted as owned), and for a frame out of place the copy of the three planes."""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    lb, cb = [tuple(r)[:4] for r in plan_rows.tolist()], [tuple(r)[:4] for r in chroma_rows.tolist()]
    la, lrows = _clipped(lb, W, H, plan_rows["radius"].tolist())
    ca, crows = _clipped(cb, CW, CH, chroma_rows["radius"].tolist())
    out = {"owner": 4 * H * W + 4 * la, "write": 4 * la + 16 * ca + la + 2 * ca}
    if method == "pixelate":
        out["cells"] = la + 2 * ca
        out["write"] += la + 2 * ca
    if method == "blur":
        out["blur_rows"] = (1 + 2) * lrows + (2 + 4) * crows
        out["blur_cols"] = 2 * lrows + 4 * crows + la + 2 * ca + 4 * la + 16 * ca
        out["write"] += la + 2 * ca
    if not in_place:
        out["copy"] = 2 * (H * W + 2 * CH * CW)
    return out


def rgb_bytes(plan_rows, H, W, method, round_trip):
    """Least bytes of the RGB route: one read of the planes and one write of the image for ``to_rgb`` (its torch passes move more), the stages of
    ``anonymize_heads`` as tools/anonymize_bench.py counts them, and for the round trip one read of the image and one write of the planes."""
    CH, CW = (H + 1) // 2, (W + 1) // 2
    area, rows = _clipped([tuple(r)[:4] for r in plan_rows.tolist()], W, H, plan_rows["radius"].tolist())
    out = {"to_rgb": H * W + 2 * CH * CW + 3 * H * W, "owner": 4 * H * W + 4 * area, "resolve": H * W * (3 + 4 + 3)}
    if method == "pixelate":
        out["cells"] = 3 * area
        out["resolve"] += 4 * area
    if method == "blur":
        out["blur_rows"] = (3 + 6) * rows
        out["blur_cols"] = 6 * rows + 4 * area
        out["resolve"] += 4 * area
    if round_trip:
        out["from_rgb"] = 3 * H * W + H * W + 2 * CH * CW
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_anonymize_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for H, W in SIZES:
        pitch = W
        surface = torch.from_numpy(np.random.default_rng(H).integers(0, 256, pitch * H * 3 // 2, dtype=np.uint8)).to(dev)
        keep = surface.clone()
        frame = YUV420Frame.from_nv12(surface, H, W, pitch=pitch)
        out_frame = YUV420Frame.empty(H, W, "nv12", dev)
        packed = YUV420Frame.empty(H, W, "nv12", dev)
        rgb_out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        for n in (1, 16, 100):
            heads = make_heads(n, H, W, seed=n)
            for region in ("box", "ellipse"):
                for method in ("fill", "pixelate", "blur"):
                    kw = dict(color=(16, 16, 16))
                    routes = {
                        "in_place": lambda: video.anonymize_frame(frame, heads, method, region, out=frame, **kw),
                        "out_of_place": lambda: video.anonymize_frame(frame, heads, method, region, out=out_frame, **kw),
                        "rgb_route": lambda: anonymize.anonymize_heads(frame.to_rgb(), heads, method, region, out=rgb_out, to_host=False, **kw),
                        "rgb_round_trip": lambda: YUV420Frame.from_rgb(anonymize.anonymize_heads(frame.to_rgb(), heads, method, region, out=rgb_out, to_host=False, **kw), out=packed),
                    }
                    # in place = out of place, on the untouched surface, before anything is timed
                    surface.copy_(keep)
                    routes["out_of_place"]()
                    routes["in_place"]()
                    torch.cuda.synchronize()
                    same = all(torch.equal(p, q) for p, q in zip(frame.planes, out_frame.planes))
                    assert same, f"{H} x {W}, {n} heads, {region}, {method}: in place differs from out of place"
                    surface.copy_(keep)
                    ev = {r: [torch.cuda.Event(enable_timing=True) for _ in range(2)] for r in ROUTES}
                    ms = {r: [] for r in ROUTES}
                    for it in range(a.warmup + a.iters):
                        for r in ROUTES[it % 4:] + ROUTES[:it % 4]:  # the routes take turns, and take turns at being the first after the synchronise
                            ev[r][0].record(stream)
                            routes[r]()
                            ev[r][1].record(stream)
                        torch.cuda.synchronize()
                        if it >= a.warmup:
                            for r in ROUTES:
                                ms[r].append(ev[r][0].elapsed_time(ev[r][1]))
                    plan = anonymize.anonymize_plan((H, W), heads, method, region)
                    chroma, _ = anonymize.plan_rows([video.chroma_box(tuple(q)[:4]) for q in plan.heads.tolist()], method, 8, 0.1, anonymize.TapTables())
                    line = {"frame": f"{W}x{H}", "heads": n, "region": region, "method": method, "in_place_equals_out_of_place": same}
                    for r in ROUTES:
                        line[f"{r}_ms"] = round(float(np.median(ms[r])), 4)
                    line["in_place_bytes"] = frame_bytes(plan.heads, chroma, H, W, method, True)
                    line["out_of_place_bytes"] = frame_bytes(plan.heads, chroma, H, W, method, False)
                    line["rgb_route_bytes"] = rgb_bytes(plan.heads, H, W, method, False)
                    line["rgb_round_trip_bytes"] = rgb_bytes(plan.heads, H, W, method, True)
                    for r in ROUTES:
                        line[f"{r}_MB"] = round(sum(line[f"{r}_bytes"].values()) / 1e6, 2)
                    lines.append(json.dumps(line))
                    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/yuv_anonymize_bench.py --iters {a.iters} --warmup {a.warmup}: video.anonymize_frame on seeded dense NV12 surfaces, device-resident, heads of 200 x 240 pixels "
                    "(margin 0.1); *_ms = median of HIP-event times around one whole call of each route, the four routes alternating inside every iteration; rgb_route = "
                    "frame.to_rgb() + anonymize_heads on that copy, rgb_round_trip = that + YUV420Frame.from_rgb back to NV12; *_bytes = the least each stage must move, from the shapes\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
