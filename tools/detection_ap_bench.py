"""COCO-style detection AP at the size of WIDER val: a seeded synthetic set of 3 226 images with a long-tailed number of ground truths per image (a few
images near 2 000, most below 20) and up to 1 000 detections per image, evaluated on the device (csrc/detection_ap.hip, libvgheval.so) beside the NumPy
float64 restatement (tests/detection_ap_ref.py) on this machine's CPU.

    match       HIP events around vghev_box_match alone: the two memsets and match_kernel (ranks, staging, the T x A greedy matchings of every image).
    accumulate  HIP events around vghev_pr_accumulate alone: the bitonic sort of the kept detections and curve_kernel (T x A x M curves).
                Boxes, offsets, thresholds, outputs and scratch are on the device before the first event.
    cpu         the restatement on a SUB-SAMPLE (every --stride-th image, the largest image included), host clock, one run: it is a per-image Python
                loop and the whole set would take minutes.  The device evaluates the same sub-sample (sub_match_ms, sub_accumulate_ms), and
                cpu_x = cpu_ms / (sub_match_ms + sub_accumulate_ms) compares the two on that same set.  Before anything is timed the device's match
                arrays, curves and stats of the sub-sample are compared BITWISE with the restatement's.
    pairs/s     detection x ground-truth pairs of the kept detections times T x A matchings, over the match time: what the walk visits at most (a
                matching skips the ignored ground truths once it has a match).

Medians over --iters after --warmup; the full set and the sub-sample are measured twice, alternating, and the second round is reported.

    python tools/detection_ap_bench.py [--iters 10] [--warmup 2] [--images 3226] [--stride 50] [--max-dets 1,10,1000] [--out profiles/detection_ap.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detection_ap_ref as ref  # noqa: E402

from head_detector_amd import _lib_eval  # noqa: E402
from head_detector_amd import detection_metrics as dm  # noqa: E402


def synthetic_set(n_images, seed=0):
    """-> (detections, ground_truth): float boxes in a 1024 x 768 frame; scores are float32 values, so some tie."""
    rng = np.random.default_rng(seed)
    counts = np.minimum(np.floor(np.exp(rng.normal(1.5, 1.3, n_images))).astype(np.int64), 2000)
    for at, n in zip(rng.choice(n_images, min(6, n_images), replace=False), (1968, 1500, 1000, 700, 513, 512)):  # the tail: crowds
        counts[at] = n
    detections, ground_truth = [], []
    for ng in counts:
        side = np.exp(rng.normal(3.0 if ng < 100 else 2.3, 0.7, ng))
        gt = np.stack([rng.uniform(0, 1024, ng), rng.uniform(0, 768, ng), side, side * rng.uniform(1.0, 1.4, ng)], axis=1).reshape(ng, 4)
        found = gt[rng.random(ng) < 0.85]
        hits = found + np.concatenate([rng.normal(0, 0.08, (len(found), 2)) * found[:, 2:], rng.normal(0, 0.08, (len(found), 2)) * found[:, 2:]], axis=1)
        n_false = int(min(1000 - min(len(hits), 1000), rng.poisson(40) + ng // 2))
        fside = np.exp(rng.normal(2.8, 0.8, n_false))
        false = np.stack([rng.uniform(0, 1024, n_false), rng.uniform(0, 768, n_false), fside, fside * 1.2], axis=1).reshape(n_false, 4)
        boxes = np.concatenate([hits[:1000], false])
        score = np.concatenate([rng.beta(5, 2, len(hits[:1000])), rng.beta(1, 6, n_false) * 0.6 + 0.01]).astype(np.float32).astype(np.float64)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], 1.0)
        order = rng.permutation(len(boxes))
        detections.append(np.concatenate([boxes, score[:, None]], axis=1)[order])
        ground_truth.append(gt)
    return detections, ground_truth


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


class DeviceRun:
    """Everything of one set on the device, and the two launches."""

    def __init__(self, detections, ground_truth, options, dev, stream):
        self.iou_thrs, self.rec_thrs, self.area_ranges, self.max_dets = dm.check_ap_arguments(**options)
        self.boxes = dm._BoxSet(detections, ground_truth)
        self.job_m, self.m, self.kept_offset, self.hold_m = dm.match_job(self.boxes, self.iou_thrs, self.area_ranges, self.max_dets[-1], dev)
        self.n_kept = int(self.kept_offset[-1])
        self.job_p, self.precision, self.scores, self.recall, self.hold_p = dm.pr_job(self.m, self.n_kept, len(self.iou_thrs), self.rec_thrs, len(self.area_ranges),
                                                                                      self.max_dets, dev)
        self.lib, self.stream = _lib_eval.load(), stream
        counts_d, counts_g = np.minimum(np.diff(self.boxes.dt_offset), self.max_dets[-1]), np.diff(self.boxes.gt_offset)
        self.pairs = int((counts_d * counts_g).sum()) * len(self.iou_thrs) * len(self.area_ranges)

    def match(self):
        _lib_eval.check(self.lib.vghev_box_match(self.job_m, self.stream.cuda_stream))

    def accumulate(self):
        _lib_eval.check(self.lib.vghev_pr_accumulate(self.job_p, self.stream.cuda_stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--stride", type=int, default=50, help="the CPU restatement runs on every stride-th image")
    ap.add_argument("--max-dets", default="1,10,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detection_ap_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    options = {"max_dets": tuple(int(v) for v in a.max_dets.split(","))}
    detections, ground_truth = synthetic_set(a.images)
    largest = int(np.argmax([len(g) for g in ground_truth]))
    pick = sorted(set(range(0, a.images, a.stride)) | {largest})
    sub_dt, sub_gt = [detections[i] for i in pick], [ground_truth[i] for i in pick]

    t0 = time.perf_counter()
    want = ref.evaluate(sub_dt, sub_gt, **options)
    cpu_ms = (time.perf_counter() - t0) * 1e3

    full, sub = DeviceRun(detections, ground_truth, options, dev, stream), DeviceRun(sub_dt, sub_gt, options, dev, stream)
    for run in (sub, full):
        run.match()
        run.accumulate()
        torch.cuda.synchronize()
        assert int(run.m["status"].item()) == 0
    for key in ("image", "rank", "index", "score", "match", "n_pos"):
        assert np.array_equal(sub.m[key].cpu().numpy(), want["match"][key]), f"{key}: the device differs from the restatement"
    assert np.array_equal(sub.m["ignore"].cpu().numpy().astype(bool), want["match"]["ignore"]), "ignore: the device differs from the restatement"
    for key, got in (("precision", sub.precision), ("scores", sub.scores), ("recall", sub.recall)):
        assert np.array_equal(got.cpu().numpy().view(np.int64), want[key].view(np.int64)), f"{key}: the device differs from the restatement"
    stats = dm.summarize_stats(full.precision.cpu().numpy(), full.recall.cpu().numpy(), full.iou_thrs, full.max_dets)

    med = {}
    for rnd in range(2):
        for name, run in (("full", full), ("sub", sub)):
            med[f"{name}_match_ms"] = median_ms(run.match, stream, a.warmup, a.iters)
            med[f"{name}_accumulate_ms"] = median_ms(run.accumulate, stream, a.warmup, a.iters)
    line = {"images": a.images, "ground_truths": int(full.boxes.gt_offset[-1]), "max_gt_per_image": full.boxes.max_gt, "detections": int(full.boxes.dt_offset[-1]),
            "kept": full.n_kept, "max_dets": list(full.max_dets), "ap": float(stats[0]), "match_ms": med["full_match_ms"], "accumulate_ms": med["full_accumulate_ms"],
            "match_gpairs_per_s": full.pairs / med["full_match_ms"] / 1e6, "sub_images": len(pick), "sub_kept": sub.n_kept, "sub_match_ms": med["sub_match_ms"],
            "sub_accumulate_ms": med["sub_accumulate_ms"], "sub_cpu_ms": cpu_ms, "sub_cpu_x": cpu_ms / (med["sub_match_ms"] + med["sub_accumulate_ms"]),
            "sub_bitwise_equal": True}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/detection_ap_bench.py --iters {a.iters} --warmup {a.warmup} --images {a.images} --stride {a.stride} --max-dets {a.max_dets}: vghev_box_match and "
                    "vghev_pr_accumulate on device-resident inputs; ms are medians of HIP-event times; cpu = one run of the float64 NumPy restatement on the sub-sample\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
