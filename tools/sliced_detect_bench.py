"""Sliced detection of a 12 MP photograph: a seeded 3000 x 4000 uint8 image, VGGHeads_L with synthetic weights, 640 x 640 tiles with 25 % overlap plus the whole
image (48 + 1 tiles), the stages of ``HeadDetector.detect_sliced`` timed one by one with the photograph already on the device.

    tiles_ms    HIP events around the tile forwards: ``engine.detect`` on pitched sub-views of the photograph, --max-batch tiles at a time, and the copies that put
                the chunks' slabs side by side.
    merge_ms    HIP events around vghm_merge_tiles alone (sliced.merge_tiles on those slabs; the outputs and the workspace are allocated inside the events).
    decode_ms   HIP events around FLAME decode of the merged survivors, each un-padded with its own tile's row.
    call_ms     HIP events around the whole ``detect_sliced`` call, upload and host-side result objects included; call_host_ms is the host clock of the same.
    merge_cpu_ms   the NumPy restatement of the merge (tests/slice_merge_ref.py, vectorised form) on this machine's CPU for the same candidates, one run; the
                device's outputs are compared BITWISE with it before anything is timed.
    crowd_merge_ms   vghm_merge_tiles alone with all 4 900 slots taken by a seeded crowd in which neighbouring tiles report the same heads (synthetic weights leave
                the real tiles few candidates and no duplicates), beside crowd_merge_cpu_ms, the restatement on the same crowd; compared bitwise as well.
    candidates / decoded   what the tiles produced against what FLAME decode ran on: the merge runs ahead of the decode so that duplicates are never decoded.

The confidence threshold is the 11th best score of the weakest tile, so that every tile yields candidates (the weights are synthetic: the detections mean
nothing, the work is real).  Medians over --iters after --warmup.

    python tools/sliced_detect_bench.py [--iters 10] [--warmup 2] [--model vgg_heads_l] [--max-batch 16] [--out profiles/sliced_detect.txt]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import slice_merge_ref as ref  # noqa: E402

from head_detector_amd import sliced  # noqa: E402
from head_detector_amd.detector import HeadDetector  # noqa: E402
from head_detector_amd.synthetic import synthetic_flame_model  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="vgg_heads_l")
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sliced_detect_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        det = HeadDetector(a.model, weights="synthetic", max_batch=a.max_batch, flame_model=synthetic_flame_model(seed=3))
    eng, S, mb = det.model, 640, a.max_batch
    image = np.random.default_rng(0).integers(0, 256, (a.height, a.width, 3), dtype=np.uint8)
    plan = sliced.plan_slices(a.height, a.width, S, overlap=0.25)
    T, kk = plan.n_tiles, eng.keep_k
    photo = torch.from_numpy(image).to(dev)
    views = [photo[y:y + h, x:x + w] for x, y, w, h in plan.tiles[:, :4].tolist()]
    conf = min(float(eng.model(views[at:at + mb])[1][:, 10, 0].min()) for at in range(0, T, mb))
    f32 = dict(dtype=torch.float32, device=dev)
    boxes, scores, params = torch.empty(T, kk, 4, **f32), torch.empty(T, kk, **f32), torch.empty(T, kk, 413, **f32)
    counts = torch.empty(T, dtype=torch.int32, device=dev)

    def tiles():
        for at in range(0, T, mb):
            d = eng.detect(views[at:at + mb], confidence_threshold=conf, flame=None)
            n = len(views[at:at + mb])
            for dst, part in ((boxes, d.boxes), (scores, d.scores), (params, d.flame_params), (counts, d.counts)):
                dst[at:at + n].copy_(part)

    held = {}

    def merge():
        held["m"] = sliced.merge_tiles(boxes, scores, counts, plan, want_status=True)

    tiles()
    merge()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = ref.merge_vec(boxes.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy(), plan)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    bad = ref.same_bytes({k: getattr(held["m"], k).cpu().numpy() for k in ref.OUTPUTS}, want)
    assert bad is None, f"{bad}: the device differs from the restatement"
    n = int(want["n_heads"][0])
    rows, tile_of = held["m"].head_row[:n].long(), held["m"].head_tile[:n].long()
    survivors, unpad = params.view(T * kk, -1)[rows].contiguous(), torch.from_numpy(plan.unpad).to(dev)[tile_of].contiguous()
    P = eng.program

    def decode():
        if n:
            det._flame.decode(survivors, unpad=unpad, shape_live=P.shape_c, expr_live=P.expr_c, want_vertices=False)

    def call():
        held["r"] = det.detect_sliced(image, conf)

    med = {}
    for _ in range(2):  # measured twice, the second round is reported
        med["tiles_ms"] = median_ms(tiles, stream, a.warmup, a.iters)
        med["merge_ms"] = median_ms(merge, stream, a.warmup, a.iters)
        med["decode_ms"] = median_ms(decode, stream, a.warmup, a.iters)
        med["call_ms"] = median_ms(call, stream, a.warmup, a.iters)
    host = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    assert len(held["r"].heads) == n
    # the merge alone with every slot taken by a seeded crowd (tests/slice_merge_ref.py random_family): synthetic weights leave the tiles few candidates and no duplicates
    cb, cs, cc = ref.random_family(plan, kk, T * kk, seed=0)
    t0 = time.perf_counter()
    crowd_want = ref.merge_vec(cb, cs, cc, plan)
    crowd_cpu_ms = (time.perf_counter() - t0) * 1e3
    cb, cs, cc = (torch.from_numpy(v).to(dev) for v in (cb, cs, cc))

    def crowd_merge():
        held["c"] = sliced.merge_tiles(cb, cs, cc, plan, want_status=True)

    med["crowd_merge_ms"] = median_ms(crowd_merge, stream, a.warmup, a.iters)
    bad = ref.same_bytes({k: getattr(held["c"], k).cpu().numpy() for k in ref.OUTPUTS}, crowd_want)
    assert bad is None, f"crowd {bad}: the device differs from the restatement"
    crowd_status = np.bincount(crowd_want["status"], minlength=5)
    crowd = {"crowd_candidates": T * kk, "crowd_truncated": int(crowd_status[2]), "crowd_suppressed": int(crowd_status[3]), "crowd_kept": int(crowd_want["n_kept_uncapped"][0]),
             "crowd_merge_cpu_ms": crowd_cpu_ms, "crowd_merge_cpu_x": crowd_cpu_ms / med["crowd_merge_ms"]}
    status = np.bincount(want["status"], minlength=5)
    line = {"model": a.model, "image": [a.height, a.width], "tiles": T, "max_batch": mb, "keep_k": kk, "confidence_threshold": conf, "candidates": int(counts.sum().item()),
            "truncated": int(status[2]), "suppressed": int(status[3]), "decoded": n, **med, "call_host_ms": float(np.median(host)), "merge_cpu_ms": cpu_ms,
            "merge_cpu_x": cpu_ms / med["merge_ms"], **crowd, "merge_bitwise_equal": True}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/sliced_detect_bench.py --iters {a.iters} --warmup {a.warmup} --model {a.model} --max-batch {a.max_batch}: the stages of HeadDetector.detect_sliced on a "
                    "seeded 12 MP image, synthetic weights; ms are medians of HIP-event times; merge_cpu_ms = one run of the NumPy restatement of the merge\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
