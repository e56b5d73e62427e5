"""Mesh benchmark metrics at the benchmark's own sizes with 1, 16, 100 and 1 000 heads whose vertices are already on the device: Z_n at the 2 470 head
vertices (top_k = 5, both neighbour rules) and the one-sided chamfer search of 2 094 face vertices against 5 023 predicted vertices (with a per-head
similarity transform and query scale, as chamfer_to_gt issues it), beside the float64 NumPy restatement (tests/mesh_metrics_ref.py) on this machine's CPU.

    launch    HIP events around vghev_z_order / vghev_nearest alone: the memset of the counts and rank_kernel or z_nearest_kernel; nearest_kernel and
              mean_kernel.  Inputs, outputs and the transform are on the device before the first event.
    cpu       the restatement of ONE head, single call, host clock; it is a per-head loop, so n heads cost n times that.  cpu_x = n * cpu / launch.
    pairs/s   distance evaluations the algorithm needs (reference rule: N * N * top_k ranked comparisons over N * top_k distances per column tile, counted
              as N * N * top_k; nearest rule: N * N; chamfer: M * P), per head, times heads, over the launch time.

Medians over --iters after --warmup; the head counts are measured twice, alternating, and the second round is reported.  The counts and distances of the
first head are compared with the restatement before anything is timed.

    python tools/mesh_metrics_bench.py [--iters 20] [--warmup 3] [--heads 1,16,100,1000] [--out profiles/mesh_metrics.txt]
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

import mesh_metrics_ref as mr  # noqa: E402

from head_detector_amd import _lib_eval  # noqa: E402

N_HEAD, M_FACE, V = 2470, 2094, 5023
TOP_K = 5


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
    ap.add_argument("--heads", default="1,16,100,1000", help="head counts, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_metrics_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    lib = _lib_eval.load()
    stream = torch.cuda.current_stream(dev)
    v_template = np.load(os.path.join(ROOT, "tests", "golden", "flame_decode.npz"))["v_template"] * 1000.0
    rng = np.random.default_rng(0)
    head_idx = np.sort(rng.choice(V, N_HEAD, replace=False))  # stand-ins for the reference's index lists (user-supplied assets): the sizes are what counts
    face_idx = np.sort(rng.choice(V, M_FACE, replace=False))
    counts = [int(v) for v in a.heads.split(",")]
    n_max = max(counts)
    gt = (v_template[None] + rng.uniform(-0.5, 0.5, size=(n_max, V, 3))).astype(np.float32)
    pred = (gt + rng.normal(0.0, 4.0, size=gt.shape)).astype(np.float32)
    T = np.tile(np.concatenate([np.eye(3), np.full((3, 1), 0.25)], axis=1), (n_max, 1, 1))
    qs, ps = np.full((n_max,), 1.01), np.full((n_max,), 0.99)

    t0 = time.perf_counter()
    cpu_ref = mr.agree(pred[0, head_idx], gt[0, head_idx], TOP_K, "reference")
    t1 = time.perf_counter()
    cpu_near = mr.agree(pred[0, head_idx], gt[0, head_idx], TOP_K, "nearest")
    t2 = time.perf_counter()
    cpu_sq, cpu_at, cpu_mean = mr.nearest_one(gt[0, face_idx], pred[0], T[0], qs[0], ps[0])
    t3 = time.perf_counter()
    cpu_ms = {"z_reference": (t1 - t0) * 1e3, "z_nearest": (t2 - t1) * 1e3, "chamfer": (t3 - t2) * 1e3}

    d_gt_head, d_pred_head = torch.from_numpy(gt[:, head_idx]).to(dev), torch.from_numpy(pred[:, head_idx]).to(dev)
    d_gt_face, d_pred = torch.from_numpy(gt[:, face_idx]).to(dev), torch.from_numpy(pred).to(dev)
    d_T, d_qs, d_ps = (torch.from_numpy(x).to(dev) for x in (T, qs, ps))
    d_count = torch.empty((n_max,), dtype=torch.int32, device=dev)
    d_sq = torch.empty((n_max, M_FACE), dtype=torch.float64, device=dev)
    d_at = torch.empty((n_max, M_FACE), dtype=torch.int32, device=dev)
    d_mean = torch.empty((n_max,), dtype=torch.float64, device=dev)

    def z_job(n, mode):
        job = _lib_eval.ZOrderJob()
        job.n_heads, job.n_points, job.top_k, job.mode = n, N_HEAD, TOP_K, _lib_eval.NEIGHBOURS[mode]
        job.pred_dev, job.gt_dev, job.agree_dev = d_pred_head.data_ptr(), d_gt_head.data_ptr(), d_count.data_ptr()
        return lambda: _lib_eval.check(lib.vghev_z_order(job, stream.cuda_stream))

    def near_job(n):
        job = _lib_eval.NearestJob()
        job.n_heads, job.n_queries, job.n_points = n, M_FACE, V
        job.query_dev, job.query_scale_dev, job.points_dev, job.transform_dev, job.point_scale_dev = (d_gt_face.data_ptr(), d_qs.data_ptr(), d_pred.data_ptr(),
                                                                                                      d_T.data_ptr(), d_ps.data_ptr())
        job.sqdist_dev, job.index_dev, job.mean_dev = d_sq.data_ptr(), d_at.data_ptr(), d_mean.data_ptr()
        return lambda: _lib_eval.check(lib.vghev_nearest(job, stream.cuda_stream))

    z_job(1, "reference")()
    assert int(d_count[0]) == cpu_ref, "Z_n, reference rule: the device differs from the restatement"
    z_job(1, "nearest")()
    assert int(d_count[0]) == cpu_near, "Z_n, nearest rule: the device differs from the restatement"
    near_job(1)()
    assert np.array_equal(d_sq[0].cpu().numpy(), cpu_sq) and np.array_equal(d_at[0].cpu().numpy(), cpu_at) and float(d_mean[0]) == cpu_mean, "chamfer search differs"

    pairs = {"z_reference": N_HEAD * N_HEAD * TOP_K, "z_nearest": N_HEAD * N_HEAD, "chamfer": M_FACE * V}
    lines = []
    for rnd in range(2):
        for n in counts:
            jobs = {"z_reference": z_job(n, "reference"), "z_nearest": z_job(n, "nearest"), "chamfer": near_job(n)}
            med = {"heads": n}
            for key, job in jobs.items():
                ms = median_ms(job, stream, a.warmup, a.iters)
                med[f"{key}_launch_ms"] = ms
                med[f"{key}_gpairs_per_s"] = n * pairs[key] / ms / 1e6
                med[f"{key}_cpu_one_head_ms"] = cpu_ms[key]
                med[f"{key}_cpu_x"] = n * cpu_ms[key] / ms
            if rnd == 1:
                lines.append(json.dumps(med))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/mesh_metrics_bench.py --iters {a.iters} --warmup {a.warmup}: vghev_z_order ({N_HEAD} points, top_k {TOP_K}) and vghev_nearest ({M_FACE} x {V}, "
                    "transform and scales) on device-resident inputs; ms are medians of HIP-event times; cpu = the float64 NumPy restatement of one head\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
