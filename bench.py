#!/usr/bin/env python3
"""Headline benchmark: images/sec at 640x640 for the VGGHeads forward path (BASELINE.json).

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python bench.py --gpus N ...          (no torchrun environment: spawns the N ranks itself through torch.distributed.run)

A plain run sets up, warms up, times the K steps of the headline workload and prints the JSON line (its `roofline` from the HIP events
of the timed steps, without traffic).  --dump-outputs DIR then writes the detections of the last timed forward (rank 0) as DIR/*.npy
(dump_detections).  Everything else below -- the secondary workloads, the FLAME decode sweep, the overlap check, power / throttle
sampling, live PMC traffic, cpu_baseline and the deviation reports -- runs with --full only.

One step = one pass of the whole hot path over one batch that is already resident in HBM:
    network (stem + ~125 fused convs) -> box/score decode -> per-image top-k(1000) -> candidate gather + FLAME
    fix-up -> NMS (every image) -> compaction -> FLAME decode of every surviving head -> (N>1) RCCL gather to rank 0.
Workload at N=1 = BASELINE.json configs[2]: VGGHeads_L, bf16, batch 64 @ 640x640 with FLAME decode per detection (per GPU; weak
scaling: configs[3] = 8 x this).  With --full, measured in the same run and reported inside `config` (and on stderr):
    configs[1]  VGGHeads_M, batch 32 @ 640                              -> config.secondary_vgg_heads_m_b32
    configs[4]  VGGHeads_L @ 1280x1280 crowd (>= 32 heads / image)      -> config.secondary_vgg_heads_l_b16_1280_crowd (one GPU's shard of the 8-GPU config) and
                                                                           config.secondary_vgg_heads_l_b256_1280_crowd (the stated batch on ONE GPU, chunked arena)
    the matrix-core PARITY mode (fp16x3: outputs within north_star's IoU >= 0.999 / 1e-4 of the fp32 reference) and the fp32 VALU mode
                                                                        -> config.parity_mode
    configs[0]'s shape on the GPU: ONE image per synchronous detect() call (L and M), median / min ms        -> config.latency_one_image_synchronous
Weights / FLAME constants are seeded synthetic tensors of the exact architecture (no network for the real assets).
The random-weight network's scores are arbitrary, so the NMS confidence threshold is calibrated ONCE (untimed) so that
about 3 heads per image survive; nothing is skipped inside the timed region.

The JSON line also carries (`traffic` and cpu_baseline with --full)
  roofline     : the conv kernel family against the dense bf16 MFMA peak, measured live with HIP events on the engine's stream around
                 the network part of every timed step; `traffic` = HBM bytes per forward from PMC passes (FETCH_SIZE / WRITE_SIZE,
                 separate rocprofv3 runs of tools/traffic_run.py launched by this script when rocprofv3 is on the box, else the
                 committed profiles/ figure) next to the algorithmic bytes of the op program;
  cpu_baseline : the oracle (torch-CPU fp32 restatement of the reference pipeline) on a bounded sample, rank 0 / N=1 only; its
                 outputs on one 640x640 image are also what config.parity_mode.vs_oracle compares the parity modes with.
The run refuses to start with any VGH_* environment variable set (experiment knobs must not leak into a measurement).
"""
import argparse
import contextlib
import json
import os
import shutil
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_DENSE_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16
MFMA_FP8_DENSE_PEAK_TFLOPS = 5000.0  # same guide: ~5 PFLOP/s dense fp8 (v_mfma_f32_32x32x64_f8f6f4)
# r06: the 8-bit link modes are EXPERIMENTAL -- 24 link tensors = 28 % of the FLOPs on the 8-bit MFMA, per-tensor scales calibrated on two seeded random
# images, 2.5 - 10 x the bf16 mode's deviation for + 5 - 11 % images/s -- and are reported as such, not beside the headline
EXPERIMENTAL_8BIT = "experimental: partial coverage (links between 3x3 convs only), synthetic calibration; not a headline mode"
NORTH_STAR_IMG_PER_S_PER_GPU = 1250.0  # BASELINE.json north_star: >= 10k images/sec on 8 GPUs


def _cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _physical_cores(fallback: int) -> int:
    """Physical cores of the host (distinct (physical id, core id) pairs of /proc/cpuinfo); SMT siblings are not counted."""
    try:
        seen, phys = set(), None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                seen.add((phys, line.split(":")[1].strip()))
        return len(seen) or fallback
    except OSError:
        return fallback


def _cpu_limits() -> dict:
    """What actually bounds the host threads of this process: the scheduler affinity mask and the cgroup CPU quota (a box that shows 64 cores but grants a quota of
    16 CPU-seconds per second runs 64 threads SLOWER than 16 -- VERDICT r05 weak 14 saw exactly that shape in the thread sweep)."""
    out = {"affinity_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "os_cpu_count": os.cpu_count()}
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            raw = open(path).read().split()
        except OSError:
            continue
        out["cgroup_file"] = path
        if path.endswith("cpu.max"):  # "<quota|max> <period>"
            out["cgroup_cpu_max"] = " ".join(raw)
            if raw and raw[0] != "max" and len(raw) > 1:
                out["cgroup_cpus_granted"] = round(int(raw[0]) / int(raw[1]), 2)
        else:
            q = int(raw[0]) if raw else -1
            try:
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            except OSError:
                per = 100000
            out["cgroup_cpu_max"] = f"{q} {per}"
            if q > 0:
                out["cgroup_cpus_granted"] = round(q / per, 2)
        break
    return out


def _timed(fn, iters: int):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def cpu_baseline(variant: str, image_size: int, flame_model):
    """Oracle (kind "port": the torch-CPU fp32 restatement of the reference pipeline, oracle/) timed on the host cores, on a bounded
    sample: end to end at batch 1 / 8 / 32 (best reported as `value`), FLAME decode alone at n = 1 / 100, top-k + NMS
    alone on 1000 candidates; median and min of the iterations.  Also returns the oracle's dense outputs for ONE seeded image
    (the checker role: config.parity_mode.vs_oracle)."""
    import torch

    from head_detector_amd import arch
    from oracle import flame_oracle as fo
    from oracle import net_oracle, postproc_oracle as po

    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    phys = max(1, min(avail, _physical_cores(avail), 64))  # one thread per physical core, at most 64
    torch.set_num_threads(phys)
    sd = arch.random_state_dict(variant, 1)
    net = net_oracle.YoloHeadsOracle({"vgg_heads_m": "m", "vgg_heads_l": "l"}[variant])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    consts = fo.FlameConstants(flame_model, torch.float32)
    net(torch.rand(1, 3, 64, 64))  # spin up the thread pool / allocator on a tiny input (untimed)
    t_start = time.time()
    # torch's CPU convolutions do not scale monotonically with threads on these hosts (r04, EPYC 9575F: 64 threads 1.5 img/s, 32 threads 3.5 img/s), and not the same
    # way at every batch size: each batch size below is timed at the best count of its own short sweep; `cores` = the count behind `value`

    def end_to_end(x):
        b, s, f = net(x)
        conf = float(s[:, 3, 0].min())
        res = po.postprocess_batched(b, s, f, conf, 0.5)
        fo.reproject(consts, torch.cat([r[2] for r in res]))

    # one thread count for every batch size understated the batched baseline (b1 7.8 > b8 2.6 > b32 1.8 img/s on 16 threads of a 64-core
    # host: the count was chosen on the network alone at batch 4).  Each batch size now runs at ITS best count: b1 and b8 sweep {physical cores <= 64, 32, 16, 8}
    # with one end-to-end pass each, b32 tries the two best counts of the b8 sweep; the timed iterations follow at the winner and `threads` says which it was
    e2e, n_img = {}, 0
    cand = sorted({phys, min(phys, 32), min(phys, 16), min(phys, 8)}, reverse=True)
    order_b8 = cand
    for bs, iters in ((1, 10), (8, 3), (32, 2)):
        x = torch.rand(bs, 3, image_size, image_size, generator=torch.Generator().manual_seed(0))
        if bs == 1:
            end_to_end(x)  # warm-up at full size
        trial = {}
        for t in (cand if bs <= 8 else order_b8[:2]):
            torch.set_num_threads(t)
            if bs == 1:
                end_to_end(x)
            t0 = time.perf_counter()
            end_to_end(x)
            trial[t] = round(bs / (time.perf_counter() - t0), 3)
            n_img += bs
        if bs == 8:
            order_b8 = sorted(trial, key=trial.get, reverse=True)
        tb = max(trial, key=trial.get)
        torch.set_num_threads(tb)
        ts = [bs / trial[tb]]  # the sweep's pass at the winning count is a sample too
        for _ in range(iters):
            t0 = time.perf_counter()
            end_to_end(x)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        e2e[f"b{bs}"] = {"img_per_s_median": round(bs / ts[len(ts) // 2], 3), "img_per_s_best": round(bs / ts[0], 3), "iters": len(ts), "threads": tb,
                         "thread_sweep_img_per_s": {str(k): v for k, v in trial.items()}}
        n_img += bs * iters
    best_b = max(e2e, key=lambda k: e2e[k]["img_per_s_median"])
    best, cores = e2e[best_b]["img_per_s_median"], e2e[best_b]["threads"]
    torch.set_num_threads(cores)
    # FLAME decode alone (per-head mesh-decode metric)
    dec = {}
    for n in (1, 100):
        p = fo.synthetic_params(n, seed=2)
        fo.reproject(consts, p)
        med, mn = _timed(lambda: fo.reproject(consts, p), 10)
        dec[f"n{n}"] = {"us_per_head_median": round(med / n * 1e6, 1), "us_per_head_min": round(mn / n * 1e6, 1)}
    # top-k(1000) + NMS alone on one image's 8400 anchors
    bx, sc = po.synthetic_detections(1, seed=2, image_size=image_size)
    fl = fo.synthetic_params(bx.shape[1], seed=4)[None]

    def topk_nms():
        cb, cs, cf, _ = po.decoding_topk(bx, sc, fl, 1000)
        po.postprocess_batched(cb, cs, cf, 0.5, 0.5)

    topk_nms()
    med, mn = _timed(topk_nms, 10)
    line = {"value": best, "unit": "images/sec", "cores": cores, "kind": "port", "cpu": _cpu_model(), "physical_cores_visible": phys, "host_cpu_limits": _cpu_limits(),
            "sample": f"{n_img} images ({variant} fp32 unfused torch-CPU net + top-k + NMS + FLAME decode at batch 1/8/32; median of the iterations, each batch size at the best thread count of its own sweep, best batch ({best_b}) reported) in {time.time() - t_start:.1f}s",
            "end_to_end": e2e,
            "note": "per-image cost of the unfused fp32 torch-CPU pipeline RISES with batch at every thread count (b1 fits the caches; b8 / b32 stream every elementwise pass through DRAM): "
                    "batch 1 -- the reference's own single-image API shape -- is its best case and is what `value` reports",
            "flame_decode_alone": dec, "topk_nms_alone_1000cand": {"ms_median": round(med * 1e3, 3), "ms_min": round(mn * 1e3, 3)}}
    # checker role: the oracle's dense decode of one seeded image (same weights as every engine below)
    x1 = torch.rand(1, 3, image_size, image_size, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ob, os_, of = net.dense(x1)
    return line, dict(x=x1, boxes=ob, scores=os_, flame=of)


def _iou(a, b):
    import torch

    lt, rb = torch.maximum(a[..., :2], b[..., :2]), torch.minimum(a[..., 2:], b[..., 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter)


def deviation_from_oracle(variant: str, precision: str, ref: dict, dev) -> dict:
    """One engine mode on the oracle's image: dense boxes / scores and the 413-vectors of the mode's own top-100 candidates, looked up
    BY ANCHOR in the oracle's dense output (relative to |ref| + 1; the exp()-amplified scale channel on its logit)."""
    import torch

    from head_detector_amd.engine import VGHeadsEngine

    S = ref["x"].shape[-1]
    eng = VGHeadsEngine(variant, image_size=S, max_batch=1, seed=1, precision=precision)
    try:
        _, _, flame = eng.model(ref["x"].to(dev))
        torch.cuda.synchronize()
        db, ds = eng.boxes_all[:1].cpu(), eng.scores_all[:1].cpu()
        idx = eng.idx[0, :100].cpu().long()
        of_at = ref["flame"][0, idx]
        rel = (flame[0, :100].cpu() - of_at).abs() / (of_at.abs() + 1.0)
        return {"dense_iou_min": round(float(_iou(db, ref["boxes"]).min()), 6), "top100_iou_min": round(float(_iou(db[0, idx], ref["boxes"][0, idx]).min()), 6),
                "dense_score_max_abs_err": float((ds - ref["scores"][..., 0]).abs().max()), "top100_param_max_rel_err": float(rel[:, :412].max()),
                "top100_log_scale_max_abs_err": float((torch.log(flame[0, :100, 412].cpu()) - torch.log(of_at[:, 412])).abs().max())}
    finally:
        eng.close()


DUMP_BUDGET_BYTES = 64 << 20


def dump_detections(det, out_dir: str, budget: int = DUMP_BUDGET_BYTES) -> None:
    """--dump-outputs: what a caller of the timed path receives from one forward (engine.Detections), valid rows only, image-major:
    counts [B]; boxes [n, 4], scores [n], flame_params [n, 413] (the first counts[b] rows of image b); head_image [n], head_pose [n, 3],
    vertices_3d [n, V, 3].  float32 as computed, the integer arrays as float64.  When the vertices would take the total past `budget`, a
    seeded sample of their rows is written (sorted, indices in vertices_3d_rows.npy)."""
    import numpy as np
    import torch

    counts = det.counts.cpu().long()
    valid = torch.arange(det.boxes.shape[1])[None, :] < counts[:, None]
    arrays = {"counts": counts.double(), "boxes": det.boxes.cpu()[valid], "scores": det.scores.cpu()[valid], "flame_params": det.flame_params.cpu()[valid]}
    if det.vertices_cap is not None:
        arrays.update(head_image=det.head_image.cpu().double(), head_pose=det.head_pose.cpu(), vertices_3d=det.vertices_3d.cpu())
    arrays = {k: v.numpy() for k, v in arrays.items()}
    vert = arrays.get("vertices_3d")
    if vert is not None and sum(a.nbytes for a in arrays.values()) > budget:
        room = budget - sum(a.nbytes for k, a in arrays.items() if k != "vertices_3d") - 8 * vert.shape[0]  # 8 bytes per row: the row indices
        rows = np.sort(np.random.default_rng(0).choice(vert.shape[0], max(0, room // vert[0].nbytes), replace=False))
        arrays.update(vertices_3d=vert[rows], vertices_3d_rows=rows.astype(np.float64))
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), np.ascontiguousarray(a))
    print(f"[bench] --dump-outputs: {', '.join(f'{k}{list(a.shape)}' for k, a in arrays.items())} -> {out_dir}", file=sys.stderr)


def make_step(eng, flame, images, unpad, conf, B, slots, gat, overlap, use_graph, n_heads_all, ev0=None, ev1=None, ready=None):
    """One step of the benchmark loop as a closure (also driven by tests/test_dist_cpu.py with a stand-in engine on gloo, so that the
    N>1 control flow -- the output slots, the gatherer's slot hand-shake, the lazy hand-over -- runs on every CPU test pass).

    r05: the exchange is LAZY.  Queuing batch k's pack + collectives right after its select (r02 - r04) parks the communication stream's hardware queue behind the
    detector's LOW-PRIORITY side stream, and a parked fourth queue cost the network 7 - 8 % (tools/exchange_probe.py, one RCCL rank: 13.63 vs 12.60 ms per forward, the
    same with plain copies instead of collectives).  Now select(k) only gets an event recorded behind it (vgh_detector_record: nothing waits for it on the device); at
    step k + EXCHANGE_LAG the HOST synchronises on that event -- two batches old, so the host still runs ahead of the GPU -- and then queues exchange(k) with no
    device-side wait: 12.72 ms.  len(slots) >= EXCHANGE_LAG + 1 output slots keep batch k's results intact until then; `step.flush()` queues what is still pending."""
    nstep = [0]
    nslots = len(slots) if slots else 2
    EXCHANGE_LAG = 2
    assert gat is None or nslots > EXCHANGE_LAG, "the lazy exchange needs at least three output slots"
    sel_done = [eng.make_event() for _ in range(nslots)] if gat is not None else None
    pending = []  # (slot, detections) of the batches whose exchange has not been queued yet, oldest first

    def hand_over(n_keep):
        while len(pending) > n_keep:
            s0, d0 = pending.pop(0)
            sel_done[s0].synchronize()  # host: that batch's select is over
            gat.submit(s0, d0.boxes, d0.scores, d0.flame_params, d0.counts, d0.n_heads, d0.vertices_cap, None)

    def step(i=None):
        s = nstep[0] % nslots
        nstep[0] += 1
        if gat is not None:
            gat.wait_slot_free(s, eng.stream)  # the exchange that last read this output slot (nslots batches ago) is over
        if i is not None and ev0 is not None:
            ev0[i].record(eng.stream)  # HIP events on the stream the kernels are launched on
        if B > getattr(eng, "arena_batch", B):
            # a batch whose tensors pass 2 GiB (configs[4] at its stated batch: 256 images @1280 = ten arena chunks): network + candidate stages chunk by chunk
            # (vgh_detector_candidates); the "network part" between the two events then includes the chunks' decode / top-k / gather kernels
            eng.forward_candidates(images, use_graph=use_graph)
            if i is not None and ev1 is not None:
                ev1[i].record(eng.stream)
        else:
            eng.forward_net(images, use_graph=use_graph)
            if i is not None and ev1 is not None:
                ev1[i].record(eng.stream)
            # post-network stages: decode/top-k/gather, then ONE library call for NMS + compaction + head list + FLAME decode of every
            # survivor (vgh_detector_select); the head count stays on the device, so the host queues ahead of the GPU
            eng.candidates(B, lazy_flame=True)  # (r06) the select below follows at once: the survivors' FLAME vectors come straight from the prediction buffers
        k = i if i is not None else 0
        det = eng.select(B, confidence_threshold=conf, iou_threshold=0.5, flame=flame, unpad=unpad, n_heads_out=n_heads_all[k : k + 1],
                         slot=slots[s] if slots else None)
        if gat is not None:
            eng.record_select_done(sel_done[s])  # behind this batch's select, on whichever stream runs it; nothing waits for it on the device
            pending.append((s, det))
            hand_over(EXCHANGE_LAG)
        return det

    step.flush = lambda: hand_over(0) if gat is not None else None
    return step


def live_traffic(variant: str, batch: int, split: int, forwards: int = 6):
    """HBM bytes of one forward, measured NOW: two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE: they do not fit one pass; kernel-trace
    only) around `tools/traffic_run.py --forwards N` -- network forwards only, so counter sum / N is bytes per forward.  Counter
    conventions per MI355X_MICROARCH.md (HBM section): KiB units, FETCH_SIZE doubled on gfx950, WRITE_SIZE as is.  Returns None when
    rocprofv3 is missing or a pass fails (the caller then falls back to the committed profile)."""
    import csv
    import glob
    import tempfile

    from head_detector_amd import arch

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    out = {}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["TMPDIR"] = "/tmp"
    with tempfile.TemporaryDirectory(prefix="vgh_pmc_") as td:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            cmd = [exe, "--kernel-trace", "--output-format", "csv", "--pmc", ctr, "-d", td, "-o", ctr, "--", sys.executable, os.path.join(ROOT, "tools", "traffic_run.py"),
                   "--variant", variant, "--batch", str(batch), "--forwards", str(forwards), "--split", str(split)]
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=240)
            except (subprocess.TimeoutExpired, OSError):
                return None
            files = sorted(glob.glob(os.path.join(td, "**", f"{ctr}_counter_collection.csv"), recursive=True))
            if r.returncode != 0 or not files:
                return None
            tot, n = 0.0, 0
            for row in csv.DictReader(open(files[0])):
                k = row["Kernel_Name"]
                if row["Counter_Name"] == ctr and arch.is_net_kernel(k):
                    tot += float(row["Counter_Value"])
                    n += 1
            if n == 0:
                return None
            out[ctr] = (tot, n)
            try:  # every op is one launch per lane: a kernel family missing from arch.NET_KERNEL_MARKERS would show up here as too few dispatches
                info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                expected = info["ops_per_forward"] * split * forwards
            except (IndexError, KeyError, ValueError):
                expected = None
            if expected is not None and n != expected:
                sys.stderr.write(f"[bench] live traffic: {n} network dispatches counted, {expected} expected -- not reporting a partial sum\n")
                return None
    rd = out["FETCH_SIZE"][0] * 1024 * 2 / forwards
    wr = out["WRITE_SIZE"][0] * 1024 / forwards
    return dict(read_bytes_per_forward=rd, write_bytes_per_forward=wr, launches_per_forward=out["FETCH_SIZE"][1] / forwards, forwards=forwards,
                source=f"live: rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE (two passes) around tools/traffic_run.py --forwards {forwards} --split {split}")


class PowerSampler:
    """Best-effort socket power / shader clock of GPU `index` during the timed region (a daemon thread reading the amdgpu hwmon files every 50 ms;
    nothing is reported when the files are not there).  The conv stack runs within a few % of the board's power cap (profiles/r03_power.txt), which is
    what bounds `roofline.frac` -- so the line says how close this run was."""

    def __init__(self, index: int):
        import glob

        self.samples, self._stop, self._thr = [], False, None
        # the box exposes every card's hwmon but only this rank's GPU to HIP: find the card by the PCI address HIP reports for the device
        self.dir = None
        try:
            import ctypes

            hip, buf = ctypes.CDLL("libamdhip64.so"), ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, int(index)) == 0:
                hw = glob.glob(f"/sys/bus/pci/devices/{buf.value.decode().lower()}/hwmon/hwmon*")
                self.dir = hw[0] if hw else None
        except OSError:
            pass
        self.pfile = next((os.path.join(self.dir, f) for f in ("power1_average", "power1_input") if self.dir and os.path.exists(os.path.join(self.dir, f))), None)
        self.ffile = os.path.join(self.dir, "freq1_input") if self.dir and os.path.exists(os.path.join(self.dir, "freq1_input")) else None
        cap = os.path.join(self.dir, "power1_cap") if self.dir else None
        self.cap_w = None
        try:
            if cap and os.path.exists(cap):
                self.cap_w = int(open(cap).read()) / 1e6
        except (OSError, ValueError):
            pass

    def _run(self):
        while not self._stop:
            try:
                p = int(open(self.pfile).read()) / 1e6
                f = int(open(self.ffile).read()) / 1e6 if self.ffile else None
                self.samples.append((p, f))
            except (OSError, ValueError):
                return
            time.sleep(0.05)

    def __enter__(self):
        if self.pfile:
            import threading

            self._thr = threading.Thread(target=self._run, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        if self._thr:
            self._thr.join(timeout=1.0)
        return False

    def summary(self):
        if len(self.samples) < 3:
            return None
        p = sorted(x[0] for x in self.samples)
        out = {"socket_power_w_median": round(p[len(p) // 2], 1), "socket_power_w_max": round(p[-1], 1), "samples": len(p), "source": self.pfile}
        f = sorted(x[1] for x in self.samples if x[1])
        if f:
            out["sclk_mhz_median"] = round(f[len(f) // 2])
        if self.cap_w:
            out["power_cap_w"] = round(self.cap_w, 1)
        return out


class ThrottleProbe:
    """What limits the shader clock during the timed steps: the SMU's violation accumulators of GPU `index`, read through the amdsmi
    python binding (amdsmi_get_violation_status: PPT power, socket / VR / HBM thermal, PROCHOT, and "gfx clock below the host limit because of power / thermal"
    per XCD) once before and once after the region; the line reports each accumulator's growth as a share of the region's accumulator ticks, plus hotspot /
    HBM temperature and the gfx clock of every XCD at the end of the region.  Best effort: nothing is reported where the binding or the driver lacks it."""

    ACC = ("acc_ppt_pwr", "acc_socket_thrm", "acc_vr_thrm", "acc_hbm_thrm", "acc_prochot_thrm", "acc_gfx_clk_below_host_limit")
    ACC_XCP = ("acc_gfx_clk_below_host_limit_pwr", "acc_gfx_clk_below_host_limit_thm", "acc_gfx_clk_below_host_limit_total", "acc_low_utilization")

    def __init__(self, index: int):
        self.h, self.smi, self.before, self.err = None, None, None, None
        try:
            import ctypes

            import amdsmi

            hip, buf = ctypes.CDLL("libamdhip64.so"), ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, int(index)) != 0:
                raise OSError("hipDeviceGetPCIBusId failed")
            bdf = buf.value.decode().lower()
            amdsmi.amdsmi_init()
            self.smi = amdsmi
            for h in amdsmi.amdsmi_get_processor_handles():
                if amdsmi.amdsmi_get_gpu_device_bdf(h).lower() == bdf:
                    self.h = h
            if self.h is None:
                self.err = f"no amdsmi device with bdf {bdf}"
        except Exception as e:  # noqa: BLE001 -- a missing binding / driver interface must never break a measurement
            self.err = f"{type(e).__name__}: {e}"[:200]

    def _read(self):
        try:
            return self.smi.amdsmi_get_violation_status(self.h)
        except Exception as e:  # noqa: BLE001
            self.err = f"{type(e).__name__}: {e}"[:200]
            return None

    def __enter__(self):
        if self.h is not None:
            self.before = self._read()
        return self

    def __exit__(self, *a):
        self.after = self._read() if self.before is not None else None
        self.metrics = None
        if self.h is not None:
            try:
                self.metrics = self.smi.amdsmi_get_gpu_metrics_info(self.h)
            except Exception as e:  # noqa: BLE001
                self.err = f"{type(e).__name__}: {e}"[:200]
        return False

    @staticmethod
    def _num(v):
        return v if isinstance(v, (int, float)) and not isinstance(v, bool) else None

    def summary(self):
        out = {}
        b, a = self.before, getattr(self, "after", None)
        if b and a:
            ticks = (self._num(a.get("acc_counter")) or 0) - (self._num(b.get("acc_counter")) or 0)
            out["accumulator_ticks"] = ticks
            share = {}
            for k in self.ACC:
                x, y = self._num(b.get(k)), self._num(a.get(k))
                if x is not None and y is not None:
                    share[k[4:]] = round((y - x) / ticks, 4) if ticks > 0 else (y - x)
            for k in self.ACC_XCP:  # per-XCP lists of per-XCD lists (or "N/A")
                try:
                    d = [yy - xx for xr, yr in zip(b[k], a[k]) for xx, yy in zip(xr, yr) if self._num(xx) is not None and self._num(yy) is not None]
                except (KeyError, TypeError):
                    d = []
                if d:
                    share[k[4:] + "_max_over_xcd"] = round(max(d) / ticks, 4) if ticks > 0 else max(d)
            out["share_of_region"] = share
            out["active_at_end"] = sorted(k[7:] for k, v in a.items() if k.startswith("active_") and v is True)
            grown = {k: v for k, v in share.items() if isinstance(v, (int, float)) and v > 0.02}
            out["limiter"] = max(grown, key=grown.get) if grown else "none of the SMU's violation accumulators grew during the region"
        m = getattr(self, "metrics", None)
        if m:
            for k in ("temperature_hotspot", "temperature_mem", "temperature_vrsoc", "current_socket_power", "average_gfx_activity", "average_umc_activity", "throttle_status", "indep_throttle_status",
                      "current_uclk"):
                if self._num(m.get(k)) is not None:
                    out[k] = m[k]
            g = [x for x in (m.get("current_gfxclks") or m.get("current_gfxclk") or []) if self._num(x) is not None and 0 < x < 10000] if isinstance(m.get("current_gfxclks") or m.get("current_gfxclk"), (list, tuple)) else []
            if g:
                out["gfxclk_mhz_per_xcd_at_end"] = g
        if self.err and not out:
            out["unavailable"] = self.err
        return out or None


def _respawn_under_torchrun(n: int):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run --nproc-per-node N bench.py <same flags>`
    (one rank per GPU over RCCL) instead of silently measuring one rank."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {n} without a launcher environment: running {' '.join(cmd)}", file=sys.stderr)
    sys.exit(subprocess.call(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", default="vgg_heads_l")
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step")
    ap.add_argument("--image-size", type=int, default=640)
    ap.add_argument("--heads-per-image", type=float, default=3.0)
    ap.add_argument("--full", action="store_true", help="also run everything beyond the headline: secondary workloads, FLAME decode sweep, overlap check, power / throttle "
                    "sampling, live PMC traffic, cpu_baseline and the deviation reports (the --no-* switches below then drop parts of it)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps write the detections of the last timed forward as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the (untimed) deviation reports of the bf16 / parity modes")
    ap.add_argument("--no-overlap-check", action="store_true", help="skip the untimed overlapped-vs-serial post-stage check before the timed steps (N = 1 only)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the separately timed secondary workloads (M b32, L @1280 crowd, parity modes)")
    ap.add_argument("--per-layer", default=None, help="write a per-op timing table (json) to this path")
    ap.add_argument("--split", type=int, default=2, help="independent sub-batches per forward on the net's lane streams (1 = off)")
    ap.add_argument("--overlap", action="store_true", help="force the post-stage overlap on (default: on for batch >= 8)")
    ap.add_argument("--no-overlap", action="store_true", help="run NMS..FLAME decode on the network stream instead of the detector's (lowest-priority) side stream")
    ap.add_argument("--graph", action="store_true", help="replay the network through a captured hipGraph")
    ap.add_argument("--exchange", action="store_true", help="run the N>1 step (output slots + RCCL gather to rank 0 on the communication stream) even with one rank")
    ap.add_argument("--tuning", default=None, help="tile table to load instead of head_detector_amd/tuning/conv_cfg.json")
    ap.add_argument("--precision", default="bf16", help="activation format of the main workload (bf16 = the headline; fp16x3 / fp32 are the parity modes)")
    ap.add_argument("--traffic", default=None, choices=["auto", "live", "file", "off"], help="roofline.traffic: PMC passes run by this script (live), the committed profile (file); "
                    "default auto with --full, off without")
    ap.add_argument("--inner", type=int, default=8, help="forwards (engine calls over one resident batch each) per timed step: the driver's 20-step run then times "
                    "> 2 s instead of 0.27 s, i.e. one clock / power state covers the region; ms_per_step is per step, config.ms_per_forward per forward")
    ap.add_argument("--dry-run-cpu", action="store_true", help="N>1 first-contact kit without GPUs: this script's step closure + DetectionGatherer on gloo ranks with a stand-in "
                    "engine (tools/dryrun_dist.py); --compact-gather selects the packed-rows exchange")
    ap.add_argument("--compact-gather", action="store_true", help="N>1: send packed survivor rows (DetectionGatherer(compact_rows=...)) instead of the [B, keep, 418] capacity slab")
    ap.add_argument("--ramp-steps", type=int, default=30, help="untimed steps before the W warm-up steps (clock ramp of a cold box; 0 = off)")
    args = ap.parse_args()
    if args.traffic is None:
        args.traffic = "auto" if args.full else "off"
    if args.dry_run_cpu:  # control flow of the N>1 step on CPU ranks (no GPU, no kernels, no measurement): tools/dryrun_dist.py
        sys.path.insert(0, os.path.join(ROOT, "tools"))  # spawn'ed ranks inherit sys.path and import the module by name
        import dryrun_dist as mod

        sys.exit(mod.main(["--gpus", str(max(args.gpus, 2)), "--steps", str(max(6, min(args.steps, 20)))] + (["--compact"] if args.compact_gather else [])))
    leaked = sorted(k for k in os.environ if k.startswith("VGH_"))
    if leaked:
        sys.exit(f"bench.py: refusing to measure with experiment switches in the environment: {leaked}")
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        _respawn_under_torchrun(args.gpus)

    import torch
    import torch.distributed as dist

    from head_detector_amd import _lib, arch
    from head_detector_amd.dist import DetectionGatherer, init_from_env, steer_collective_stream
    from head_detector_amd.engine import VGHeadsEngine
    from head_detector_amd.flame import FLAMELayer
    from head_detector_amd.synthetic import synthetic_flame_model

    rank, world, local = init_from_env(single_rank_group=args.exchange)
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; launch with --nproc-per-node {args.gpus} (or without a launcher: the script spawns the ranks itself)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    _lib.load()
    S = args.image_size
    flame_model = synthetic_flame_model(seed=3)
    flame = FLAMELayer(model=flame_model, device=dev, max_heads=max(4096, max(args.batch, 32) * 100, 256 * 64))  # 256 * 64: the b256 @1280 crowd leg decodes ~40 heads per image
    nsplit = 1 if args.graph else max(1, min(4, args.split))

    steered = [False]

    def run_workload(variant: str, B: int, steps: int, warmup: int, per_layer_path=None, image_size: int = S, heads_per_image: float = args.heads_per_image,
                     precision: str = "bf16", inner: int = 1, dump_dir=None) -> dict:
        """The timed region of the contract for one (variant, batch): W warm-up steps, barrier + synchronize, K steps, synchronize +
        barrier, max over ranks.  HIP events on the engine's stream bracket the network part of every timed step."""
        # post stages of batch s under the network of batch s+1: pays from batch 8 up (measured r02: 2.89 vs 2.95 ms at B=8, 13.25 vs 13.42 at B=64), costs
        # at B=1 (2.2 vs 1.9 ms: the network itself is a chain of small latency-bound kernels there)
        overlap = (args.overlap or (B >= 8 and not args.no_overlap)) and not args.graph
        eng = VGHeadsEngine(variant, image_size=image_size, max_batch=B, seed=1, precision=precision)
        if args.tuning:
            eng.load_tuning(args.tuning)
        # synthetic images, seed 0 (+rank): u8 NHWC resident in HBM (what the letterbox stage hands over, detector.py:48-51)
        images = torch.randint(0, 256, (B, image_size, image_size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(rank)).to(dev)
        unpad = torch.tensor([[0.0, 0.0, 1.0]], device=dev).expand(B, 3).contiguous()
        # calibrate the confidence threshold once (untimed): ~heads_per_image survivors per image
        _, scores, _ = eng.model(images)
        torch.cuda.synchronize()
        lo, hi = float(scores.min()), float(scores.max())
        conf = hi
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            mean_heads = float(eng.detect(images, confidence_threshold=mid).counts.float().mean())
            conf = mid
            if mean_heads > heads_per_image:
                lo = mid
            else:
                hi = mid
            if abs(mean_heads - heads_per_image) < max(0.25, 0.05 * heads_per_image):
                break
        nfw = steps * inner  # forwards in the timed region
        ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(nfw)]
        ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(nfw)]
        n_heads_all = torch.zeros(max(nfw, 1), dtype=torch.int32, device=dev)
        # throughput mode: NMS .. FLAME decode of batch s run on the detector's side stream underneath the network of batch s+1
        eng.set_overlap(overlap)
        eng.set_split(nsplit)
        if args.tuning:
            eng.load_tuning(args.tuning)

        # N>1: the detections of every rank go to rank 0 -- fixed-capacity slabs allocated once, two output slots, collectives queued
        # on a communication stream behind the detector's side stream: the gather of batch s runs under the network of batch s+1 and
        # nothing in the steady-state loop waits on the host (head_detector_amd/dist.py::DetectionGatherer)
        slots = gat = ready = None
        if world > 1 or args.exchange:
            NSLOTS = 3
            slots = [eng.new_output_slot(flame) for _ in range(NSLOTS)]
            gat = DetectionGatherer(B, eng.keep_k, flame.num_vertices, vertex_rows=B * int(1.5 * heads_per_image + 1), device=dev, dst=0, stream=eng.acquire_stream(),
                                    always_collective=args.exchange, compact_rows=B * int(1.5 * heads_per_image + 1) if args.compact_gather else 0, slots=NSLOTS)
            ready = [torch.cuda.Event() for _ in range(NSLOTS)]
            if gat.collective and not steered[0]:
                # RCCL launches its kernels on a stream of torch's pool; on the hardware queue of the engine stream or of a lane they would
                # hold up the next batch's network (a queue is in-order).  Steer the pool before the first collective, then measure.
                steered[0] = True
                ok = steer_collective_stream(eng.streams_in_use())
                print(f"[bench] rank {rank}: collective stream {'clear of' if ok else 'SHARES a hardware queue with'} the engine's streams", file=sys.stderr)
        step = make_step(eng, flame, images, unpad, conf, B, slots, gat, overlap, args.graph, n_heads_all, ev0, ev1, ready)

        for _ in range(args.ramp_steps):  # untimed: a cold box needs a few hundred ms of load before its clocks settle
            step()
        for _ in range(warmup * inner):
            step()
        # Overlap report (untimed).  r05 found engines whose low-priority side stream was STARVED (every forward stalled 2.5 - 3 ms at the prediction guard) and worked around it
        # here by timing both modes and keeping the faster.  r06 found the mechanism -- the side stream's hardware queue shared a compute pipe with the caller's stream or a
        # lane (csrc/streams.hip::blocked_behind, profiles/r06_starved_side_stream_classes.txt) -- and the library now acquires the side stream clear of those pipes, so the
        # workaround is gone: the overlap stays on; both timings and the pipe test are only REPORTED (config.*.overlap_check), so that a regression would be seen, not hidden
        overlap_check = None
        if args.full and overlap and world == 1 and not args.no_overlap_check:
            def probe(n=4 * max(inner, 2)):
                eng.join()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(n):
                    step()
                eng.join()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / n * 1e3
            on_ms = probe()
            eng.set_overlap(False)
            off_ms = probe()
            eng.set_overlap(True)
            for _ in range(2):
                step()
            st_ = eng.streams_in_use()
            hol = [int(eng.lib.vgh_stream_blocked_behind(a.cuda_stream, st_[-1].cuda_stream)) for a in st_[:-1]] if len(st_) > 1 else []
            overlap_check = dict(ms_per_forward_overlapped=round(on_ms, 3), ms_per_forward_serial_post_stages=round(off_ms, 3), chosen="overlapped",
                                 side_stream_blocked_behind_main_and_lanes=hol)
            if off_ms < 0.97 * on_ms or any(hol):
                print(f"[bench] WARNING {variant} {precision} b{B}: the overlapped post stages are slower than serial ones ({on_ms:.3f} vs {off_ms:.3f} ms per forward, pipe test {hol}): "
                      "a starved side stream -- the library's stream acquisition should have prevented this", file=sys.stderr)
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()
        with ThrottleProbe(local) if args.full else contextlib.nullcontext() as throttle, PowerSampler(local) if args.full else contextlib.nullcontext() as power:
            t0 = time.perf_counter()
            for i in range(nfw):  # K steps of `inner` forwards each
                det = step(i)
            step.flush()  # the exchanges of the last two batches
            eng.join()
            last_exchanges = []
            if gat is not None:
                for s in range(len(slots)):
                    last_exchanges.append(gat.result(s))  # the exchanges still in flight
            torch.cuda.synchronize()
            if dist.is_initialized():
                dist.barrier()
            dt = time.perf_counter() - t0
        dt_local, per_rank = dt, None
        if dist.is_initialized():
            t = torch.tensor([dt], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t)
            # every rank's own clock around the same region and the rank count the collective itself saw (an all_reduce of ones): what the driver's
            # "did RCCL see N ranks / does N = 1 agree with BENCH" checks read straight off the line
            allt = [torch.zeros(1, device=dev) for _ in range(world)]
            dist.all_gather(allt, torch.tensor([dt_local], device=dev))
            ones = torch.ones(1, device=dev)
            dist.all_reduce(ones)
            per_rank = {"seconds": [round(float(x), 6) for x in allt], "images_per_sec": [round(B * nfw / float(x), 2) for x in allt], "ranks_seen_by_all_reduce": int(ones.item()),
                        "backend": dist.get_backend()}
        # compact exchange: a crowded batch beyond the fixed row cap is CUT (counts clamped, dist.py) -- a measurement that dropped detections must say so
        dropped = sum(int(o.dropped_rows_per_rank.sum()) for o in last_exchanges if o is not None and o.dropped_rows_per_rank is not None)
        if dropped:
            print(f"[bench] WARNING: the compact exchange cut {dropped} survivor rows at its cap in the last two steps", file=sys.stderr)
        net_ms = sum(a.elapsed_time(b) for a, b in zip(ev0, ev1)) / max(nfw, 1)  # per forward
        heads = int(n_heads_all.sum().item())
        if dump_dir and rank == 0:
            dump_detections(det, dump_dir)
        if per_layer_path and rank == 0:
            eng.join()
            eng.set_split(1)  # per-op events make sense on one stream only: the table is the single-stream view of every op
            json.dump(eng.profile_ops(images, repeats=7), open(per_layer_path, "w"), indent=0)  # per-op median of 7 profiled forwards
        alg = arch.program_algorithmic_bytes(eng.program, B, fused_stem=eng.stem_fused and images.dtype == torch.uint8)  # (the stem tensor does not exist when its conv runs inside the stage-1 pair's launch)
        fp8_flops = 2.0 * sum(op["macs"] for op in eng.program.ops if arch.op_touches_fp8(eng.program, op) and eng.program.bufs[op["in_buf"]]["is_f32"] in arch.Q8_FMTS)
        out = dict(variant=variant, B=B, steps=steps, warmup=warmup, dt=dt, net_ms=net_ms, fp8_flops_per_image=fp8_flops, fp8_links=sum(bf["is_f32"] in arch.Q8_FMTS for bf in eng.program.bufs), heads_per_img=heads / max(nfw * B, 1), overlap=overlap, inner=inner,
                   value=B * world * nfw / dt, flops_per_image=eng.flops_per_image, conv_tflops=eng.flops_per_image * B / (net_ms * 1e-3) / 1e12,
                   alg_bytes=alg["read"] + alg["write"], arena_batch=eng.arena_batch, power=power.summary() if power else None, exchange_dropped_rows=dropped, per_rank=per_rank,
                   overlap_check=overlap_check)
        thr = throttle.summary() if throttle else None
        if thr and out["power"] is not None:
            out["power"]["throttle"] = thr
        elif thr:
            out["power"] = {"throttle": thr}
        eng.close()
        return out

    def one_image_latency(variant: str, calls: int = 150) -> dict:
        """Wall time of detect() on ONE image including the host wait for its result (network, top-k / NMS, FLAME decode of the survivors; u8 image resident
        in HBM): what a caller of HeadDetector.__call__ sees per image after the letterbox.  Median / min over `calls` synchronous calls."""
        eng = VGHeadsEngine(variant, image_size=S, max_batch=1, seed=1)
        img = torch.randint(0, 256, (1, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).to(dev)
        unp = torch.tensor([[0.0, 0.0, 1.0]], device=dev)
        _, sc, _ = eng.model(img)
        conf = float(sc[0, 2, 0])  # the three best candidates pass the threshold
        for _ in range(20):
            eng.detect(img, confidence_threshold=conf, flame=flame, unpad=unp)
        torch.cuda.synchronize()
        out = {"calls": calls}
        for graph in (False, True):  # the network as ~135 launches, or replayed through a captured hipGraph (detect(use_graph=True))
            for _ in range(10):
                eng.detect(img, confidence_threshold=conf, flame=flame, unpad=unp, use_graph=graph)
            torch.cuda.synchronize()
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                d = eng.detect(img, confidence_threshold=conf, flame=flame, unpad=unp, use_graph=graph)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                out["heads_decoded"] = int(d.num_heads)
            ts.sort()
            sfx = "_graph" if graph else ""
            out["ms_median" + sfx], out["ms_min" + sfx] = round(ts[len(ts) // 2], 3), round(ts[0], 3)
        eng.close()
        out["images_per_sec_at_median"] = round(1e3 / min(out["ms_median"], out["ms_median_graph"]), 1)
        return out

    def brief(m: dict) -> dict:
        return {"images_per_sec": round(m["value"], 2), "ms_per_step": round(m["dt"] / m["steps"] * 1e3, 3), "net_ms_per_step": round(m["net_ms"] * m.get("inner", 1), 3),
                "conv_tflops": round(m["conv_tflops"], 2), "roofline_frac": round(m["conv_tflops"] / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "steps": m["steps"],
                "heads_per_image_decoded": round(m["heads_per_img"], 2), **({"overlap_check": m["overlap_check"]} if m.get("overlap_check") else {})}

    main_run = run_workload(args.variant, args.batch, args.steps, args.warmup, args.per_layer, precision=args.precision, inner=max(1, args.inner), dump_dir=args.dump_outputs)
    B = args.batch

    # FLAME decode alone (second headline metric): us per head at n = 96 (all 400 coefficients), straight through the C ABI with preallocated outputs -- the
    # facade's torch.empty + ctypes marshalling (~20 us of host time per call) would otherwise be what the events see now that a call is ~40 us of GPU time
    from head_detector_amd import _lib as _vl

    def decode_us(n_heads: int, iters: int = 200) -> float:
        p = torch.randn(n_heads, 413, device=dev)
        proj = torch.empty(n_heads, flame.num_vertices, 3, device=dev)
        rot = torch.empty(n_heads, 3, 3, device=dev)
        h, st, lib = flame._need_handle(), torch.cuda.current_stream().cuda_stream, _vl.load()
        call = lambda: _vl.check(lib.vgh_flame_decode(h, p.data_ptr(), n_heads, 300, 100, None, None, rot.data_ptr(), proj.data_ptr(), st))  # noqa: E731
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    decode_sweep = {f"n{k}": round(decode_us(k), 2) for k in (1, 8, 32, 96, 512, 1024)} if args.full else None

    if rank == 0:
        inner = main_run["inner"]
        config = {"workload": f"{args.variant} {args.precision} batch {B}/GPU @ {S}x{S}, u8 NHWC input resident in HBM, ~{main_run['heads_per_img']:.2f} heads/img decoded; "
                              f"one step = {inner} forwards of that batch back to back ({inner * B} images per GPU per step)",
                  "global_batch": B * world, "forwards_per_step": inner, "images_per_step": inner * B * world,
                  "ms_per_forward": round(main_run["dt"] / (args.steps * inner) * 1e3, 3), "net_ms_per_forward": round(main_run["net_ms"], 3), "image_size": S, "parallelism": f"dp{world}", "gflop_per_image": round(main_run["flops_per_image"] / 1e9, 2),
                  "graph": bool(args.graph), "exchange_to_rank0": bool(world > 1 or args.exchange), "overlap_post": main_run["overlap"], "batch_split": nsplit,
                  "net_ms_per_step": round(main_run["net_ms"] * inner, 3), "ramp_steps": args.ramp_steps}
        if decode_sweep:
            config.update(flame_decode_us_per_head_n96=round(decode_sweep["n96"] / 96, 3), flame_decode_us_per_call_all400=decode_sweep)
        if main_run["overlap_check"]:
            config["overlap_check"] = main_run["overlap_check"]  # untimed report: overlapped vs serial post stages on this engine + the pipe test of its side stream (the overlap stays on)
        if main_run["power"]:
            config["power_during_timed_steps"] = main_run["power"]
        if main_run["per_rank"]:
            config["per_rank"] = main_run["per_rank"]  # each rank's own images/sec over the timed region; `value` = all images / the slowest rank's time
        if main_run["exchange_dropped_rows"]:
            config["exchange_dropped_rows"] = main_run["exchange_dropped_rows"]
        sec_steps = max(50, args.steps // 2)
        if args.full and world == 1 and not args.no_secondary:
            if (args.variant, B) != ("vgg_heads_m", 32):
                m = run_workload("vgg_heads_m", 32, sec_steps, args.warmup)
                config["secondary_vgg_heads_m_b32"] = brief(m)
                print(f"[bench] BASELINE configs[1] vgg_heads_m bf16 batch 32 @ {S}: {m['value']:.1f} img/s, {m['dt'] / m['steps'] * 1e3:.3f} ms/step, "
                      f"net {m['net_ms']:.3f} ms = {m['conv_tflops']:.1f} TFLOP/s ({m['conv_tflops'] / MFMA_BF16_DENSE_PEAK_TFLOPS:.3f} of the bf16 MFMA peak)", file=sys.stderr)
            # BASELINE configs[4]: 1280 x 1280 crowd images (>= 32 heads per image survive NMS and are decoded), 33 600 anchors per image
            m = run_workload("vgg_heads_l", 16, max(20, sec_steps // 4), max(3, args.warmup // 2), image_size=1280, heads_per_image=40.0)
            config["secondary_vgg_heads_l_b16_1280_crowd"] = dict(brief(m), gflop_per_image=round(m["flops_per_image"] / 1e9, 2), anchors_per_image=33600)
            print(f"[bench] BASELINE configs[4] vgg_heads_l bf16 batch 16 @ 1280 crowd: {m['value']:.1f} img/s, {m['heads_per_img']:.1f} heads/img decoded, "
                  f"net {m['net_ms']:.3f} ms = {m['conv_tflops']:.1f} TFLOP/s", file=sys.stderr)
            # ... and at BASELINE's stated batch (r06): 256 crowd images through the chunked arena (a 1280 activation tensor passes 2 GiB beyond 27 images: 9 x 27 + 13)
            m = run_workload("vgg_heads_l", 256, 4, 1, image_size=1280, heads_per_image=40.0)
            config["secondary_vgg_heads_l_b256_1280_crowd"] = dict(brief(m), gflop_per_image=round(m["flops_per_image"] / 1e9, 2), anchors_per_image=33600, arena_chunks="9 x 27 + 13 images")
            print(f"[bench] BASELINE configs[4] at its stated batch: vgg_heads_l bf16 batch 256 @ 1280 crowd: {m['value']:.1f} img/s, {m['heads_per_img']:.1f} heads/img decoded, "
                  f"net {m['net_ms']:.3f} ms = {m['conv_tflops']:.1f} TFLOP/s", file=sys.stderr)
            # the parity modes, timed by the same loop: fp16x3 on the matrix cores (csrc/conv_split.hip) and the fp32 VALU kernel
            pm = run_workload(args.variant, 32, max(20, sec_steps // 4), max(3, args.warmup // 2), precision="fp16x3")
            pv = run_workload(args.variant, 8, 10, 2, precision="fp32")
            config["parity_mode"] = {
                "dtype": "fp16x3: two fp16 planes per value, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulate (outputs within IoU >= 0.999 / 1e-4 of the fp32 oracle: "
                         "tests/test_gpu_split.py::test_fp16x3_matrix_core_mode_meets_north_star_tolerances)",
                "workload": f"{args.variant} fp16x3 batch 32 @ {S}", **brief(pm), "effective_conv_tflops": round(pm["conv_tflops"], 2),
                "mfma_tflops_issued": round(3 * pm["conv_tflops"], 2), "north_star_target_images_per_sec_per_gpu": NORTH_STAR_IMG_PER_S_PER_GPU,
                "meets_throughput_target": bool(pm["value"] >= NORTH_STAR_IMG_PER_S_PER_GPU),
                "fp32_valu_mode": {"workload": f"{args.variant} fp32 (v_fma_f32, csrc/conv_f32.hip) batch 8 @ {S}", **brief(pv)}}
            print(f"[bench] parity mode fp16x3 {args.variant} batch 32 @ {S}: {pm['value']:.1f} img/s (target {NORTH_STAR_IMG_PER_S_PER_GPU:.0f}/GPU), net {pm['net_ms']:.3f} ms; "
                  f"fp32 VALU mode batch 8: {pv['value']:.1f} img/s", file=sys.stderr)
            # N4 (r05): the "fp8" mode -- bf16 with OCP-e4m3 links between 3x3 / stride-1 convs (csrc/conv_pp.hip) -- timed by the same loop.  Its roof is MIXED: the
            # convs that read an e4m3 link are priced at the 5 PFLOP/s fp8 peak, everything else at the bf16 peak
            f8 = run_workload(args.variant, B, max(20, sec_steps // 2), max(3, args.warmup // 2), precision="fp8", inner=max(1, args.inner))
            f8_fl, all_fl = f8["fp8_flops_per_image"] * B, f8["flops_per_image"] * B
            ideal_ms = (f8_fl / (MFMA_FP8_DENSE_PEAK_TFLOPS * 1e12) + (all_fl - f8_fl) / (MFMA_BF16_DENSE_PEAK_TFLOPS * 1e12)) * 1e3
            config["experimental_fp8_links"] = dict(
                brief(f8), status=EXPERIMENTAL_8BIT, workload=f"{args.variant} fp8 links batch {B} @ {S}", e4m3_link_tensors=f8["fp8_links"], share_of_flops_on_fp8_mfma=round(f8_fl / all_fl, 4),
                roofline_frac_vs_mixed_roof=round(ideal_ms / f8["net_ms"], 4), mixed_roof_ms_per_forward=round(ideal_ms, 3), speedup_vs_bf16_headline=round(f8["value"] / main_run["value"], 4),
                note="roofline_frac above is against the bf16 peak (algorithmic FLOPs / time / 2.5 PF), roofline_frac_vs_mixed_roof prices the e4m3-input convs at 5 PF; "
                     "activation scales calibrated on two seeded random images; deviation from the oracle: modes_vs_oracle_one_image.fp8")
            print(f"[bench] (experimental) fp8 links {args.variant} batch {B} @ {S}: {f8['value']:.1f} img/s ({f8['value'] / main_run['value']:.3f} x the bf16 headline), net {f8['net_ms']:.3f} ms, "
                  f"{100 * f8_fl / all_fl:.1f} % of the FLOPs on the fp8 MFMA, {ideal_ms / f8['net_ms']:.3f} of the mixed roof", file=sys.stderr)
            # r05: the "int8" mode -- the same links as signed bytes (the reference exporter's QuantizationMode.INT8: exportable_mesh_model.py:175-178,398-411), v_mfma_i32_32x32x32_i8,
            # with the folded identity branch of the RepVGG convs applied in fp32 (diagonal bypass, csrc/conv_pp.hip DG).  No spec peak for int8 in the guide ("2 x the bf16 rate"):
            # the mixed roof prices the int8-input convs at 5 POP/s like the fp8 ones
            i8 = run_workload(args.variant, B, max(20, sec_steps // 2), max(3, args.warmup // 2), precision="int8", inner=max(1, args.inner))
            i8_fl = i8["fp8_flops_per_image"] * B
            ideal8 = (i8_fl / (MFMA_FP8_DENSE_PEAK_TFLOPS * 1e12) + (all_fl - i8_fl) / (MFMA_BF16_DENSE_PEAK_TFLOPS * 1e12)) * 1e3
            config["experimental_int8_links"] = dict(
                brief(i8), status=EXPERIMENTAL_8BIT, workload=f"{args.variant} int8 links batch {B} @ {S}", int8_link_tensors=i8["fp8_links"], share_of_flops_on_int8_mfma=round(i8_fl / all_fl, 4),
                roofline_frac_vs_mixed_roof=round(ideal8 / i8["net_ms"], 4), mixed_roof_ms_per_forward=round(ideal8, 3), speedup_vs_bf16_headline=round(i8["value"] / main_run["value"], 4),
                note="as experimental_fp8_links with int8 codes (scale = calibrated max * 1.25 / 127) and the diagonal bypass on the RepVGG cv2 convs; deviation from the oracle: "
                     "modes_vs_oracle_one_image.int8 (about 2.5 x the bf16 mode's, less than half of the e4m3 links')")
            print(f"[bench] (experimental) int8 links {args.variant} batch {B} @ {S}: {i8['value']:.1f} img/s ({i8['value'] / main_run['value']:.3f} x the bf16 headline), net {i8['net_ms']:.3f} ms, "
                  f"{ideal8 / i8['net_ms']:.3f} of the mixed roof", file=sys.stderr)
            # r05: the single-plane fp16 mode (the reference's own FP16 export format: exportable_mesh_model.py:177,299,409) -- same bytes and MFMA count as bf16
            fh = run_workload(args.variant, B, max(20, sec_steps // 2), max(3, args.warmup // 2), precision="fp16", inner=max(1, args.inner))
            config["secondary_fp16"] = dict(brief(fh), workload=f"{args.variant} fp16 (one fp16 plane per value, v_mfma_f32_32x32x16_f16) batch {B} @ {S}", speed_vs_bf16_headline=round(fh["value"] / main_run["value"], 4),
                                            note="the fp16 split kernels with one K segment + the fp16 ping-pong tiles, per-op tile table tuned once (profiles/r05_tune_fp16_*.json); no streaming 1x1 / pipelined patch tiles in this "
                                                 "format yet, hence the gap to bf16; deviation from the oracle: modes_vs_oracle_one_image.fp16")
            print(f"[bench] fp16 {args.variant} batch {B} @ {S}: {fh['value']:.1f} img/s ({fh['value'] / main_run['value']:.3f} x the bf16 headline), net {fh['net_ms']:.3f} ms", file=sys.stderr)
            # BASELINE configs[0]'s shape on the GPU: ONE 640 x 640 image per call, the caller waits for the result (the reference's own API is single-image)
            config["latency_one_image_synchronous"] = {v: one_image_latency(v) for v in ("vgg_heads_l", "vgg_heads_m")}
        # roofline.traffic: HBM bytes of one forward of the main workload
        traffic = None
        if args.traffic in ("auto", "live") and world == 1 and S == 640 and args.precision == "bf16":
            traffic = live_traffic(args.variant, B, nsplit)
        if traffic is None and args.traffic in ("auto", "file") and S == 640:
            for name in (f"r04_traffic_{args.variant[-1]}{B}_x{nsplit}.json", f"r03_traffic_{args.variant[-1]}{B}_x{nsplit}.json"):
                tpath = os.path.join(ROOT, "profiles", name)
                if os.path.exists(tpath):
                    t = json.load(open(tpath))
                    traffic = dict(read_bytes_per_forward=t["read_bytes_per_forward"], write_bytes_per_forward=t["write_bytes_per_forward"], launches_per_forward=t["launches_per_forward"],
                                   source=f"committed PMC pass profiles/{name} (not this run)")
        roof = {"bound": "mfma", "achieved": round(main_run["conv_tflops"], 2), "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(main_run["conv_tflops"] / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "traffic": None,
                "algorithmic_bytes_per_forward": round(main_run["alg_bytes"]),
                "kernel": "conv3x3_pp_kernel<*> + conv_igemm_kernel<*> + conv3x3_patch_kernel<*> + conv3x3_patch3_kernel<*> + conv1x1_stream_kernel<*> + stem / pool (all launches of one forward = one pass of the op program over the batch: "
                          "algorithmic 2*MACs / HIP-event time of the network part; traffic = PMC HBM bytes of one forward)"}
        if traffic is not None:
            tb = traffic["read_bytes_per_forward"] + traffic["write_bytes_per_forward"]
            roof.update({"traffic": round(tb), "traffic_read_bytes": round(traffic["read_bytes_per_forward"]), "traffic_write_bytes": round(traffic["write_bytes_per_forward"]),
                         "traffic_over_algorithmic": round(tb / main_run["alg_bytes"], 3), "traffic_launches_per_forward": round(traffic["launches_per_forward"], 1),
                         "traffic_hbm_tbps_at_net_time": round(tb / (main_run["net_ms"] * 1e-3) / 1e12, 3), "traffic_source": traffic["source"]})
            print(f"[bench] roofline.traffic source: {traffic['source']}", file=sys.stderr)
        line = {
            "metric": "images/sec at 640x640 (VGGHeads forward path: net -> top-k/NMS -> FLAME decode)",
            "value": round(main_run["value"], 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(main_run["dt"] / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic", "config": config, "roofline": roof,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"], ref = cpu_baseline(args.variant, S, flame_model)
            if not args.no_accuracy and S == 640:
                # checker role of the oracle: every precision mode on the oracle's image (parity_mode.vs_oracle is what north_star's bar reads)
                dev_tab = {p: deviation_from_oracle(args.variant, p, ref, dev) for p in ("fp16x3", "fp32", "bf16x3", "bf16", "fp16", "fp8", "int8")}
                config.setdefault("parity_mode", {})["vs_oracle"] = dev_tab["fp16x3"]
                config["modes_vs_oracle_one_image"] = dev_tab
    # the line is the LAST thing on stdout: RCCL prints its version banner through C stdio, which (redirected to a file or a pipe) is block-buffered and would
    # otherwise be flushed at process exit, i.e. AFTER a line python has already written.  Every rank flushes its C and python buffers, then a barrier, then rank 0 prints
    import ctypes

    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
