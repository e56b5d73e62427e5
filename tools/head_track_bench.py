"""Head tracking: vght_track_frames alone, timed on seeded videos (tests/head_track_ref.py ``random_sequence``: heads drifting over a 1280 x 960 image, seen with
probability 0.85, false positives, scores on both sides of the thresholds), beside the NumPy restatement on this machine's CPU.

    frame_ms[n]       HIP events around ONE call of one frame (``tracking.track_frames``: the outputs and the workspace are allocated inside the events) on a table that
                      has seen --history frames, at n = 16 / 100 / 1 000 live heads (max_tracks 256 / 256 / 2 048, keep_k 100 / 200 / 2 048).  The state is put back
                      before every timed call, so every call does the same work.
    frame_cpu_ms[n]   one run of the restatement's vectorised form on the same frame and state; the device's outputs and state are compared BITWISE with it before
                      anything is timed.
    call64_ms         one call of 64 frames at 100 live heads from a fresh state; call64_cpu_ms the restatement on the same frames.

Medians over --iters after --warmup.

    python tools/head_track_bench.py [--iters 20] [--warmup 3] [--history 8] [--out profiles/head_track.txt]
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

import head_track_ref as ref  # noqa: E402

from head_detector_amd import tracking  # noqa: E402

FIELDS = dict(n_out="n_out", out_slot="slot", out_id="ids", out_det_row="det_row", out_hits="hits", out_misses="misses", out_box="boxes", out_score="scores",
              out_params="params", det_id="det_id", n_born="n_born", n_freed="n_freed", n_dropped="n_dropped")
STATE = dict(next_id="next_id", frame="frame", id="ids", hits="hits", misses="misses", age="age", det_row="det_row", score="scores", box="boxes", vel="vel", params="params")


def median_ms(fn, stream, warmup, iters, before=None):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for it in range(warmup + iters):
        if before:
            before()
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        ev[1].synchronize()
        if it >= warmup:
            out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


def check(out, state, want, want_state, what):
    bad = ref.same_bytes({k: getattr(out, name).cpu().numpy() for k, name in FIELDS.items()}, want, ref.OUTPUTS)
    assert bad is None, f"{what}: {bad}: the device differs from the restatement"
    bad = ref.same_bytes({k: getattr(state, name).cpu().numpy() for k, name in STATE.items()}, want_state, ref.STATE_FIELDS)
    assert bad is None, f"{what}: state {bad}: the device differs from the restatement"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--history", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_track_bench: needs the MI355X")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rule = dict(tracking.RULE_DEFAULTS, min_hits=2, max_age=5)
    line = {"rule": rule, "history": a.history}
    held = {}
    for live, M, K in ((16, 256, 100), (100, 256, 200), (1000, 2048, 2048)):
        H = a.history
        seq = ref.random_sequence(M, K, live, H + 1, seed=live)
        on_dev = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in seq[:4]]
        want_state, state = ref.new_state(M), tracking.TrackState(M, dev)
        ref.track(want_state, *[x[:H] for x in seq], "vec", **rule)
        tracking.track_frames(*[x[:H] for x in on_dev], seq[4][:H], state, **rule)
        torch.cuda.synchronize()
        saved = state.buffer.clone()
        last = [x[H:H + 1].contiguous() for x in on_dev]
        t0 = time.perf_counter()
        want = ref.track(want_state, *[x[H:H + 1] for x in seq], "vec", **rule)
        cpu_ms = (time.perf_counter() - t0) * 1e3

        def frame():
            held["f"] = tracking.track_frames(*last, seq[4][H:H + 1], state, **rule)

        frame()
        torch.cuda.synchronize()
        check(held["f"], state, want, want_state, f"{live} live")
        ms = median_ms(frame, stream, a.warmup, a.iters, before=lambda: state.buffer.copy_(saved))
        line[f"frame_ms[{live}]"], line[f"frame_cpu_ms[{live}]"] = ms, cpu_ms
        line[f"tracks[{live}]"], line[f"rows[{live}]"], line[f"reported[{live}]"] = int((want_state["id"] >= 0).sum()), int(seq[3][H]), int(want["n_out"][0])
    M, K, B = 256, 200, 64
    seq = ref.random_sequence(M, K, 100, B, seed=64)
    on_dev = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in seq[:4]]
    want_state, state = ref.new_state(M), tracking.TrackState(M, dev)
    t0 = time.perf_counter()
    want = ref.track(want_state, *seq, "vec", **rule)
    line["call64_cpu_ms"] = (time.perf_counter() - t0) * 1e3

    def call64():
        held["c"] = tracking.track_frames(*on_dev, seq[4], state, **rule)

    call64()
    torch.cuda.synchronize()
    check(held["c"], state, want, want_state, "64 frames")
    line["call64_ms"] = median_ms(call64, stream, a.warmup, a.iters, before=state.reset)
    line["bitwise_equal"] = True
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/head_track_bench.py --iters {a.iters} --warmup {a.warmup} --history {a.history}: vght_track_frames alone on seeded videos; ms are medians of "
                    "HIP-event times; *_cpu_ms = one run of the NumPy restatement (vectorised form) on the CPU\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
