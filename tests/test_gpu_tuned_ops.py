"""GPU (-m gpu): every op of the BENCHMARKED programs, on the tiles tuning/conv_cfg.json picks for them, against the plain reference of that one op.

The number this project reports is a forward of the tuned engine: per conv a tile looked up by batch bucket, lane count and GEMM shape.  The other per-op checks
(test_network_every_op, test_fp16_network_every_op) run untuned or b1-bucket engines on maps of at most 64 pixels a side; the forced-tile tests run every tile on small
maps; the full-size tests compare an image in the batch with the same image alone ON THE SAME TILES, which a tile that is wrong in the same way for every image passes.
Here: the engine of each benchmarked workload (program_ref.TUNED_CASES; the lane counts are bench.py's: --split 2 for every timed workload, one stream for the
max_batch = 1 latency engines), one forward of the full batch in the default fusion mode, then every op's stored output for the probe images against
program_ref.run_op on the engine's OWN inputs of that op (no error accumulates across layers).  Image 0 alone is never the probe of a batch: the probes are the last
image and, for the two headline batches, the first image of the second lane.  The 9- and 13-wide SPP windows meet real borders here (20 x 20 / 40 x 40 maps).

Fused launches: the tensor between the ops of an arch.b2b_pairs pair, and for u8 input the stem tensor, are never written -- asserted to be all zero over the WHOLE
batch, so a change of the fusion set cannot hide -- and the group is checked as one reference chain (stem -> downsample -> conv1|conv2, bf16 between them) at the
last op's store segments, at the single-op tolerance + 2 x program_ref.CHAIN_FLOOR (measured on the CPU alone; tests/test_host_logic.py holds it against two
reference evaluations).  Tolerances are the project's own (program_ref.op_tolerance).  tests/test_host_logic.py plants faults into a reference forward and proves
that program_ref.check_ops names them.

The table applied as written: load_tuning must apply exactly the entries pack.tile_names_for finds, and the library must not replace any of them (its log line).

Seconds per case, measured on an MI355X box (16 CPU threads for the reference), engine construction and CPU reference included: 0.9 - 4.0 s, see SECONDS_MEASURED
(plus ~2 s of imports once per process).
"""
import pytest

import program_ref as pr
from engine_case import run_case

pytestmark = pytest.mark.gpu

# wall seconds of each case on an MI355X box with 16 CPU threads (engine construction + forward + copies + CPU reference), from this file's own "[tuned ops]" lines
SECONDS_MEASURED = {"l64": 1.9, "m32": 1.2, "l8": 1.2, "l1": 1.2, "m1": 0.9, "l16_1280": 3.3, "l256_1280": 4.0, "l64_fp16": 2.2, "l32_fp16x3": 2.1}


def _probes(cid, B, lanes):
    """Probe images: the last one; for the two headline batches also the first image of the second lane (csrc/net.hip: lane 0 takes the first ceil(B / lanes) images)."""
    second_lane = (B + lanes - 1) // lanes
    return ([second_lane] if cid in ("l64", "m32") else []) + [B - 1] if B > 1 else [0]


@pytest.mark.parametrize("cid", list(pr.TUNED_CASES))
def test_tuned_engine_every_op_at_the_benchmarked_shape(gpu_lib, capfd, cid):
    r = run_case(cid, capfd, "[tuned ops]", lambda B, lanes: _probes(cid, B, lanes))  # (tests/engine_case.py: the procedure, shared with tests/test_gpu_offpath_ops.py)
    if cid == "l256_1280":
        assert r["B"] == 27  # a 1280 activation tensor passes 2 GiB beyond 27 images: the 256-image batch runs in arena chunks of this size
    assert not r["problems"], f"{r['what']}: {len(r['problems'])} problem(s):\n" + "\n".join(r["problems"][:12])
