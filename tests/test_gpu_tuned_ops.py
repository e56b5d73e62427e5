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
import re
import time

import pytest
import torch

import program_ref as pr

pytestmark = pytest.mark.gpu

# wall seconds of each case on an MI355X box with 16 CPU threads (engine construction + forward + copies + CPU reference), from this file's own "[tuned ops]" lines
SECONDS_MEASURED = {"l64": 1.9, "m32": 1.2, "l8": 1.2, "l1": 1.2, "m1": 0.9, "l16_1280": 3.3, "l256_1280": 4.0, "l64_fp16": 2.2, "l32_fp16x3": 2.1}


def _probes(cid, B, lanes):
    """Probe images: the last one; for the two headline batches also the first image of the second lane (csrc/net.hip: lane 0 takes the first ceil(B / lanes) images)."""
    second_lane = (B + lanes - 1) // lanes
    return ([second_lane] if cid in ("l64", "m32") else []) + [B - 1] if B > 1 else [0]


def _family(name):
    return re.match(r"[a-z]*", name).group() or "igemm"  # plain implicit-GEMM tiles are named by their size


@pytest.mark.parametrize("cid", list(pr.TUNED_CASES))
def test_tuned_engine_every_op_at_the_benchmarked_shape(gpu_lib, capfd, cid):
    from collections import Counter

    from head_detector_amd import pack
    from head_detector_amd.engine import VGHeadsEngine

    t0 = time.perf_counter()
    variant, S, MB, lanes, prec = pr.TUNED_CASES[cid]
    dev = torch.device("cuda", torch.cuda.current_device())
    capfd.readouterr()
    eng = VGHeadsEngine(variant, image_size=S, max_batch=MB, seed=7, precision=prec)
    eng.set_split(lanes)
    P = eng.program
    problems = []

    # ---- the table applied as written
    found = pack.tile_names_for(P, MB, lanes)
    applied = eng.load_tuning()
    index = {n: i for i, n in enumerate(eng.cfg_names())}
    refused = [(P.ops[i]["name"], n) for i, n in found.items() if n not in index or not eng.cfg_ok(index[n], P.ops[i])]
    if applied != len(found) or refused:
        problems.append(f"load_tuning applied {applied} of the {len(found)} entries the table holds for this program; refused: {refused}")
    log = capfd.readouterr().err
    if "net_set_cfg" in log:
        problems.append("the library replaced table entries: " + " | ".join(sorted({ln for ln in log.splitlines() if "net_set_cfg" in ln})))
    convs = [i for i, op in enumerate(P.ops) if op["kind"] == 1]
    fam = Counter(_family(found[i]) if i in found else "library's choice" for i in convs)

    # ---- one forward of the benchmarked batch
    B = min(MB, eng.arena_batch)
    if cid == "l256_1280":
        assert B == 27  # a 1280 activation tensor passes 2 GiB beyond 27 images: the 256-image batch runs in arena chunks of this size
    probes = _probes(cid, B, lanes)
    assert probes != [0] or B == 1
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(S + B))
    eng.forward_net(x.to(dev))
    eng.stream.synchronize()
    chains = pr.fused_chains(P, eng.stem_fused)
    if prec == "bf16":
        assert len(chains) == eng.b2b_pairs >= 1 and eng.stem_fused and chains[0][0] == 0 and P.ops[0]["kind"] == 0
    else:
        assert chains == [] and not eng.stem_fused
    for ch in chains:  # never written, in ANY image of the batch
        for i in ch[:-1]:
            nz = int(torch.count_nonzero(eng.buffer(P.ops[i]["out_buf"], B)))
            if nz:
                problems.append(f"op {P.ops[i]['name']}: its output tensor lies inside a fused launch and must never be written; {nz} non-zero values")
    sel = torch.tensor(probes, device=dev)
    got = [eng.buffer(i, B)[sel].float().cpu() for i in range(len(P.bufs))]  # one buffer at a time, sliced on the device
    eng.close()
    t1 = time.perf_counter()

    # ---- every op against its reference
    w_all, b_all = P.arrays()
    if prec == "fp16":
        w_all = pr.fp16_weights(P, w_all)
    rep = pr.check_ops(P, got, x[probes], probes, prec, chains, found, w_all, b_all)
    n_ops = sum(op["kind"] in (0, 1, 2) for op in P.ops)
    with capfd.disabled():
        print(f"\n[tuned ops] {cid}: {applied} applied / {len(found)} looked up of {len(convs)} convs; tile families {dict(sorted(fam.items()))}; B {B} probes {probes}; "
              f"{rep['single']} ops singly + {rep['chained']} in {len(chains)} chains; {len(rep['failures'])} failures; engine + forward {t1 - t0:.1f} s, reference {time.perf_counter() - t1:.1f} s")
    assert rep["single"] + rep["chained"] == n_ops and rep["chained"] == sum(len(c) for c in chains)
    problems += [m for _, m in rep["failures"]]
    assert not problems, f"{cid} ({variant} @{S}, max_batch {MB}, {lanes} lane(s), {prec}): {len(problems)} problem(s):\n" + "\n".join(problems[:12])
