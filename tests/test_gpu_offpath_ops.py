"""GPU (-m gpu): every op of the programs the benchmark NEVER runs, on the tiles the two selectors pick for them, against the plain reference of that one op.

tests/test_gpu_tuned_ops.py holds the nine benchmarked programs to program_ref.check_ops; all nine are 640 or 1280, forward full batches and (but for the latency engines)
run two lanes.  The selectors reach many other tiles, which the suite otherwise only compares with themselves (batch independence, raw against canvas route, lanes against
no lanes) -- a tile that is wrong the same way on both sides passes all of that.  Here, by the same procedure (tests/engine_case.py), program_ref.OFFPATH_CASES:

  * sizes the measured table has no entry for (352, 416, 480, 736; fp16 / fp16x3 away from their 640 prefixes): every conv on the class heuristic's tile (bf16) or the
    split pick rules' (fp16, fp16x3), on pyramids that are ragged against every tile shape (final maps 11 x 11, 13 x 13, 15 x 15, 23 x 23);
  * the (GEMM shape, tile) pairs the table selects for batch buckets, lane counts and sizes no benchmarked case has -- tests/test_host_logic.py holds the two case tables
    to EVERY pair of its sweep on the CPU;
  * a tuned engine given fewer images than max_batch (37 of 64 on two lanes: probes 18, 19, 36 = the last of lane 0, the first of lane 1, the last image; 1 of 32: the
    second lane is empty).  The images behind the forwarded batch must keep what an earlier full-batch forward left in every buffer, bit for bit.

Probes: never image 0 alone when B > 1; with two lanes the first image of lane 1 and the last image.  One line per case names the tile of every conv outside the fused
chains as engine.op_tiles() reports it (vgh_net_op_cfg: the SELECTION, also where the table has no entry; see its header comment for where a launch may still differ).  The off-table bf16 cases must have run a halo-patch ("p") tile, and every off-table
program holds a 3x3 / stride-1 conv on a map that is ragged in both directions (Ho % 8 != 0 and Wo % 8 != 0).  The split pick rules (csrc/conv_split.hip pick_split_cfg)
take a halo-patch tile only on maps that are whole multiples of 16 x 16 or 8 x 40: an fp16 / fp16x3 program is held to "a patch tile ran" exactly when it has such a map,
which the 352 and 416 pyramids do not -- so the automatic selection never runs a split halo-patch tile on a ragged map; only the forced tiles of tests/test_gpu_fp16.py do.

Tolerances: program_ref.op_tolerance; a bf16 chain at the single-op tolerance + 2 x the program's OWN measured floor (program_ref.chain_floor_for / CHAIN_FLOOR_MEASURED).

Seconds per case on an MI355X box (16 CPU threads for the reference), engine construction and CPU reference included: 0.6 - 3.4 s, and 6.5 / 7.6 s for the two 1280 fp16 cases on two lanes, see SECONDS_MEASURED.  The two 1280 fp16
cases on two lanes (l17_1280_fp16x2, m33_1280_fp16x2) forward 2 images of their 17 / 33, one per lane: with full batches their two-probe float64 references took 22 and 16 s.
A case with a forwarded batch is a partial-batch case (program_ref.PARTIAL_BATCH), so these two also run the full-arena forward and the tail check; their figures include it (2.0 / 1.2 s on the engine, 4.5 / 6.4 s for the one-probe float64 reference).
"""
import pytest

import program_ref as pr
from engine_case import family, run_case

pytestmark = pytest.mark.gpu

# wall seconds of each case on an MI355X box with 16 CPU threads (engine construction + forward(s) + copies + CPU reference), from this file's own "[offpath ops]" lines
SECONDS_MEASURED = {"m5_352x2": 1.0, "l3_416x1": 0.8, "l2_480": 0.8, "m20_736x2": 1.4, "m3_352_fp16x3": 0.7, "l3_416_fp16": 1.1, "l32_fp16x1": 1.7, "l32x1": 0.9, "m32x1": 0.6,
                    "m16x1": 0.6, "l8x1": 0.9, "l17x2": 1.2, "l4_1280x1": 2.7, "m4_1280x1": 1.8, "l8_320x1": 0.7, "m8_320x1": 0.6, "l1_320": 0.7, "m17_fp16x2": 3.4, "m33_320x1": 0.6,
                    "l17_fp16x3x1": 1.4, "l17_320_fp16x2": 1.8, "l17_320x2": 0.7, "m17_1280_fp16x3x1": 3.4, "m17_1280x1": 2.0, "m33_1280_fp16x2": 6.5, "l1_1280": 2.9,
                    "l17_320_fp16x3x1": 1.1, "m33_320_fp16x2": 1.2, "l33x1": 0.8, "l17_320x1": 0.8, "l33_320x2": 0.8, "l33_320_fp16x2": 1.8, "l17_1280_fp16x2": 7.6, "l64_fwd37": 2.1,
                    "m32_fwd1x2": 0.7}


def _probes(cid, B, lanes):
    """Never image 0 alone when B > 1.  Two lanes (csrc/net.hip: lane 0 takes the first ceil(B / lanes) images): the first image of lane 1 and the last image; a partial
    batch also the last image of lane 0 where that is not image 0 (the batch of 37: 18, 19, 36; a batch of 2: image 1 is both the first of lane 1 and the last)."""
    if B == 1:
        return [0]
    second_lane = (B + lanes - 1) // lanes
    if lanes == 1 or second_lane >= B:
        return [B - 1]
    return sorted({second_lane - 1, second_lane, B - 1} if cid in pr.PARTIAL_BATCH and second_lane > 1 else {second_lane, B - 1})


def _maps_3x3s1(P):
    return {(P.bufs[op["out_buf"]]["h"], P.bufs[op["out_buf"]]["w"]) for op in P.ops if op["kind"] == 1 and op["ksize"] == 3 and op["stride"] == 1}


@pytest.mark.parametrize("cid", list(pr.OFFPATH_CASES))
def test_engine_every_op_on_the_selections_the_benchmark_never_runs(gpu_lib, capfd, cid):
    r = run_case(cid, capfd, "[offpath ops]", lambda B, lanes: _probes(cid, B, lanes), floor=pr.chain_floor_for, keep_tail=cid in pr.PARTIAL_BATCH, check_getter=True)
    P, tiles, problems = r["P"], r["tiles"], r["problems"]
    if cid == "l64_fwd37":
        assert r["B"] == 37 and r["probes"] == [18, 19, 36]
    if cid in ("m33_1280_fp16x2", "l17_1280_fp16x2"):
        assert r["B"] == 2 and r["probes"] == [1]
    if cid == "m32_fwd1x2":
        assert r["B"] == 1 and r["probes"] == [0]
    if cid in pr.OFF_TABLE:
        assert not r["found"], "an off-table case takes no entry of the measured table"
        maps = _maps_3x3s1(P)
        assert any(h % 8 and w % 8 for h, w in maps), maps
        fams = {family(tiles[i]) for i in r["own"]}  # (the ops of the fused chains never launch on the tile named for them)
        if P.precision == "bf16":
            if "p" not in fams:
                problems.append(f"no halo-patch (p) tile ran: families {sorted(fams)}")
        elif any((h % 16 == 0 and w % 16 == 0) or (w % 40 == 0 and h % 8 == 0) for h, w in maps):
            if "sp" not in fams:
                problems.append(f"no halo-patch (sp) tile ran: families {sorted(fams)}")
    else:
        assert r["found"], "a table case looks entries up"
    assert not problems, f"{r['what']}: {len(problems)} problem(s):\n" + "\n".join(problems[:12])
