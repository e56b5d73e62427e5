"""TEST INFRASTRUCTURE (GPU): one case of program_ref.TUNED_CASES / OFFPATH_CASES run the way the benchmark runs an engine, every op judged by program_ref.check_ops.
Shared by tests/test_gpu_tuned_ops.py and tests/test_gpu_offpath_ops.py: build the engine, set_split, load_tuning, ONE forward of u8 images in the default fusion mode,
the buffers of the probe images, check_ops with fused_chains, the never-written tensors zero over the whole batch, no table entry replaced by the library."""
import re
import time
from collections import Counter

import torch

import program_ref as pr


def family(name):
    return re.match(r"[a-z]*", name).group() or "igemm"  # plain implicit-GEMM tiles are named by their size


def run_case(cid, capfd, tag, probes_of, floor=None, keep_tail=False, check_getter=False):
    """Runs case `cid`; probes_of(B, lanes) -> probe image indices.  keep_tail (cases that forward fewer images than the arena holds): a first forward of a FULL batch of
    other images fills every buffer, and the rows behind the forwarded batch must hold the same bits after the case's own forward.
    check_getter: hold engine.op_tiles() to "one name per conv" and to the table entries load_tuning applied (the off-path test; the benchmarked test asserts what it always did).
    Returns dict(problems=[...], rep=check_ops' report, tiles=engine.op_tiles(), found=the table's entries, P=program, B, probes, convs, own (the convs outside the fused chains), chains, n_ops, line=summary text).
    The asserts in here are about the case itself (its batch, its probes, its fusion set); what the engine computed goes into `problems`."""
    from head_detector_amd import pack
    from head_detector_amd.engine import VGHeadsEngine

    t0 = time.perf_counter()
    variant, S, MB, lanes, prec, fwd = pr.case_tuple(cid)
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
    fam = Counter(family(found[i]) if i in found else "library's choice" for i in convs)
    tiles = eng.op_tiles()
    if check_getter:
        assert sorted(tiles) == convs, "vgh_net_op_cfg names a tile for every conv and for nothing else"
        wrong = [(P.ops[i]["name"], n, tiles[i]) for i, n in found.items() if n in index and eng.cfg_ok(index[n], P.ops[i]) and tiles[i] != n]
        if wrong:
            problems.append(f"vgh_net_op_cfg names another tile than the table entry load_tuning applied: {wrong[:6]}")

    # ---- one forward of the case's batch
    full = min(MB, eng.arena_batch)
    B = full if fwd is None else fwd
    assert 1 <= B <= full
    probes = probes_of(B, lanes)
    assert probes != [0] or B == 1
    tails = None
    if keep_tail:
        assert B < full
        x0 = torch.randint(0, 256, (full, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(S + full + 1))
        eng.forward_net(x0.to(dev))
        eng.stream.synchronize()
        tails = [eng.buffer(i, full)[B:].clone() for i in range(len(P.bufs))]
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
    if tails is not None:
        for i, t in enumerate(tails):
            now = eng.buffer(i, full)[B:]
            if not torch.equal(now, t):
                ne = (now != t).flatten(1).any(1).nonzero().flatten().tolist()
                problems.append(f"buffer {P.bufs[i]['name']}: a forward of {B} images changed rows of the images behind them: images {[B + j for j in ne[:8]]}")
        del tails
    sel = torch.tensor(probes, device=dev)
    got = [eng.buffer(i, B)[sel].float().cpu() for i in range(len(P.bufs))]  # one buffer at a time, sliced on the device
    eng.close()
    t1 = time.perf_counter()

    # ---- every op against its reference
    w_all, b_all = P.arrays()
    if prec == "fp16":
        w_all = pr.fp16_weights(P, w_all)
    rep = pr.check_ops(P, got, x[probes], probes, prec, chains, tiles, w_all, b_all, floor=floor(P) if floor is not None and prec == "bf16" else None)
    n_ops = sum(op["kind"] in (0, 1, 2) for op in P.ops)
    fused = {i for ch in chains for i in ch}  # these never launch on their own tile: the pair's launch runs them (csrc/ds_b2b.hip, the b2b implicit-GEMM tile)
    own = [i for i in convs if i not in fused]
    ran = {}
    for i in own:
        ran.setdefault(family(tiles[i]), Counter())[tiles[i]] += 1
    ran = "; ".join(f"{f}: " + ", ".join(f"{n} x{c}" for n, c in sorted(k.items())) for f, k in sorted(ran.items()))
    line = (f"\n{tag} {cid}: {applied} applied / {len(found)} looked up of {len(convs)} convs; tile families {dict(sorted(fam.items()))}; tiles selected for the {len(own)} convs outside the fused chains [{ran}]; "
            f"B {B} probes {probes}; {rep['single']} ops singly + {rep['chained']} in {len(chains)} chains; {len(rep['failures'])} failures; "
            f"engine + forward {t1 - t0:.1f} s, reference {time.perf_counter() - t1:.1f} s")
    with capfd.disabled():
        print(line)
    assert rep["single"] + rep["chained"] == n_ops and rep["chained"] == sum(len(c) for c in chains)
    problems += [m for _, m in rep["failures"]]
    return dict(problems=problems, rep=rep, tiles=tiles, found=found, P=P, B=B, probes=probes, convs=convs, own=own, chains=chains, n_ops=n_ops, line=line,
                what=f"{cid} ({variant} @{S}, max_batch {MB}, {lanes} lane(s), {prec})")
