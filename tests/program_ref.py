"""TEST INFRASTRUCTURE: executes a head_detector_amd.arch.Program with plain torch CPU ops (F.conv2d / max_pool2d),
optionally emulating the engine's bf16 storage (inputs, weights and every stored activation rounded to bf16,
fp32 accumulation).  Used (a) on CPU to prove that fold + fusion + concat-by-offset lowering reproduces the
unfused oracle network, (b) on the GPU box as the per-op checker of the HIP kernels on the engine's own inputs."""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F


def rb(t: torch.Tensor, bf16: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32) if bf16 else t


def alloc(P, B: int):
    return [torch.zeros(B, bf["h"], bf["w"], bf["pitch"], dtype=torch.float32) for bf in P.bufs]


def run_op(P, op, bufs, image, bf16: bool, w_all=None, b_all=None, f64: bool = False):
    """Executes one op in place on `bufs` (list of [B,h,w,pitch] float tensors).  f64: the arithmetic of the op in float64 (inputs and
    stored result stay float32) -- the reference for the parity modes, whose own error is then not mixed with torch's fp32 summation order."""
    up = (lambda t: t.double()) if f64 else (lambda t: t)
    if w_all is None:
        w_all, b_all = P.arrays()
    kind = op["kind"]
    if kind == 3:  # FORK: scheduling only
        return
    if kind == 0:  # stem: exact fp32 conv on the image, ReLU, stored as bf16
        W = torch.from_numpy(w_all[op["w_off"] : op["w_off"] + 48 * 27].reshape(48, 3, 3, 3)).permute(0, 3, 1, 2).contiguous()
        b = torch.from_numpy(b_all[op["b_off"] : op["b_off"] + 48])
        x = image if image.dtype == torch.float32 else image.permute(0, 3, 1, 2).float() / 255.0
        y = torch.relu(F.conv2d(up(x), up(W), up(b), stride=2, padding=1)).permute(0, 2, 3, 1).float()
        out = bufs[op["out_buf"]]
        out[..., op["out_coff"] : op["out_coff"] + 48] = rb(y, bf16)
        if op["cout_store"] > 48:  # 64-channel pitch (parity modes): 16 stored zeros; the bf16 mode stores the 48 channels at a 48-channel pitch
            out[..., op["out_coff"] + 48 : op["out_coff"] + 64] = 0
        return
    if kind == 2:  # SPP pools
        buf = bufs[op["in_buf"]]
        C, c0 = op["cin"], op["in_coff"]
        x = buf[..., c0 : c0 + C].permute(0, 3, 1, 2)
        for i, k in enumerate((5, 9, 13)):
            buf[..., c0 + (i + 1) * C : c0 + (i + 2) * C] = F.max_pool2d(x, k, 1, k // 2).permute(0, 2, 3, 1)
        return
    k, cin, rp = op["ksize"], op["cin"], op["cout_pad"]
    W = torch.from_numpy(w_all[op["w_off"] : op["w_off"] + rp * k * k * cin].reshape(rp, k, k, cin)).permute(0, 3, 1, 2).contiguous()
    b = torch.from_numpy(b_all[op["b_off"] : op["b_off"] + rp])
    gc = op.get("grp_cout", 0)
    if gc:  # grouped conv: cout group g reads its own cin-channel window
        ys = []
        for g in range(rp // gc):
            c0 = op["in_coff"] + g * op["grp_in_stride"]
            xg = bufs[op["in_buf"]][..., c0 : c0 + cin].permute(0, 3, 1, 2)
            ys.append(F.conv2d(up(rb(xg, bf16)), up(rb(W[g * gc : (g + 1) * gc], bf16)), None, stride=op["stride"], padding=k // 2))
        y = torch.cat(ys, 1) + up(b)[None, :, None, None]
    else:
        x = bufs[op["in_buf"]][..., op["in_coff"] : op["in_coff"] + cin]
        if x.shape[-1] < cin:
            # a K window wider than the pitch (the 48-channel stem tensor read as 64 channels): the engine's window runs on into the next pixel and meets
            # all-zero weight columns (checked here, and by vgh_net_create); zeros stand in for those finite values
            assert float(W[:, x.shape[-1] :].abs().max()) == 0.0
            x = torch.cat([x, torch.zeros(*x.shape[:-1], cin - x.shape[-1], dtype=x.dtype)], -1)
        x = x.permute(0, 3, 1, 2)
        y = F.conv2d(up(rb(x, bf16)), up(rb(W, bf16)), None, stride=op["stride"], padding=k // 2) + up(b)[None, :, None, None]
    if op["act"] == 1:
        y = torch.relu(y)
    elif op["act"] == 2:
        y = y * torch.sigmoid(y)
    y = y.permute(0, 2, 3, 1)  # [B,ho,wo,rp]
    out = bufs[op["out_buf"]]
    is_f32 = P.bufs[op["out_buf"]]["is_f32"]
    if op["shuffle"]:
        C = rp // 4
        B_, h, w, _ = y.shape
        z = torch.zeros(B_, 2 * h, 2 * w, C, dtype=y.dtype)
        for d in range(4):
            z[:, d // 2 :: 2, d % 2 :: 2, :] = y[..., d * C : (d + 1) * C]
        y = z
    if op["res_buf"] >= 0:
        n = min(y.shape[-1], op["cout_store"])
        r = bufs[op["res_buf"]][..., op["res_coff"] : op["res_coff"] + n]
        y = y.clone()
        y[..., :n] = y[..., :n] + (float(np.float32(op["alpha"])) * up(r) if f64 else np.float32(op["alpha"]) * r)
    store = op["cout_store"] if not op["shuffle"] else rp // 4
    split = min(op["out_split"], store)
    y = y.float()
    y = y if is_f32 else rb(y, bf16)
    out[..., op["out_coff"] : op["out_coff"] + split] = y[..., :split]
    if store > split:
        out[..., op["out_coff2"] : op["out_coff2"] + store - split] = y[..., split:store]


def run_program(P, image, bf16: bool):
    bufs = alloc(P, image.shape[0])
    w_all, b_all = P.arrays()
    for op in P.ops:
        run_op(P, op, bufs, image, bf16, w_all, b_all)
    return bufs


def fp16_weights(P, w_all):
    """Copy of the program's weights as the single-plane fp16 mode stores them: per conv a power-of-two prescale into [512, 1024), rounded to fp16
    (vgh_pack_conv_weights_split, fmt VGH_FMT_F16), back in real units."""
    w_all = w_all.copy()
    for op in P.ops:
        if op["kind"] != 1:
            continue
        sl = slice(op["w_off"], op["w_off"] + op["cout_pad"] * op["ksize"] ** 2 * op["cin"])
        w = torch.from_numpy(w_all[sl])
        mx = float(w.abs().max())
        sc = 2.0 ** (10 - int(np.frexp(mx)[1])) if mx > 0 else 1.0
        w_all[sl] = ((w * sc).half().float() / sc).numpy()
    return w_all


# ------------------------------------------------------------------------------------------------------
# per-op checker of a whole forward (tests/test_gpu_tuned_ops.py on the GPU; tests/test_host_logic.py proves on the CPU that it discriminates)
# ------------------------------------------------------------------------------------------------------
# |fp32 evaluation - float64 evaluation| at the output of a fused chain, both with bf16 storage: two correct evaluations differ where an intermediate value (stem or
# downsample output) lands on the other side of a bf16 rounding boundary.  MEASURED on the CPU alone (no kernel involved; `python tests/program_ref.py [size ...]` prints it; x86-64,
# torch CPU convolutions, seed-7 weights, two u8 images of seed 640): the chains of L @640 and M @640 (the l64 / m32 programs of tests/test_gpu_tuned_ops.py) below -- the
# worst is one bf16 ulp of an output in [16, 32).  A chain is held to the single-op tolerance plus TWICE the worst value: either side of the comparison may flip.
CHAIN_FLOOR_MEASURED = {"vgg_heads_l@640": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_m@640": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        # the other bf16 programs of OFFPATH_CASES, measured the same way (two u8 images of seed = image size): each is held to ITS OWN worst value
                        # (chain_floor_for); none of them moves CHAIN_FLOOR
                        "vgg_heads_l@320": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_m@320": {"backbone.stage1.blocks.conv1|conv2": 0.0078125, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_m@352": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.0625},
                        "vgg_heads_l@416": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_l@480": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_m@736": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125},
                        "vgg_heads_l@1280": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.25},  # one bf16 ulp of an output in [32, 64)
                        "vgg_heads_m@1280": {"backbone.stage1.blocks.conv1|conv2": 0.015625, "neck.neck2.blocks.conv1|conv2": 0.125}}
CHAIN_FLOOR = max(v for k in ("vgg_heads_l@640", "vgg_heads_m@640") for v in CHAIN_FLOOR_MEASURED[k].values())  # 0.125: the 640 programs only, whatever the others measure

# absolute + relative tolerance of one fp16x3 conv with O(1) values (tests/test_gpu_split.py TOL[FMT_F16X2]); scaled by max(1, max|e|) of the op's output
F16X3_TOL = (2e-5, 1e-5)


def own_channels(P, op):
    """(buffer, [(first channel, count), ...]): the channels of the arena this op writes."""
    if op["kind"] == 2:
        return op["in_buf"], [(op["in_coff"] + op["cin"], 3 * op["cin"])]
    if op["kind"] == 0:
        return op["out_buf"], [(op["out_coff"], op["cout_store"])]
    store = op["cout_store"] if not op["shuffle"] else op["cout_pad"] // 4
    split = min(op["out_split"], store)
    return op["out_buf"], [(op["out_coff"], split)] + ([(op["out_coff2"], store - split)] if store > split else [])


def seg(P, op, t):
    """The op's own channels of its output buffer `t`, concatenated (a CSP concat buffer: other ops write the rest of it)."""
    return torch.cat([t[..., c0 : c0 + n] for c0, n in own_channels(P, op)[1]], -1)


def fused_chains(P, stem_fused: bool):
    """Op-index chains the engine's default mode runs as ONE launch each: every arch.b2b_pairs pair (i, i + 1); the stem in front of the pair that reads its tensor when the
    engine fuses it (u8 images, VGHeadsEngine.stem_fused).  The tensors between the ops of a chain are never written."""
    from head_detector_amd import arch

    out = []
    for i in arch.b2b_pairs(P):
        ch = [i, i + 1]
        if stem_fused and i > 0 and P.ops[i - 1]["kind"] == 0 and P.ops[i]["in_buf"] == P.ops[i - 1]["out_buf"]:
            ch = [i - 1] + ch
        out.append(ch)
    return out


def run_chain(P, chain, got, image, w_all, b_all, f64: bool = False):
    """Reference of a fused chain on the inputs of its first op: every op in turn, each intermediate tensor rounded to bf16 (run_op's storage); returns the last op's output buffer."""
    exp = list(got)
    for i in chain:
        ob = P.ops[i]["out_buf"]
        exp[ob] = torch.zeros_like(got[ob]) if i != chain[-1] else got[ob].clone()
    for i in chain:
        run_op(P, P.ops[i], exp, image, True, w_all, b_all, f64=f64)
    return exp[P.ops[chain[-1]]["out_buf"]]


def op_tolerance(mode: str, is_f32: bool, e, chained: bool = False, floor: float = None):
    """The project's per-op tolerances (test_network_every_op, test_fp16_network_every_op, test_gpu_split.TOL) for an expected tensor `e` (the op's own channels).
    floor: the chain allowance of the program when it is not the global CHAIN_FLOOR (chain_floor_for)."""
    if mode == "bf16":
        tol = (2e-3 + 1e-4 * e.abs()) if is_f32 else (2e-2 + 1.0 / 64 * e.abs())  # bf16: 2 ulps (accumulation order can cross a rounding boundary)
        return tol + 2.0 * (CHAIN_FLOOR if floor is None else floor) if chained else tol
    assert not chained, "only bf16 programs have fused chains"
    if mode == "fp16":
        return (2e-3 + 2e-4 * e.abs()) if is_f32 else (1e-3 + 1.0 / 1024 * e.abs())  # exact operands: one fp16 ulp + accumulation-order slack
    if mode == "fp16x3":
        atol, rtol = F16X3_TOL
        return atol * max(1.0, float(e.abs().max())) + rtol * e.abs()
    raise ValueError(mode)


def check_ops(P, got, image, probes, mode: str = "bf16", chains=(), tiles=None, w_all=None, b_all=None, floor: float = None):
    """Every op of kind 0 / 1 / 2 of a forward against run_op on the forward's OWN inputs of that op (no error accumulates across layers).
    got[b]: float32 CPU tensor [len(probes), h, w, pitch] of buffer b for the probe images; image: the probe images (u8 NHWC / f32 NCHW); probes: their indices in the
    batch (for the messages).  mode: "bf16" (bf16-emulating fp32 reference), "fp16" (float64 reference on the prescaled fp16 weights: pass fp16_weights as w_all),
    "fp16x3" (float64 reference).  chains (fused_chains): the ops of a chain are checked as one reference chain at the last op's output, and the tensors between them must
    be all zero (never written).  tiles {op index: tile name}: for the messages.  floor: op_tolerance's.
    Returns dict(single=ops checked singly, chained=ops inside chains, failures=[(op name, message)]); nothing is raised for a mismatch."""
    if w_all is None:
        w_all, b_all = P.arrays()
    tiles = tiles or {}
    f64 = mode != "bf16"
    in_chain = {i: ch for ch in chains for i in ch}
    rep = dict(single=0, chained=0, failures=[])

    def compare(op_idx, names, a_buf, e_buf):
        op = P.ops[op_idx]
        ob, _ = own_channels(P, op)
        a, e = seg(P, op, a_buf), seg(P, op, e_buf)
        tol = op_tolerance(mode, P.bufs[ob]["is_f32"] == 1, e, chained=len(names) > 1, floor=floor)
        err = (a - e).abs()
        bad = ~(err <= tol)  # (a NaN is a mismatch)
        if not bool(bad.any()):
            return
        idx = bad.nonzero()
        worst = int((torch.nan_to_num(err, nan=float("inf")) * bad).flatten().argmax())
        key = "m%d_n%d_k%d_ks%d_s%d" % (*op["gemm"], op["ksize"], op["stride"]) + ("_res" if op.get("res_buf", -1) >= 0 else "") if op["kind"] == 1 else f"kind{op['kind']}"
        tile = "|".join(str(tiles.get(i, "library's choice")) for i in (in_chain.get(op_idx) or [op_idx]))
        for p in sorted(set(idx[:, 0].tolist())):
            sel = idx[idx[:, 0] == p]
            pix = (sel[:, 1] * e.shape[2] + sel[:, 2]) % 32
            rep["failures"].append((names[-1], f"op {' -> '.join(names)} tile {tile} gemm {key} map {e.shape[1]}x{e.shape[2]} probe image {probes[p]}: {len(sel)}/{e[p].numel()} mismatches; "
                                    f"worst of the op got {float(a.flatten()[worst])} want {float(e.flatten()[worst])} at {[int(v) for v in np.unravel_index(worst, tuple(e.shape))]}; "
                                    f"first {sel[:4, 1:].tolist()}; pixel%32 hist {torch.bincount(pix, minlength=32).tolist()}; chan%32 hist {torch.bincount(sel[:, 3] % 32, minlength=32).tolist()}"))

    for i, op in enumerate(P.ops):
        if op["kind"] == 3:
            continue
        ch = in_chain.get(i)
        if ch is not None:
            rep["chained"] += 1
            if i != ch[-1]:
                ob = op["out_buf"]
                if float(got[ob].abs().max()) != 0.0:
                    rep["failures"].append((op["name"], f"op {op['name']}: its output tensor lies inside a fused chain and must never be written, but holds max |x| = {float(got[ob].abs().max())}"))
                continue
            e_buf = run_chain(P, ch, got, image, w_all, b_all, f64=f64)
            compare(i, [P.ops[j]["name"] for j in ch], got[op["out_buf"]], e_buf)
            continue
        rep["single"] += 1
        ob, _ = own_channels(P, op)
        exp = list(got)
        exp[ob] = got[ob].clone()
        run_op(P, op, exp, image, mode == "bf16", w_all, b_all, f64=f64)
        compare(i, [op["name"]], got[ob], exp[ob])
    return rep


def head_outputs(P, bufs):
    """per level: (reg [B,68,H,W], cls [B,1,H,W], raw branch dict) as NCHW torch tensors (oracle format)."""
    out = []
    S, E = P.shape_c, P.expr_c
    for lv in P.levels:
        t = bufs[lv["buf"]].permute(0, 3, 1, 2)
        o = 72  # VGH_PRED_FLAME_OFF: [reg 68 | cls 1 | 3 unused | shape | expr | rot jaw trans scale]
        raw = dict(shape=t[:, o : o + S], expr=t[:, o + S : o + S + E], rot=t[:, o + S + E : o + S + E + 6], jaw=t[:, o + S + E + 6 : o + S + E + 9],
                   trans=t[:, o + S + E + 9 : o + S + E + 12], scale=t[:, o + S + E + 12 : o + S + E + 13])
        out.append((t[:, :68], t[:, 68:69], raw))
    return out


# the benchmarked workloads whose tuned tile choices are checked op by op: id -> (variant, image size, max_batch, lanes, precision).  The lane counts are bench.py's: its
# run_workload sets --split (default 2) for every timed workload, its one_image_latency builds max_batch = 1 engines and never splits.
TUNED_CASES = {
    "l64": ("vgg_heads_l", 640, 64, 2, "bf16"),  # the benchmark line
    "m32": ("vgg_heads_m", 640, 32, 2, "bf16"),
    "l8": ("vgg_heads_l", 640, 8, 2, "bf16"),
    "l1": ("vgg_heads_l", 640, 1, 1, "bf16"),  # latency lanes
    "m1": ("vgg_heads_m", 640, 1, 1, "bf16"),
    "l16_1280": ("vgg_heads_l", 1280, 16, 2, "bf16"),
    "l256_1280": ("vgg_heads_l", 1280, 256, 2, "bf16"),  # runs arena_batch (27) images per chunk
    "l64_fp16": ("vgg_heads_l", 640, 64, 2, "fp16"),
    "l32_fp16x3": ("vgg_heads_l", 640, 32, 2, "fp16x3"),
}


# selections the benchmark never runs, checked op by op by tests/test_gpu_offpath_ops.py: id -> (variant, image size, max_batch, lanes, precision[, images forwarded]).
# tests/test_host_logic.py::test_every_table_pair_of_the_sweep_has_a_reference_checked_case holds TUNED_CASES + OFFPATH_CASES to every (GEMM shape, tile) pair the table
# can select over M / L x {320, 640, 1280} x max_batch {1, 2, 3, 8, 16, 17, 32, 33, 64} x lanes {1, 2} x {bf16, fp16, fp16x3}: a table entry added without a case fails there.
OFFPATH_CASES = {
    # sizes the table has no entry for: the class heuristic (bf16) / the split pick rules (fp16, fp16x3) choose every tile, on ragged pyramids
    "m5_352x2": ("vgg_heads_m", 352, 5, 2, "bf16"),  # uneven lanes (3 + 2), final maps 11 x 11
    "l3_416x1": ("vgg_heads_l", 416, 3, 1, "bf16"),
    "l2_480": ("vgg_heads_l", 480, 2, 1, "bf16"),  # the latency-lane schedule on 15 x 15 maps
    "m20_736x2": ("vgg_heads_m", 736, 20, 2, "bf16"),  # the two largest pixel buckets of the heuristic with ragged maps
    "m3_352_fp16x3": ("vgg_heads_m", 352, 3, 1, "fp16x3"),
    "l3_416_fp16": ("vgg_heads_l", 416, 3, 1, "fp16"),
    "l32_fp16x1": ("vgg_heads_l", 640, 32, 1, "fp16"),  # no table entry applies
    # table pairs no benchmarked program selects: mostly the single-lane buckets (what an engine uses unless set_split is called)
    "l32x1": ("vgg_heads_l", 640, 32, 1, "bf16"),
    "m32x1": ("vgg_heads_m", 640, 32, 1, "bf16"),
    "m16x1": ("vgg_heads_m", 640, 16, 1, "bf16"),
    "l8x1": ("vgg_heads_l", 640, 8, 1, "bf16"),
    "l17x2": ("vgg_heads_l", 640, 17, 2, "bf16"),  # the bucket edge, lanes of 9 and 8
    "l4_1280x1": ("vgg_heads_l", 1280, 4, 1, "bf16"),
    "m4_1280x1": ("vgg_heads_m", 1280, 4, 1, "bf16"),
    "l8_320x1": ("vgg_heads_l", 320, 8, 1, "bf16"),
    "m8_320x1": ("vgg_heads_m", 320, 8, 1, "bf16"),
    "l1_320": ("vgg_heads_l", 320, 1, 1, "bf16"),
    # what the completeness sweep demanded beyond the above (17 is the smallest batch of the b32 bucket, 33 of the b64 bucket)
    "m17_fp16x2": ("vgg_heads_m", 640, 17, 2, "fp16"),
    "m33_320x1": ("vgg_heads_m", 320, 33, 1, "bf16"),
    "l17_fp16x3x1": ("vgg_heads_l", 640, 17, 1, "fp16x3"),
    "l17_320_fp16x2": ("vgg_heads_l", 320, 17, 2, "fp16"),
    "l17_320x2": ("vgg_heads_l", 320, 17, 2, "bf16"),
    "m17_1280_fp16x3x1": ("vgg_heads_m", 1280, 17, 1, "fp16x3"),
    "m17_1280x1": ("vgg_heads_m", 1280, 17, 1, "bf16"),
    "m33_1280_fp16x2": ("vgg_heads_m", 1280, 33, 2, "fp16", 2),  # 2 images forwarded (one per lane): a float64 reference of two 1280 probes took 16 s, of one 4.5 s
    "l1_1280": ("vgg_heads_l", 1280, 1, 1, "bf16"),
    "l17_320_fp16x3x1": ("vgg_heads_l", 320, 17, 1, "fp16x3"),
    "m33_320_fp16x2": ("vgg_heads_m", 320, 33, 2, "fp16"),
    "l33x1": ("vgg_heads_l", 640, 33, 1, "bf16"),
    "l17_320x1": ("vgg_heads_l", 320, 17, 1, "bf16"),
    "l33_320x2": ("vgg_heads_l", 320, 33, 2, "bf16"),
    "l33_320_fp16x2": ("vgg_heads_l", 320, 33, 2, "fp16"),
    "l17_1280_fp16x2": ("vgg_heads_l", 1280, 17, 2, "fp16", 2),  # 2 images forwarded, as above (two probes: 22 s, one: 6.4 s)
    # fewer images than max_batch on a tuned engine: the tiles-per-workgroup loops of the persistent tiles depend on the image count
    # (the two 1280 fp16 cases above are of this kind too: their max_batch picks the table bucket, their batch is cut for the reference's sake)
    "l64_fwd37": ("vgg_heads_l", 640, 64, 2, "bf16", 37),  # lanes of 19 and 18
    "m32_fwd1x2": ("vgg_heads_m", 640, 32, 2, "bf16", 1),  # the second lane is empty
}
OFF_TABLE = ("m5_352x2", "l3_416x1", "l2_480", "m20_736x2", "m3_352_fp16x3", "l3_416_fp16", "l32_fp16x1")  # no table entry applies to any of their convs
PARTIAL_BATCH = tuple(c for c, t in OFFPATH_CASES.items() if len(t) > 5)


def case_tuple(cid: str):
    """(variant, image size, max_batch, lanes, precision, images forwarded or None) of a TUNED_CASES / OFFPATH_CASES id."""
    t = TUNED_CASES[cid] if cid in TUNED_CASES else OFFPATH_CASES[cid]
    return (*t[:5], t[5] if len(t) > 5 else None)


def chain_floor_for(P) -> float:
    """The chain allowance of a bf16 OFFPATH_CASES program: the worst of ITS OWN measured |fp32 - float64| chain values (CHAIN_FLOOR_MEASURED).  The nine benchmarked cases
    keep the global CHAIN_FLOOR whatever any other program measures."""
    return max(CHAIN_FLOOR_MEASURED[f"{P.variant}@{P.image_size}"].values())


def table_pair(P, op, tile: str):
    """What the completeness sweep counts as one selection of the table: (precision, GEMM shape, ksize, stride, residual, epilogue class, tile name)."""
    from head_detector_amd.engine import _epilogue_class

    return (P.precision, tuple(op["gemm"]), op["ksize"], op["stride"], op.get("res_buf", -1) >= 0, _epilogue_class(op), tile)


@functools.lru_cache(maxsize=None)
def _state_dict(variant, seed):
    from head_detector_amd import arch

    return arch.random_state_dict(variant, seed)  # (build_program folds it into arrays of its own and leaves it as it is)


@functools.lru_cache(maxsize=None)
def _built_program(variant, S, precision, seed):
    from head_detector_amd import arch

    return arch.build_program(variant, _state_dict(variant, seed), S, precision)


def program_for(variant, S, MB, prec, seed: int = 7):
    """The op program VGHeadsEngine(variant, image_size=S, max_batch=MB, seed=seed, precision=prec) runs, built on the host (no GPU, no library)."""
    from head_detector_amd import arch
    from head_detector_amd.engine import LATENCY_MAX_BATCH

    P = copy.copy(_built_program(variant, S, prec, seed))
    P.ops = [dict(op) for op in P.ops]
    return arch.schedule_latency(P) if MB <= LATENCY_MAX_BATCH else P


def case_program(cid: str, seed: int = 7):
    """program_for a TUNED_CASES / OFFPATH_CASES id."""
    variant, S, MB, _, prec, _ = case_tuple(cid)
    return program_for(variant, S, MB, prec, seed)


def chain_floor(P, image):
    """max |fp32 - float64| evaluation of every fused chain of P at the chain's output (bf16 storage in both), on the reference's own forward of `image`: {last op name: value}."""
    w_all, b_all = P.arrays()
    got = run_program(P, image, True)
    out = {}
    for ch in fused_chains(P, image.dtype == torch.uint8):
        last = P.ops[ch[-1]]
        a = run_chain(P, ch, got, image, w_all, b_all, f64=False)
        b = run_chain(P, ch, got, image, w_all, b_all, f64=True)
        out[last["name"]] = float((seg(P, last, a) - seg(P, last, b)).abs().max())
    return out


if __name__ == "__main__":  # python tests/program_ref.py: re-measures CHAIN_FLOOR_MEASURED (CPU only)
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from head_detector_amd import arch

    progs = sorted({(t[0], t[1]) for t in list(TUNED_CASES.values()) + list(OFFPATH_CASES.values()) if t[4] == "bf16"}, key=lambda p: (p[1], p[0]))
    for variant, S in [p for p in progs if not sys.argv[1:] or str(p[1]) in sys.argv[1:]]:
        Q = arch.build_program(variant, arch.random_state_dict(variant, 7), S)
        img = torch.randint(0, 256, (2, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(S))
        print(f'"{variant}@{S}": {chain_floor(Q, img)},', flush=True)
