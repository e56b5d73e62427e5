"""GPU (-m gpu): the stem-in-pair launch -- the "u" tile of csrc/ds_b2b.hip, ds_b2b_kernel<T2, STEM = 1>: stem conv as a bf16 x 3 split GEMM, stage-1 downsample,
CSP conv1|conv2, one launch, what every forward of u8 images starts with -- held TO THE BIT on the exact-arithmetic cases of tests/stem_pair_exact_cases.py.  The tile is
by design not bit-identical to the stem kernel + "t" tile (another summation order, / 255 rounded on the weights), so every other test holds it to a tolerance; on these
operands its fp32 accumulators hold the mathematically exact sums in any order and every stored bf16 has exactly one right value.  Every comparison here is an equality
of int16 bit patterns with a float64 reference; tests/test_stem_pair_exact_cases_host.py shows on the CPU that the cases are exact, hold ties / inexact values / ReLU
zeros in numbers, and that a dropped lo or mid part, a sign-extended pixel, a clamped instead of zero-padded image border, a ninth (kx, ci) value from the wrong kernel
row, a kept out-of-map ring and the three wrong roundings each change outputs of the family meant to catch them.

Per engine (variant x size x family x seed; the planted weights replace ops 0..2 of a random-weight program, use_tuning=False, default b2b mode, eng.stem_fused asserted),
each of: the default grid; at most one workgroup per XCD (3 - 4 tiles per workgroup: the image-patch double buffer, the plane buffers and the two exchange areas all
cycle, the k + 2 < n_my edges are hit, one XCD gets a short chunk and one none); two batch-split lanes -- each with the full batch into a zeroed output tensor, then B - 1
other images, behind which the last image's rows stay as they were.  The stem tensor and the tensor between the two convs stay all zero.
On the chain case also set_b2b(3) (stem kernel + t tile) and set_b2b(0) (three launches): their pair outputs against the float64 downsample + 1x1 reference computed
from THE DEVICE'S stem tensor, bit for bit -- an independent reference for paths that are otherwise held only to each other.  The stem kernel's tensor itself is NOT
required to equal rne(exact): it runs an fmaf chain over fl(q / 255), and on the chain case -- integer sums, a tenth of them exact ties -- that chain lands on the
other side of a tie or of zero often.  Measured on the chain cases (S = 96 / 64, M and L; printed by the test as "[stem pair exact] ... stem kernel"): see
STEM_KERNEL_DIFFERS below.

Sizes: S = 96 is a 3 x 3 grid of tiles per image (interior, four edges, four corners), S = 64 four corner tiles; B = 3 / 5.  vgg_heads_m has T2 = 4 (compute wave 2 has
no second-conv groups), vgg_heads_l T2 = 6."""
import time

import pytest
import torch

import conv_exact_cases as cx
import stem_pair_exact_cases as sp

pytestmark = pytest.mark.gpu

# wall seconds per case on an MI355X box (engine construction, 6 - 8 forwards, copies and the CPU references), from this file's own "[stem pair exact] ... s" lines
SECONDS_MEASURED = {"m96b3-chain0": 0.8, "m96b3-pass_int0": 0.5, "m96b3-pass_int1": 0.4, "m96b3-pass_mid0": 0.5, "m96b3-pass_mid1": 0.4, "m96b3-pass_lo0": 0.4, "m96b3-pass_lo1": 0.5, "m64b5-chain0": 0.5, "m64b5-pass_int0": 0.4, "m64b5-pass_int1": 0.4, "m64b5-pass_mid0": 0.4, "m64b5-pass_mid1": 0.4, "m64b5-pass_lo0": 0.4, "m64b5-pass_lo1": 0.4, "l96b3-chain0": 0.7, "l96b3-pass_int0": 0.7, "l96b3-pass_int1": 0.7, "l96b3-pass_mid0": 0.7, "l96b3-pass_mid1": 0.7, "l96b3-pass_lo0": 0.7, "l96b3-pass_lo1": 0.7, "l64b5-chain0": 0.7, "l64b5-pass_int0": 0.7, "l64b5-pass_int1": 0.7, "l64b5-pass_mid0": 0.7, "l64b5-pass_mid1": 0.7, "l64b5-pass_lo0": 0.7, "l64b5-pass_lo1": 0.7}
# share of the stem kernel's values (set_b2b(3)) that differ from rne(exact sum) on the chain cases: information, not asserted
STEM_KERNEL_DIFFERS = {"m96b3-chain0": 8.87e-03, "m64b5-chain0": 7.46e-03, "l96b3-chain0": 8.53e-03, "l64b5-chain0": 9.77e-03}


def _id(c):
    return f"{c[0][-1]}{c[1]}b{c[2]}-{c[3]}{c[4]}"


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _tile_report(idx, h):
    """idx [n, 4] (b, y, x, c) of differing outputs -> histogram by tile kind, by tile, and by position inside the 8 x 8 tile"""
    n = h // 8
    ty, tx = idx[:, 1] // 8, idx[:, 2] // 8
    borders = ((ty == 0) | (ty == n - 1)).long() + ((tx == 0) | (tx == n - 1)).long()
    kinds = torch.bincount(borders, minlength=3).tolist()
    per_tile = torch.bincount(ty * n + tx, minlength=n * n).view(n, n).tolist()
    inside = torch.bincount((idx[:, 1] % 8) * 8 + idx[:, 2] % 8, minlength=64).view(8, 8).tolist()
    return (f"by tile kind: corner {kinds[2]}, edge {kinds[1]}, interior {kinds[0]}; by tile (ty, tx) {per_tile}; by image {torch.bincount(idx[:, 0]).tolist()}; "
            f"by channel % 32 {torch.bincount(idx[:, 3] % 32, minlength=32).tolist()}; by position inside the 8 x 8 tile (rows y % 8) {inside}")


def _compare(case, got, rows, where):
    """got: int16 [n,h,w,C2] of images `rows` (a slice of the case's batch) -> equal to the reference's bits, or a report"""
    want = sp.output_bits(sp.reference(case))[rows]
    assert got.shape == want.shape, (where, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = got != want
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    as_f = lambda t: float(t.view(torch.bfloat16)[first])  # noqa: E731
    msg = [f"{where}: {int(bad.sum())} of {bad.numel()} stored values differ; first {idx[:8].tolist()} (b, y, x, cout); at {first} got {as_f(got)!r} want {as_f(want)!r}",
           _tile_report(idx, got.shape[1])]
    hit = [f for f in sp.FAULTS if torch.equal(got, sp.output_bits(sp.reference(case, fault=f))[rows])]
    hit += [r for r in cx.WRONG_ROUNDINGS if torch.equal(got, sp.output_bits(sp.reference(case, rounding=r))[rows])]
    msg.append(f"reproduced exactly by: {', '.join(hit)}" if hit else "reproduced by none of the planted faults and wrong roundings")
    if case["family"] != "chain":
        srcs = sorted({sp.source_of_output(case, int(c)) for c in idx[:2000, 3]})
        msg.append(f"(ky, kx, stem channel) behind the differing outputs: {srcs[:24]}")
    raise AssertionError("\n".join(msg))


@pytest.mark.parametrize("cid", sp.GPU_CASES, ids=_id)
def test_stem_in_pair_launch_stores_the_one_right_value(gpu_lib, monkeypatch, cid):
    from head_detector_amd import arch
    from head_detector_amd.engine import VGHeadsEngine, _alias

    t0 = time.time()
    variant, S, B, family, seed = cid
    case = sp.stem_pair_case(*cid)
    ws, bs = sp.program_arrays(case)
    real = arch.build_program

    def planted(*a, **k):
        P = real(*a, **k)
        for i in range(3):
            assert P.weights[i].shape == ws[i].shape and P.biases[i].shape == bs[i].shape
            P.weights[i], P.biases[i] = ws[i].copy(), bs[i].copy()
        return P

    monkeypatch.setattr(arch, "build_program", planted)
    eng = VGHeadsEngine(variant, image_size=S, max_batch=B, use_tuning=False, keep_top_k=50)  # (a 64 x 64 image has 84 anchors)
    try:
        P = eng.program
        assert eng.stem_fused and eng.b2b_pairs >= 1 and arch.b2b_pairs(P)[0] == 1, "the stem does not run inside the pair's launch: this test would be about another kernel"
        o0, o1, o2 = P.ops[:3]
        assert o2["cout_store"] == sp.C2[variant] and all(op["act"] == 1 for op in (o0, o1, o2))
        seg = lambda t: torch.cat([t[..., o2["out_coff"]:o2["out_coff"] + o2["out_split"]], t[..., o2["out_coff2"]:o2["out_coff2"] + o2["cout_store"] - o2["out_split"]]], -1).contiguous().view(torch.int16).cpu()  # noqa: E731
        x = case["images"].to(_dev())
        others = x[1:].contiguous()  # B - 1 other images for rows 0 .. B - 2
        ob = P.bufs[o2["out_buf"]]

        def zero_out():
            n = B * ob["h"] * ob["w"] * ob["pitch"]
            eng.stream.synchronize()
            _alias(eng.lib.vgh_net_buffer(eng._net, o2["out_buf"]), (n,), "<i2", eng.device).zero_()
            torch.cuda.synchronize()

        def full_then_fewer(where):
            zero_out()
            eng.forward_net(x)
            _compare(case, seg(eng.buffer(o2["out_buf"], B)), slice(0, B), f"{_id(cid)} {where}, {B} images")
            eng.forward_net(others)
            got = seg(eng.buffer(o2["out_buf"], B))
            _compare(case, got[: B - 1], slice(1, B), f"{_id(cid)} {where}, {B - 1} other images")
            _compare(case, got[B - 1 :], slice(B - 1, B), f"{_id(cid)} {where}, the last image's rows behind a batch of {B - 1}")

        full_then_fewer("default grid")
        try:
            assert gpu_lib.vgh_conv_set_max_blocks_per_xcd(1) == 0
            full_then_fewer("one workgroup per XCD")
        finally:
            gpu_lib.vgh_conv_set_max_blocks_per_xcd(0)
        eng.set_split(2)
        full_then_fewer("two lanes")
        eng.set_split(1)
        for op in (o0, o1):  # neither the stem tensor nor the tensor between the two convs was ever written
            assert float(eng.buffer(op["out_buf"], B).float().abs().max()) == 0.0, op["name"]
        if family == "chain":
            exact = sp.reference(case, stages=True)[0]
            for mode, what in ((3, "stem kernel + t tile"), (0, "three launches")):
                eng.set_b2b(mode)
                zero_out()
                eng.forward_net(x)
                stem = eng.buffer(o0["out_buf"], B).float().cpu()
                assert stem.shape == exact.shape
                differs = int((stem != exact).sum())
                print(f"[stem pair exact] {_id(cid)} set_b2b({mode}): the stem kernel's tensor differs from rne(exact) in {differs} of {stem.numel()} values ({differs / stem.numel():.2e})")
                assert float((stem - exact).abs().max()) <= 0.01 * float(exact.abs().max())  # (the same conv: a rounding step apart at the most, checked loosely)
                # where the exact sum is 0 the stem kernel may hold 1e-5: off the integer grid, and a downsample sum that reads it is not exact in fp32.  Compared: the
                # output pixels whose 3 x 3 x 48 stem values are all on the grid (a zero sum is one stem value in a few thousand: most pixels)
                ok = sp.exact_pixels(case, stem)
                off = int((~sp.on_grid(case, stem)).sum())
                print(f"[stem pair exact] {_id(cid)} set_b2b({mode}): {off} stem values off the grid; {int(ok.sum())} of {ok.numel()} output pixels compared")
                assert int(ok.sum()) * 2 >= ok.numel()
                _, d, o = sp.reference(case, stem=stem, stages=True)
                got = seg(eng.buffer(o2["out_buf"], B))
                want = sp.output_bits(o)
                bad = (got != want) & ok[..., None]
                if bad.any():
                    idx = bad.nonzero()
                    raise AssertionError(f"{_id(cid)} {what} against the float64 reference from the device's own stem tensor: {idx.shape[0]} of {int(ok.sum()) * want.shape[-1]} differ; first {idx[:8].tolist()}\n{_tile_report(idx, want.shape[1])}")
                if mode == 0:  # the tensor between the two convs exists: the downsample alone
                    mid = eng.buffer(o1["out_buf"], B)[..., o1["out_coff"] : o1["out_coff"] + 96].contiguous().view(torch.int16).cpu()
                    assert not ((mid != sp.output_bits(d)) & ok[..., None]).any(), f"{_id(cid)} {what}: the downsample's own tensor"
            eng.set_b2b(1)
    finally:
        eng.close()
    print(f"[stem pair exact] {_id(cid)}: {time.time() - t0:.1f} s")
