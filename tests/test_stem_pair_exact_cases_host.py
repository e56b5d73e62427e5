"""No GPU, no library (but for the planting test, which reads arch.build_program): the conditions under which tests/test_gpu_stem_pair_exact.py means something,
checked on tests/stem_pair_exact_cases.py alone, for every case the GPU test runs (sp.GPU_CASES).

  EXACTNESS  v = fl32(w / 255) for every stem weight and hi + mid + lo = v; every part and every bias is a multiple of the family's grid; max sum |terms| + |bias| of
             each of the three layers is below 2^24 grid units; a float32 emulation of the stem sum over a sample of outputs gives the float64 value in four orders
             (ascending k, descending k, a seeded permutation of the 81 products, by part: all lo products, then mid, then hi).
  COUNTS     (counts, not shares: a small map cannot make them vacuous) chain: >= 100 exact ties and >= 100 inexact non-ties among the compared final outputs, >= 1 000 of
             each at the stem, and ReLU zeros there; every pass_* case shows >= 1 000 stem ties directly; pass_lo has lo != 0 in >= 1/4 of its stem weights, pass_mid
             mid != 0 in >= 1/2.
  FAULTS     which family shows which planted fault (VISIBLE below; everything else is asserted INVISIBLE, so the table says who catches what):
                 drop_lo      only pass_lo (nowhere else is there a third part)
                 drop_mid     pass_mid and pass_lo
                 pixel_sign   every family with dense pixels (pass_lo's stay below 4)
                 left_clamp   every family, and only in the outputs of column 0: the tiles on the left image border; top_clamp: row 0
                 ninth_row    every family
                 ring_kept    only chain (a pass-through downsample has no tap with ky == 0 or kx == 0), and only in row 0 / column 0
                 truncate, half_up, half_away at the stem: every family
  PLANTING   the planted arrays have the shapes, dtypes and zero columns of the program's own ops 0..2 for both variants, and are exact in bf16 where the library stores
             bf16 (both convs' weights)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as cx
import stem_pair_exact_cases as sp

VISIBLE = {
    "chain": {"pixel_sign", "left_clamp", "top_clamp", "ninth_row", "ring_kept"},
    "pass_int": {"pixel_sign", "left_clamp", "top_clamp", "ninth_row"},
    "pass_mid": {"drop_mid", "pixel_sign", "left_clamp", "top_clamp", "ninth_row"},
    "pass_lo": {"drop_lo", "drop_mid", "left_clamp", "top_clamp", "ninth_row"},
}


def _id(c):
    return f"{c[0][-1]}{c[1]}b{c[2]}-{c[3]}{c[4]}"


def _pre_final(case):
    """the 1x1's exact sums before ReLU and the store, float32"""
    _, d, _ = sp.reference(case, stages=True)
    y = d.double() @ torch.from_numpy(case["w_11"].reshape(-1, 96).T.copy()).double() + torch.from_numpy(case["b_11"]).double()
    assert torch.equal(y.float().double(), y)
    return y.float()


@pytest.mark.parametrize("cid", sp.GPU_CASES, ids=_id)
def test_every_layer_is_exact_in_fp32(cid):
    c = sp.stem_pair_case(*cid)
    g = c["grid"]
    assert c["w"].dtype == np.float32 and np.array_equal((c["w"] / np.float32(255.0)).astype(np.float32), c["v"])
    assert np.array_equal(c["hi"] + c["mid"] + c["lo"], c["v"].astype(np.float64))
    for part in (c["hi"], c["mid"], c["lo"], c["b_stem"].astype(np.float64), c["b_ds"].astype(np.float64), c["b_11"].astype(np.float64)):
        assert np.array_equal(np.round(part / g), part / g)
    for part in (c["hi"], c["mid"], c["lo"]):
        assert torch.equal(torch.from_numpy(part).bfloat16().double(), torch.from_numpy(part))
    assert np.array_equal(np.round(c["w_ds"]), c["w_ds"]) and np.array_equal(np.round(c["w_11"]), c["w_11"]) and float(np.abs(c["w_ds"]).max()) <= 2 and float(np.abs(c["w_11"]).max()) <= 2
    assert int(c["images"].max()) == (3 if c["family"] == "pass_lo" else 255) and c["images"].dtype == torch.uint8 and c["images"].shape == (c["B"], c["S"], c["S"], 3)
    bounds = sp.abs_sum_bounds(c)
    print(f"[stem pair exact] {_id(cid)}: max sum |terms| + |bias| = 2^{math.log2(bounds[0]):.1f}, 2^{math.log2(bounds[1]):.1f}, 2^{math.log2(bounds[2]):.1f} grid units")
    assert all(b < 2 ** 24 for b in bounds), bounds
    # the stem sum in float32, one product at a time, on a sample of stem pixels (all 48 channels of each)
    exact = sp.stem_exact(c).reshape(-1, 48)
    A = sp._taps_s2(c["images"].double()).reshape(-1, 27)
    pick = torch.randperm(A.shape[0], generator=torch.Generator().manual_seed(5))[:1500]
    pick = torch.cat([pick, torch.arange(0, c["S"] // 2)])  # (and the first stem row: the zero padding above it)
    A32, want = A[pick].float(), exact[pick]
    parts = [torch.from_numpy(c[n]).float() for n in ("hi", "mid", "lo")]
    bias = torch.from_numpy(c["b_stem"])
    asc = [(p, k) for k in range(27) for p in (2, 1, 0)]
    perm = [asc[i] for i in torch.randperm(81, generator=torch.Generator().manual_seed(81)).tolist()]
    by_part = [(p, k) for p in (2, 1, 0) for k in range(27)]
    for name, order in (("ascending", asc), ("descending", asc[::-1]), ("permuted", perm), ("by part", by_part)):
        acc = torch.zeros(A32.shape[0], 48, dtype=torch.float32)
        for p, k in order:
            acc = acc + A32[:, k : k + 1] * parts[p][k : k + 1]
        y = acc + bias
        assert y.dtype == torch.float32 and torch.equal(y.double(), want), (cid, name)
        y = bias + acc if name == "permuted" else y
        assert torch.equal(y.double(), want), (cid, name)


def test_reference_equals_torch_conv2d():
    """the explicit-padding chain against torch's own convolutions in float64 (roundings between the layers as this file's reference makes them)"""
    c = sp.stem_pair_case("vgg_heads_m", 64, 5, "chain", 0)
    nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    v = torch.from_numpy(c["v"].astype(np.float64)).T.reshape(48, 3, 3, 3)
    y = F.conv2d(nchw(c["images"].double()), nchw(v), torch.from_numpy(c["b_stem"]).double(), stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(y, sp.stem_exact(c))
    s, d, o = sp.reference(c, stages=True)
    assert torch.equal(s, torch.relu(cx.rne(y.float(), cx.BF16)))
    y = F.conv2d(nchw(s.double()), nchw(torch.from_numpy(c["w_ds"][..., :48]).double()), torch.from_numpy(c["b_ds"]).double(), stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(d, torch.relu(cx.rne(y.float(), cx.BF16)))
    y = d.double() @ torch.from_numpy(c["w_11"].reshape(-1, 96).T.copy()).double() + torch.from_numpy(c["b_11"]).double()
    assert torch.equal(o, torch.relu(cx.rne(y.float(), cx.BF16))) and o.shape == (5, 16, 16, 128)
    assert torch.equal(sp.reference(c, stem=s), o)
    sp.output_bits(o)  # representable
    # a stem tensor from elsewhere with one value off the grid: exactly the four output pixels that read stem pixel (5, 7) are not defined, the others as before
    assert bool(sp.on_grid(c, s).all()) and bool(sp.exact_pixels(c, s).all())
    t = s.clone()
    t[0, 5, 7, 11] = 1e-5
    ok = sp.exact_pixels(c, t)
    assert (~ok).nonzero().tolist() == [[0, 2, 3], [0, 2, 4], [0, 3, 3], [0, 3, 4]] and int((~sp.on_grid(c, t)).sum()) == 1
    assert torch.equal(sp.reference(c, stem=t)[ok], o[ok])
    assert sp.stem_pair_case("vgg_heads_m", 64, 5, "chain", 0) is c and not torch.equal(c["images"], sp.stem_pair_case("vgg_heads_m", 64, 5, "chain", 1)["images"])


@pytest.mark.parametrize("cid", sp.GPU_CASES, ids=_id)
def test_counts_of_ties_inexact_values_and_zeros(cid):
    c = sp.stem_pair_case(*cid)
    e = sp.stem_exact(c).float()
    _, tie, inexact = cx.classify(e, cx.BF16)
    pos = e > 0
    n_tie, n_inexact, n_zero = int((tie & pos).sum()), int((inexact & pos).sum()), int((~pos).sum())
    lo_share, mid_share = float((c["lo"] != 0).mean()), float((c["mid"] != 0).mean())
    print(f"[stem pair exact] {_id(cid)}: stem values {e.numel()}: {n_tie} ties, {n_inexact} inexact non-ties, {n_zero} ReLU zeros; lo != 0 in {lo_share:.3f}, mid != 0 in {mid_share:.3f} of the weights")
    assert n_tie >= 1000 and n_inexact >= 1000 and n_zero >= 1000
    if c["family"] == "chain":
        y = _pre_final(c)
        _, t2, i2 = cx.classify(y, cx.BF16)
        print(f"[stem pair exact] {_id(cid)}: final outputs {y.numel()}: {int((t2 & (y > 0)).sum())} ties, {int((i2 & (y > 0)).sum())} inexact non-ties")
        assert int((t2 & (y > 0)).sum()) >= 100 and int((i2 & (y > 0)).sum()) >= 100
    else:
        # every compared output IS the stem value the selector names: the ties above are shown directly.  Seeds 0 and 1 together: every (tap, channel) pair
        s, _, o = sp.reference(c, stages=True)
        for ch_out in (0, 47, 95, 96, sp.C2[c["variant"]] - 1):
            ky, kx, ch = sp.source_of_output(c, ch_out)
            assert torch.equal(o[..., ch_out], s[:, ky - 1 :: 2, kx - 1 :: 2, ch])
        both = {sp.selector(seed, ch) for seed in (0, 1) for ch in range(96)}
        assert both == {(ky, kx, ch) for ky in (1, 2) for kx in (1, 2) for ch in range(48)}
        assert {sp.final_source(o_) for o_ in range(sp.C2[c["variant"]])} == set(range(96))
    if c["family"] == "pass_lo":
        assert lo_share >= 0.25
    if c["family"] == "pass_mid":
        assert mid_share >= 0.5 and lo_share == 0.0
    if c["family"] in ("chain", "pass_int"):
        assert lo_share == 0.0 and mid_share == 0.0


@functools.lru_cache(maxsize=None)
def _clean_bits(cid):
    return sp.output_bits(sp.reference(sp.stem_pair_case(*cid)))


@pytest.mark.parametrize("cid", sp.GPU_CASES, ids=_id)
def test_planted_faults_show_in_the_family_meant_to_catch_them(cid):
    c = sp.stem_pair_case(*cid)
    clean = _clean_bits(cid)
    seen = {}
    for fault in sp.FAULTS:
        bad = sp.output_bits(sp.reference(c, fault=fault)) != clean
        seen[fault] = int(bad.sum())
        if fault in VISIBLE[c["family"]]:
            assert seen[fault] >= 1, (cid, fault)
        else:
            assert seen[fault] == 0, (cid, fault)
        where = bad.nonzero()
        if fault == "left_clamp":
            assert bool((where[:, 2] == 0).all())
        if fault == "top_clamp":
            assert bool((where[:, 1] == 0).all())
        if fault == "ring_kept":
            assert bool(((where[:, 1] == 0) | (where[:, 2] == 0)).all())
    for name in cx.WRONG_ROUNDINGS:
        seen[name] = int((sp.output_bits(sp.reference(c, rounding=name)) != clean).sum())
        assert seen[name] >= 1, (cid, name)
    print(f"[stem pair exact] {_id(cid)}: outputs changed of {clean.numel()}: {seen}")


@pytest.mark.parametrize("variant", sorted(sp.C2))
def test_planted_arrays_fit_the_programs_first_three_ops(variant):
    from head_detector_amd import arch

    S = 64
    P = arch.build_program(variant, arch.random_state_dict(variant, 1), S)
    assert [op["name"] for op in P.ops[:3]] == ["backbone.stem.conv", "backbone.stage1.downsample", "backbone.stage1.blocks.conv1|conv2"]
    assert [op["kind"] for op in P.ops[:3]] == [0, 1, 1] and all(op["act"] == 1 for op in P.ops[:3])  # (ReLU behind all three: what the reference applies)
    o1, o2 = P.ops[1], P.ops[2]
    assert (o1["cin"], o1["cout_pad"], o1["ksize"], o1["stride"]) == (64, 96, 3, 2) and (o2["cin"], o2["cout_pad"], o2["cout_store"], o2["ksize"]) == (96, sp.C2[variant], sp.C2[variant], 1)
    assert arch.b2b_pairs(P)[0] == 1
    for fam, seed in sp.FAMILY_SEEDS:
        c = sp.stem_pair_case(variant, S, 5, fam, seed)
        ws, bs = sp.program_arrays(c)
        for i in range(3):
            assert ws[i].shape == P.weights[i].shape and ws[i].dtype == P.weights[i].dtype == np.float32 and ws[i].flags["C_CONTIGUOUS"], (fam, i)
            assert bs[i].shape == P.biases[i].shape and bs[i].dtype == P.biases[i].dtype == np.float32, (fam, i)
        assert np.array_equal(ws[0].reshape(48, 3, 3, 3)[7, 2, 1, 0], c["w"][(2 * 3 + 1) * 3 + 0, 7])
        assert float(np.abs(ws[1].reshape(96, 3, 3, 64)[..., 48:]).max()) == 0.0  # vgh_net_create checks these columns
        assert float(np.abs(P.weights[1].reshape(96, 3, 3, 64)[..., 48:]).max()) == 0.0
        for i in (1, 2):  # stored as bf16 by the library
            t = torch.from_numpy(ws[i])
            assert torch.equal(t.bfloat16().float(), t)
