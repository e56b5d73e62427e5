"""No GPU: the conditions under which tests/test_gpu_conv_q8_exact.py means something, checked on tests/conv_q8_exact_cases.py (and, for the weight scales the cases
rely on, the library's own host-side packers).  Every case is exact in fp32 in any summation order; every 8-bit output holds enough ties, inexact values,
representable values and values beyond either clamp; every wrong store and every planted fault changes at least 1 % of what is stored."""
import functools

import numpy as np
import pytest
import torch

import conv_exact_cases as cx
import conv_q8_exact_cases as q8

# every shape under the four 8-bit-input links, the two bf16-input links on one shape
CASES = [(s, l) for l in q8.LINKS[:4] for s in q8.SHAPES] + [(q8.BF16_IN_SHAPE, l) for l in q8.LINKS[4:]]


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _f32_ordered(A, Wm, order, start):
    """start + sum_k A[:, k] * Wm[k] in float32, one term at a time in the given order of k"""
    acc = start.clone()
    for kk in order:
        acc.addcmul_(A[:, kk : kk + 1], Wm[kk : kk + 1])
    return acc


@functools.lru_cache(maxsize=None)
def _f32_sums(shape, src):
    """the accumulator of one shape in float32, in the units the tile counts in (e4m3: 64ths -- the codes hold 64 * w and the bias arrives as 64 * b), in four
    orders: torch's matmul with the bias last, reversed and a seeded permutation with the accumulator STARTING at the bias, 16-term groups summed first"""
    c = q8.q8_link(shape, src + "_bf16" if src != "bf16" else "bf16_i8")
    Cin, Cout = shape[3], shape[4]
    K = 9 * Cin
    unit = 64.0 if src == "f8" else 1.0
    A = cx.taps(c["x"], 3, 1).reshape(-1, K)
    Wm = (c["W"] * unit).reshape(Cout, K).T.contiguous()
    zero = torch.zeros(A.shape[0], Cout, dtype=torch.float32)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)).tolist()
    groups = zero.clone()
    for k0 in range(0, K, 16):
        groups += _f32_ordered(A, Wm, range(k0, min(K, k0 + 16)), zero)
    return A @ Wm, groups, lambda b: _f32_ordered(A, Wm, range(K - 1, -1, -1), zero + b), lambda b: _f32_ordered(A, Wm, perm, zero + b)


@pytest.mark.parametrize("shape,link", CASES, ids=_id)
def test_accumulator_and_value_are_exact_in_every_summation_order(shape, link):
    src = link.split("_")[0]
    c = q8.q8_link(shape, link)
    x, W = c["x"], c["W"]
    assert torch.equal(x, x.round()) and torch.equal(W, W.round()) and torch.equal(c["bias"], c["bias"].round()) and c["alpha"] == 0.5
    assert torch.equal(c["g"].double(), torch.pow(torch.tensor(2.0, dtype=torch.float64), -c["e"].double())) and int(c["e"].abs().max()) <= 6
    if src == "i8":
        spikes = x.abs() == 127
        assert float(x.min()) == -127 and float(x.max()) == 127 and float(x[~spikes].abs().max()) == 3  # never -128
        assert 0.5 / q8.SPIKE_ONE_IN < float(spikes.float().mean()) < 2.0 / q8.SPIKE_ONE_IN
        planted = W.abs() == 127
        assert bool((planted.flatten(1).sum(1) == 1).all()) and float(W[~planted].abs().max()) == 4
        assert torch.equal(W.flatten(1)[planted.flatten(1)], torch.where(torch.arange(shape[4]) % 2 == 0, 127.0, -127.0))
    else:
        assert float(x.abs().max()) == 3 and bool((W.abs().flatten(1).max(1).values == 4).all())
    # int8: |acc| < 2^24 makes float(acc) exact, and acc * 2^-e always is; the other two accumulate in fp32
    unit = 64.0 if src == "f8" else 1.0
    assert q8.abs_sum_bound(c) * unit < 2 ** 24
    want = (q8.conv_sum(c) + c["bias"].double()) * unit
    mm, groups, rev, perm = _f32_sums(shape, src)
    b = c["bias"] * unit
    for name, acc in (("matmul", mm + b), ("groups16", groups + b), ("reversed", rev(b)), ("permuted", perm(b))):
        assert acc.dtype == torch.float32 and torch.equal(acc.reshape(want.shape).double(), want), (shape, link, name)
        v = acc.reshape(want.shape) * q8.kernel_gscale(c)  # fp32 x fp32, as the epilogue
        assert v.dtype == torch.float32 and torch.equal(v.double(), q8.value(c)), (shape, link, name)
    for act in (0, 1):
        q8.exact_f32(q8.value(c, act))
        if link.endswith("bf16"):
            q8.exact_f32(q8.value(c, act, True))
            if link == "i8_bf16" and shape[3] >= shape[4]:
                q8.exact_f32(q8.value(c, act, True, True))
                q8.exact_f32(q8.value(c, act, False, True))
    # the vectors the library is given
    kb = q8.kernel_bias(c)
    if src == "i8":
        assert torch.equal(kb.view(torch.int32).double(), c["bias"].double())
    else:
        assert torch.equal(kb.double() * q8.kernel_gscale(c).double(), (c["bias"] * c["g"]).double())


def test_the_packers_give_the_weight_scales_the_cases_count_on():
    """vgh_pack_conv_weights_i8: one planted +-127 per row -> wscale == 1 and every weight its own code.  vgh_pack_conv_weights_fp8: largest weight 4 -> wscale == 2^-6,
    the codes hold 64 * w (all e4m3 values).  vgh_pack_conv_weights: integers up to 4 are bf16 values."""
    from head_detector_amd import _lib
    from test_gpu_fp8 import _pack_fp8, _unswizzle
    from test_gpu_int8 import _pack_i8

    lib = _lib.load()
    for shape in q8.SHAPES:
        Cin, Cout = shape[3], shape[4]
        W = q8.q8_link(shape, "i8_i8")["W"]
        pack, ws = _pack_i8(lib, W)
        assert bool((ws == 1.0).all()), shape
        codes = torch.from_numpy(_unswizzle(pack, Cout, 3, Cin).view(np.int8).astype(np.float32))
        assert torch.equal(codes, W), shape
        W = q8.q8_link(shape, "f8_f8")["W"]
        pack, ws = _pack_fp8(lib, W)
        assert bool((ws == q8.F8_WSCALE).all()), shape
        codes = torch.from_numpy(_unswizzle(pack, Cout, 3, Cin))
        assert torch.equal(codes, (W * 64.0).to(q8.E4M3).view(torch.uint8)) and torch.equal((W * 64.0).to(q8.E4M3).float(), W * 64.0), shape
        assert torch.equal(W.to(torch.bfloat16).float(), W)
    x = q8.q8_link(q8.SHAPES[0], "f8_f8")["x"]
    assert torch.equal(x.to(q8.E4M3).float(), x) and torch.equal(x.to(torch.bfloat16).float(), x)


def test_stores_are_what_they_say():
    """store_f8's own e4m3 grid against torch's conversion on a dense sweep; the wrong stores on hand-made values of both signs, at the clamps and around zero"""
    g = torch.Generator().manual_seed(8)
    v = torch.cat([torch.randn(20000, generator=g, dtype=torch.float64) * 150.0, torch.arange(-4000, 4000).double() / 8.0, torch.arange(-600, 600).double() / 512.0])
    step = q8._f8_step(v.clamp(-448.0, 448.0))
    mine = torch.round(v.clamp(-448.0, 448.0) / step) * step
    assert torch.equal(mine.float().to(q8.E4M3).float().double(), mine)  # on the grid
    assert torch.equal(q8.store_f8(v, 0).view(q8.E4M3).float().double(), mine)  # torch rounds to the nearest, halves to even, as restated
    assert not bool(((q8.store_f8(v * 4.0, 0) & 0x7F) == 0x7F).any()) and int(q8.store_f8(torch.tensor([1e4, -1e4], dtype=torch.float64), 0)[0]) == 0x7E
    assert q8.store_f8(torch.tensor([1e4, -1e4, 448.0, 460.0], dtype=torch.float64), 0, "nan_overflow").tolist() == [0x7F, 0xFF, 0x7E, 0x7F]
    assert q8.store_f8(torch.tensor([-5.0, 500.0], dtype=torch.float64), 1).tolist() == [0x00, 0x7E]
    f = lambda t, how: q8.store_f8(torch.tensor(t, dtype=torch.float64), 0, how).view(q8.E4M3).float().tolist()
    t = [17.0, 19.0, -17.0, -19.0, 17.5, -18.5, 18.0, 2.0 ** -10, -(2.0 ** -10)]  # [16, 32): steps of 2; below 2^-6: steps of 2^-9
    assert f(t, "rne") == [16.0, 20.0, -16.0, -20.0, 18.0, -18.0, 18.0, 0.0, -0.0]
    assert f(t, "truncate") == [16.0, 18.0, -16.0, -18.0, 16.0, -18.0, 18.0, 0.0, -0.0]
    assert f(t, "half_away") == [18.0, 20.0, -18.0, -20.0, 18.0, -18.0, 18.0, 2.0 ** -9, -(2.0 ** -9)]
    assert q8.store_f8(torch.tensor([-(2.0 ** -10)], dtype=torch.float64), 0, "truncate").tolist() == [0x80] == q8.store_f8(torch.tensor([-(2.0 ** -10)], dtype=torch.float64), 0).tolist()
    cl = [m.tolist() for m in q8.classify_f8(torch.tensor([18.0, 17.0, 17.5, 460.0, -460.0, 448.0], dtype=torch.float64), 0)]
    assert cl == [[True, False, False, True, True, True], [False, True, False, False, False, False], [False, False, True, False, False, False],
                  [False, False, False, True, False, False], [False, False, False, False, True, False]]
    i = lambda t, act, how: q8.store_i8(torch.tensor(t, dtype=torch.float64), act, how).tolist()
    t = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.25, -2.75, 126.5, 127.4, 127.5, 300.0, -127.5, -128.0, -300.0]
    assert i(t, 0, "rne") == [0, 2, 2, 0, -2, -2, 2, -3, 126, 127, 127, 127, -127, -127, -127]
    assert i(t, 0, "truncate") == [0, 1, 2, 0, -1, -2, 2, -2, 126, 127, 127, 127, -127, -127, -127]
    assert i(t, 0, "half_away") == [1, 2, 3, -1, -2, -3, 2, -3, 127, 127, 127, 127, -127, -127, -127]
    assert i(t, 0, "half_up") == [1, 2, 3, 0, -1, -2, 2, -3, 127, 127, 127, 127, -127, -127, -127]
    assert i(t, 0, "clamp_128") == [0, 2, 2, 0, -2, -2, 2, -3, 126, 127, 127, 127, -128, -128, -128]
    assert i(t, 1, "rne") == [0, 2, 2, 0, 0, 0, 2, 0, 126, 127, 127, 127, 0, 0, 0] == i(t, 1, "clamp_128")
    cl = [m.tolist() for m in q8.classify_i8(torch.tensor([3.0, 2.5, 2.25, 127.5, -127.5, -127.0], dtype=torch.float64), 0)]
    assert cl == [[True, False, False, True, True, True], [False, True, False, False, False, False], [False, False, True, False, False, False],
                  [False, False, False, True, False, False], [False, False, False, False, True, False]]
    assert not bool(q8.classify_i8(torch.tensor([-500.0], dtype=torch.float64), 1)[4].any())  # under ReLU the bottom is no clamp of the format's


@pytest.mark.parametrize("shape,link", CASES, ids=_id)
def test_mix_of_outputs_and_visible_wrong_stores(shape, link):
    c = q8.q8_link(shape, link)
    out = link.split("_")[1]
    if out == "bf16":  # cx's floors: ties >= 10 %, >= 5 % with ReLU or a residual
        variants = [(0, False, False), (1, False, False), (1, True, False)] + ([(0, False, True), (1, True, True)] if link == "i8_bf16" and shape[3] >= shape[4] else [])
        for act, with_res, diag in variants:
            v = q8.exact_f32(q8.value(c, act, with_res, diag))
            exact, tie, inexact = (float(m.float().mean()) for m in cx.classify(v, cx.BF16))
            print(f"[q8 exact] {shape} {link} act={act} res={with_res} diag={diag}: exact {exact:.3f} ties {tie:.3f} inexact {inexact:.3f} max |v| {float(v.abs().max()):.0f}")
            assert tie >= (0.10 if (act, with_res, diag) == (0, False, False) else 0.05) and inexact >= 0.20 and exact >= 0.10, (exact, tie, inexact)
            good = cx.rne(v, cx.BF16)
            cx.storage_bits(good, cx.BF16)
            for name, fn in cx.WRONG_ROUNDINGS.items():
                d = float((fn(v, cx.BF16) != good).float().mean())
                assert d >= 0.025, (name, d)
        return
    for act in (0, 1):
        v = q8.value(c, act)
        q8.exact_f32(v)
        exact, tie, inexact, top, bottom = (float(m.float().mean()) for m in q8.CLASSIFY[out](v, act))
        print(f"[q8 exact] {shape} {link} act={act}: exact {exact:.3f} ties {tie:.3f} inexact {inexact:.3f} top clamp {top:.3f} bottom clamp {bottom:.3f}")
        assert tie >= 0.03 and inexact >= 0.20 and exact >= 0.10 and top >= 0.01 and (act == 1 or bottom >= 0.01), (exact, tie, inexact, top, bottom)
        assert exact + tie + inexact == pytest.approx(1.0)
        good = q8.STORE[out](v, act)
        assert torch.equal(good, q8.expected(c, act))
        if out == "i8":
            assert int(good.min()) == (0 if act else -127) and int(good.max()) == 127
        else:
            assert not bool(((good & 0x7F) == 0x7F).any()) and int(good.max()) == (0x7E if act else 0xFE) and bool((good == 0x7E).any())
        for how in q8.WRONG_STORES[out]:
            if how == "clamp_128" and act == 1:
                continue  # (the ReLU's zero is the bottom there)
            d = float((q8.STORE[out](v, act, how) != good).float().mean())
            print(f"[q8 exact]   {how} differs from the correct store in {d:.3f}")
            assert d >= 0.01, (how, d)


@pytest.mark.parametrize("shape,link", CASES, ids=_id)
def test_planted_faults_are_visible_after_the_store(shape, link):
    c = q8.q8_link(shape, link)
    src, out = link.split("_")
    store = (lambda v, act: cx.rne(q8.exact_f32(v), cx.BF16)) if out == "bf16" else (lambda v, act: q8.STORE[out](v, act))
    res = out == "bf16"
    faults = ["tap_shift", "drop_channel", "bias_real_units", "swap_runs"] + (["x_unsigned"] if src == "i8" else []) + (["res_before_act"] if res else [])
    for act in (0, 1):
        clean = store(q8.value(c, act, res and act == 1), act)
        for fault in faults:
            if fault == "res_before_act" and act == 0:
                continue
            d = float((store(q8.value(c, act, res and act == 1, fault=fault), act) != clean).float().mean())
            print(f"[q8 exact] {shape} {link} act={act}: {fault} changes {d:.3f}")
            assert d >= 0.01, (fault, act, d)
    if link == "i8_bf16" and shape[3] >= shape[4]:
        for act, with_res in ((0, False), (1, True)):
            clean = store(q8.value(c, act, with_res, True), act)
            assert float((clean != store(q8.value(c, act, with_res, False), act)).float().mean()) >= 0.25  # the bypass itself
            for fault in ("diag_next_channel", "x_unsigned", "swap_runs"):
                d = float((store(q8.value(c, act, with_res, True, fault=fault), act) != clean).float().mean())
                print(f"[q8 exact] {shape} {link} bypass act={act}: {fault} changes {d:.3f}")
                assert d >= 0.01, (fault, act, d)
        # +-127 on the diagonal channels themselves
        diag_x = c["x"][..., : shape[4]]
        assert bool((diag_x == 127).any()) and bool((diag_x == -127).any())


def test_cases_are_seeded_and_share_operands_by_input_format():
    s = q8.SHAPES[2]
    a, b = q8.q8_link(s, "i8_bf16"), q8.q8_link(s, "i8_i8")
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["W"], b["W"]) and not torch.equal(a["bias"], b["bias"])
    q8.q8_link.cache_clear()
    q8._i8_operands.cache_clear()
    a2 = q8.q8_link(s, "i8_bf16")
    assert a2 is not a and all(torch.equal(a[k], a2[k]) for k in ("x", "W", "res", "bias", "e", "g", "diag"))
    assert not torch.equal(a["x"], q8.q8_link(s, "i8_bf16", 1)["x"])
    f, h = q8.q8_link(s, "f8_f8"), q8.q8_link(s, "f8_bf16")
    assert f["x"] is cx.exact_case(*s, 3, 1, 0, cx.BF16)["x"] and torch.equal(f["W"], h["W"])
    assert len(q8.E_OFFSETS) == len(q8.BIAS_SIGMAS) == len(q8.DIAG_TABLE) == 16 and 0 not in q8.DIAG_TABLE
    for link in ("i8_i8", "bf16_i8"):
        assert int(q8.q8_link(q8.SHAPES[0], link)["e"].min()) >= 1  # no int8 store of bare integers
