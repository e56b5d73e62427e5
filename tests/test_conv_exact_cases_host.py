"""No GPU, no library: the conditions under which tests/test_gpu_conv_exact.py means something, checked on tests/conv_exact_cases.py alone.  Every case is exact in
fp32 in any summation order, holds enough ties, inexact values and representable values for its storage width, and tells the three wrong roundings and three
structural faults from the correct result."""
import functools

import pytest
import torch

import conv_exact_cases as cx

STORAGES = (cx.BF16, cx.FP16)


def _ids(shape):
    return "x".join(str(v) for v in shape)


def _f32_ordered(A, Wm, order):
    """sum_k A[:, k] * Wm[k] in float32, one term at a time in the given order of k"""
    acc = torch.zeros(A.shape[0], Wm.shape[1], dtype=torch.float32)
    for kk in order:
        acc.addcmul_(A[:, kk : kk + 1], Wm[kk : kk + 1])
    return acc


@functools.lru_cache(maxsize=None)
def _f32_sums(shape):
    """the conv sum (no bias) of one shape in float32, in four orders: torch's own matmul, reversed, a seeded permutation, 16-term groups summed first"""
    c = cx.exact_case(*shape, 0, cx.BF16)
    _, _, _, Cin, Cout, k, stride = shape
    K = k * k * Cin
    A = cx.taps(c["x"], k, stride).reshape(-1, K)
    Wm = c["W"].reshape(Cout, K).T.contiguous()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)).tolist()
    groups = torch.zeros(A.shape[0], Cout, dtype=torch.float32)
    for k0 in range(0, K, 16):
        groups += _f32_ordered(A, Wm, range(k0, min(K, k0 + 16)))
    return {"matmul": A @ Wm, "reversed": _f32_ordered(A, Wm, range(K - 1, -1, -1)), "permuted": _f32_ordered(A, Wm, perm), "groups16": groups}


@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_every_summation_order_is_exact(shape):
    _, _, _, Cin, Cout, k, stride = shape
    sums = _f32_sums(shape)
    for storage in STORAGES:
        c = cx.exact_case(*shape, 0, storage)
        assert all(float(c[n].abs().max()) <= m and torch.equal(c[n], c[n].round()) for n, m in (("x", cx.X_MAX), ("W", cx.W_MAX), ("res", cx.RES_MAX)))
        assert torch.equal(c["bias"], c["bias"].round()) and c["alpha"] == 0.5
        for with_res in (False, True):
            assert cx.abs_sum_bound(c, with_res) < 2 ** 16
        ref = cx.reference(c)
        for name, s in sums.items():
            # bias last (matmul, reversed, groups) and bias first (permuted: the accumulator starts from it, as a kernel may)
            y = (s + c["bias"]) if name != "permuted" else (c["bias"] + s)
            assert y.dtype == torch.float32 and torch.equal(y.reshape(ref.shape).double(), ref), (shape, storage, name)
        for act in (0, 1):
            y = cx.reference(c, act, True)
            y32 = (torch.relu(sums["matmul"] + c["bias"]) if act else sums["matmul"] + c["bias"]).reshape(y.shape) + c["alpha"] * c["res"]
            assert y32.dtype == torch.float32 and torch.equal(y32.double(), y), (shape, storage, act)
        lim = 65504.0 if storage == cx.FP16 else 2.0 ** 16
        assert float(ref.abs().max()) < lim and float(cx.reference(c, 1, True).abs().max()) < lim


def test_reference_equals_torch_conv2d():
    """the explicit-padding im2col against torch's own convolution (float64), both strides and kernel sizes"""
    import torch.nn.functional as F

    for shape in (cx.SHAPES[0], cx.SHAPES[2], cx.SHAPES[7]):
        c = cx.exact_case(*shape, 0, cx.BF16)
        k, stride = shape[5], shape[6]
        y = F.conv2d(c["x"].double().permute(0, 3, 1, 2), c["W"].double().permute(0, 3, 1, 2), c["bias"].double(), stride=stride, padding=k // 2).permute(0, 2, 3, 1)
        assert torch.equal(cx.reference(c), y)
        assert torch.equal(cx.reference(c, 1, True), torch.relu(y) + 0.5 * c["res"].double())


@pytest.mark.parametrize("storage", STORAGES)
def test_roundings_are_what_they_say(storage):
    """rne against torch's own conversion on a dense sweep; the wrong roundings on hand-made values of both signs; +-0, subnormals and non-finite values left alone"""
    drop = 24 - storage
    g = torch.Generator().manual_seed(storage)
    y = torch.cat([torch.randn(20000, generator=g) * 300.0, torch.arange(-5000, 5000).float(), torch.arange(-5000, 5000).float() * 0.5, torch.arange(30000, 34000).float()])
    dt = torch.bfloat16 if storage == cx.BF16 else torch.float16
    assert torch.equal(cx.rne(y, storage).view(torch.int32), y.to(dt).float().view(torch.int32))
    one = 2.0 ** storage  # the first integer whose neighbours in the storage are 2 apart
    v = torch.tensor([one + 1, one + 3, -(one + 1), -(one + 3), one + 0.5, -(one + 0.5), one + 1.5, -(one + 1.5), one + 2, -(one + 2)], dtype=torch.float32)
    want = {
        "rne": [one, one + 4, -one, -(one + 4), one, -one, one + 2, -(one + 2), one + 2, -(one + 2)],
        "truncate": [one, one + 2, -one, -(one + 2), one, -one, one, -one, one + 2, -(one + 2)],
        "half_up": [one + 2, one + 4, -one, -(one + 2), one, -one, one + 2, -(one + 2), one + 2, -(one + 2)],
        "half_away": [one + 2, one + 4, -(one + 2), -(one + 4), one, -one, one + 2, -(one + 2), one + 2, -(one + 2)],
    }
    for name, fn in dict(cx.WRONG_ROUNDINGS, rne=cx.rne).items():
        assert fn(v, storage).tolist() == want[name], name
        assert torch.equal(fn(v, storage), fn(fn(v, storage), storage))
        special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
        assert torch.equal(fn(special, storage).view(torch.int32), special.view(torch.int32)), name
    exact, tie, inexact = cx.classify(v, storage)
    assert exact.tolist() == [False] * 8 + [True] * 2 and tie.tolist() == [True] * 4 + [False] * 6 and inexact.tolist() == [False] * 4 + [True] * 4 + [False] * 2
    assert (1 << drop) == {cx.BF16: 65536, cx.FP16: 8192}[storage]
    assert cx.storage_bits(torch.tensor([0.0, -0.0]), storage).tolist() == [0, -32768]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_mix_of_outputs_and_visible_roundings(shape, storage):
    c = cx.exact_case(*shape, 0, storage)
    y = cx.reference(c).float()
    exact, tie, inexact = (float(m.float().mean()) for m in cx.classify(y, storage))
    print(f"[conv exact] {shape} bits={storage}: exact {exact:.3f} ties {tie:.3f} inexact {inexact:.3f} max |y| {float(y.abs().max()):.0f}")
    assert tie >= 0.10 and inexact >= 0.20 and exact >= 0.20, (exact, tie, inexact)
    yr = cx.reference(c, 1, False).float()
    assert float(cx.classify(yr, storage)[1].float().mean()) >= 0.05
    assert float(cx.classify(cx.reference(c, 1, True).float(), storage)[1].float().mean()) >= 0.05  # (with the half-integer residual the ties move, they do not vanish)
    good = cx.rne(y, storage)
    assert torch.equal(good, cx.expected(c, storage))
    cx.storage_bits(good, storage)  # representable
    for name, fn in cx.WRONG_ROUNDINGS.items():
        d = float((fn(y, storage) != good).float().mean())
        print(f"[conv exact]   {name} differs from rne in {d:.3f}")
        assert d >= 0.05, (name, d)
        assert float((fn(yr, storage) != cx.rne(yr, storage)).float().mean()) >= 0.025, name  # ReLU halves what is left to round


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_structural_faults_are_visible_after_the_store(shape, storage):
    c = cx.exact_case(*shape, 0, storage)
    clean = cx.expected(c, storage, 1, True)
    for fault in cx.FAULTS:
        y = cx.reference(c, 1, True, fault=fault).float()
        d = float((cx.rne(y, storage) != clean).float().mean())
        assert d >= 0.01, (fault, d)
    clean0 = cx.expected(c, storage, 0, False)
    for fault in cx.FAULTS[:2]:
        d = float((cx.rne(cx.reference(c, 0, False, fault=fault).float(), storage) != clean0).float().mean())
        assert d >= 0.01, (fault, d)


def test_cases_are_seeded_and_shared_across_storages():
    a, b = cx.exact_case(*cx.SHAPES[2], 0, cx.BF16), cx.exact_case(*cx.SHAPES[2], 0, cx.FP16)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["W"], b["W"]) and torch.equal(a["res"], b["res"]) and not torch.equal(a["bias"], b["bias"])
    assert not torch.equal(a["x"], cx.exact_case(*cx.SHAPES[2], 1, cx.BF16)["x"])
    assert len(cx.BIAS_TABLE[cx.BF16]) == len(cx.BIAS_TABLE[cx.FP16]) == 16 and max(map(abs, cx.BIAS_TABLE[cx.FP16])) < 40000
    z = cx.pixel_shuffle(torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(1, 2, 3, 8))
    assert z.shape == (1, 4, 6, 2) and z[0, 1, 0].tolist() == [4.0, 5.0] and z[0, 0, 1].tolist() == [2.0, 3.0]
