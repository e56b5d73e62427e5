"""GPU (-m gpu): every conv tile on exact-arithmetic operands (tests/conv_exact_cases.py) -- small integers, so that the fp32 accumulator of a correct tile is the same
number in any K order, ring depth, MFMA shape or split, and what is stored is ONE well-defined rounding of it.  Every comparison here is an equality of bits against
this file's own float64 reference: the bf16 tiles of csrc/conv_kernels.inc, conv_pp.hip, conv_patch.hip, conv_rings.hip and ds_b2b.hip through each of their store
paths (LDS-transposed 16-byte epilogue, general epilogue, both fp32 epilogues, the ping-pong tiles' register epilogue, two-segment store, pixel-shuffle store), the
two split formats and the single-plane fp16 mode of csrc/conv_split.hip.  A store that truncates or rounds halves up, one product dropped from or repeated in a long K
loop, a lost sign of zero: each is a failure here, and the message says which wrong rounding, if any, reproduces the output.  tests/test_conv_exact_cases_host.py
shows on the CPU that the cases can tell these apart.

Also: images and pixels are independent (include/vgh.h, vgh_net_set_split).  Non-finite values planted in four pixels of image 0 and in one pixel of the residual
change only the outputs whose receptive field holds them."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as cx

pytestmark = pytest.mark.gpu

SENTINEL = -768.0  # what the helpers prefill the output with: exactly representable in bf16, fp16 and both split formats
# runs per shape that do not depend on the map: the automatic tile and every tile of a family without launch-time conditions (all but r / w / s) that
# vgh_conv_cfg_ok admits, under both epilogues -- counted from the tile table as it stands; a pull request that retires tiles lowers these on purpose
MIN_RUNS = dict(zip(cx.SHAPES, (21, 20, 49, 164, 132, 164, 164, 106, 106, 49, 117)))


def _ids(shape):
    return "x".join(str(v) for v in shape)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """float32 tensors, bit for bit (-0 against +0 counts; a 16-bit store widened to float32 has equal int16 views exactly when these are equal)"""
    return torch.equal(_bits(got), _bits(want))


def _store(y32, storage):
    """what a correct tile stores of the exact float32 value, widened back to float32; storage None: an fp32 output, the value itself"""
    if storage is None:
        return y32
    s = cx.rne(y32, storage)
    cx.storage_bits(s, storage)  # (asserts that the expectation is representable)
    return s


def _check(out, parts, storage, where):
    """out: the whole output buffer as float32 [B,H,W,pitch]; parts: [(channel offset, exact float32 value [B,H,W,n])]: those channels hold the correct rounding of
    the value bit for bit, every other channel still holds the sentinel."""
    want = torch.full_like(out, SENTINEL)
    for off, y in parts:
        want[..., off : off + y.shape[-1]] = _store(y, storage)
    if _same(out, want):
        return
    live = torch.zeros(out.shape[-1], dtype=torch.bool)
    for off, y in parts:
        live[off : off + y.shape[-1]] = True
    bad = _bits(out) != _bits(want)
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    msg = [f"{where}: {int(bad.sum())} of {int(live.sum()) * bad[..., 0].numel()} stored values differ, {int(bad[..., ~live].sum())} outside the stored channels; "
           f"first {idx[:5].tolist()} (b, y, x, channel of the buffer); at {first} got {float(out[first])!r} want {float(want[first])!r}"]
    if storage is not None:
        hit = []
        for name, fn in cx.WRONG_ROUNDINGS.items():
            alt = torch.full_like(out, SENTINEL)
            for off, y in parts:
                alt[..., off : off + y.shape[-1]] = fn(y, storage)
            if _same(out, alt):
                hit.append(name)
        msg.append(f"reproduced exactly by: {', '.join(hit)}" if hit else "reproduced by none of truncate / half_up / half_away")
    pix = (idx[:, 1] * out.shape[2] + idx[:, 2]) % 32
    msg.append(f"pixel%32 hist {torch.bincount(pix, minlength=32).tolist()}; chan%32 hist {torch.bincount(idx[:, 3] % 32, minlength=32).tolist()}; "
               f"image hist {torch.bincount(idx[:, 0], minlength=out.shape[0]).tolist()}")
    raise AssertionError("\n".join(msg))


def _names(lib):
    return [lib.vgh_conv_cfg_name(i).decode() for i in range(lib.vgh_conv_num_cfgs())]


def _tile(names, cfg):
    return names[cfg] if cfg >= 0 else "auto"


# ======================================================================================================
# bf16: every tile, both epilogues
# ======================================================================================================
@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_every_bf16_tile_stores_the_nearest_even_rounding_of_the_exact_sum(gpu_lib, shape):
    from test_gpu_parity import _LaunchPredicate, _run_conv

    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.BF16)
    y = cx.reference(c).float()
    rp = (Cout + 31) // 32 * 32
    out_f32 = Cout % 4 != 0
    names = _names(gpu_lib)
    launch_ok = {oc0: _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride, out_coff=oc0, out_f32=out_f32) for oc0 in (8, 4)}
    refused, tested, n_s = set(), 0, 0
    try:
        for cfg in [-1] + list(range(len(names))):
            for oc0 in (8, 4):  # 8: LDS-transposed 16-byte epilogue (when Cout % 8 == 0); 4: general epilogue
                fast = int(oc0 == 8 and Cout % 8 == 0 and not out_f32)
                if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, k, stride, rp, fast, 0):
                    continue
                if cfg >= 0 and not launch_ok[oc0](cfg):
                    refused.add(names[cfg])
                    continue
                out, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=0, cfg=cfg, out_f32=out_f32, out_coff=oc0)
                assert st == Cout and o0 == oc0
                _check(out, [(o0, y)], None if out_f32 else cx.BF16, f"{shape} tile {_tile(names, cfg)} out_coff={oc0}")
                tested += 1
                n_s += cfg >= 0 and names[cfg][0] == "s"
    finally:
        for p_ in launch_ok.values():
            p_.close()
    assert all(n[0] in "rws" for n in refused), f"only the r / w / s tiles have launch-time conditions on the map: {sorted(refused)}"
    assert tested >= MIN_RUNS[shape], (tested, sorted(refused))
    if shape == (2, 23, 45, 96, 192, 3, 2):
        assert sorted(refused) == ["r8x8x96_n4"]
    if shape == (2, 32, 48, 96, 192, 3, 2):
        assert not refused  # the r tile ran
    if shape == (5, 24, 32, 96, 96, 3, 1):
        assert not [n for n in refused if n[0] == "w"]  # the w tile ran
    if shape in ((3, 9, 19, 192, 192, 3, 1), (2, 11, 13, 96, 96, 3, 1)):
        assert not [n for n in refused if n[0] == "s"] and n_s >= 1, (sorted(refused), n_s)


@pytest.mark.parametrize("shape", [(2, 40, 40, 64, 128, 3, 1), (5, 24, 32, 96, 96, 3, 1), (2, 32, 48, 96, 192, 3, 2), (2, 19, 19, 576, 192, 1, 1)], ids=_ids)
def test_bf16_tiles_stay_exact_with_many_tiles_per_workgroup(gpu_lib, shape):
    """The persistent kernels with their grid capped to 2 workgroups per XCD: tile loops, operand streams and rings that run across tiles, cout-tile changes between
    consecutive tiles of a workgroup, ragged last tiles.  Plain, and with the residual where the tile takes one."""
    from test_gpu_parity import _LaunchPredicate, _run_conv

    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.BF16)
    y, y_res = cx.reference(c, 1, False).float(), cx.reference(c, 1, True).float()
    names = _names(gpu_lib)
    ok = {r: _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride, res=r) for r in (False, True)}
    tested = 0
    try:
        assert gpu_lib.vgh_conv_set_max_blocks_per_xcd(2) == 0
        for cfg in range(-1, len(names)):
            if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, k, stride, Cout, 1, 0):
                continue
            for with_res in (False, True):
                if cfg >= 0 and not ok[with_res](cfg):
                    continue
                out, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=1, res=c["res"] if with_res else None, alpha=c["alpha"] if with_res else 0.0, cfg=cfg)
                _check(out, [(o0, y_res if with_res else y)], cx.BF16, f"{shape} 2 workgroups per XCD, tile {_tile(names, cfg)} res={with_res}")
                tested += 1
    finally:
        gpu_lib.vgh_conv_set_max_blocks_per_xcd(0)
        for p_ in ok.values():
            p_.close()
    assert tested >= MIN_RUNS[shape] // 2, tested


# ======================================================================================================
# bf16: every epilogue
# ======================================================================================================
EPILOGUE_SHAPES = [(2, 12, 12, 64, 128, 3, 1), (2, 12, 12, 64, 128, 1, 1), (2, 11, 13, 64, 96, 3, 1), (2, 11, 13, 64, 128, 3, 1)]


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES, ids=_ids)
def test_bf16_residual_and_two_segment_stores_are_exact_under_every_tile(gpu_lib, shape):
    """ReLU, then + 0.5 * residual in fp32, then the one rounding (both epilogues); the output in two channel segments; an input view at a channel offset inside
    a wider pixel.  Every tile that the library admits for that very launch."""
    from test_gpu_parity import _LaunchPredicate, _run_conv

    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.BF16)
    y_res, y_relu = cx.reference(c, 1, True).float(), cx.reference(c, 1, False).float()
    names = _names(gpu_lib)
    h = Cout // 2
    ok_res = {oc0: _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride, out_coff=oc0, res=True) for oc0 in (8, 4)}
    ok_seg = _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride, split=(h, h + 8, 0))
    ok_in = _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride)  # (the launch rules ask in_coff % 8 and in_pitch % 8 only: 32 / Cin + 64 answer as 0 / Cin do)
    n_res = n_seg = n_in = 0
    try:
        for cfg in range(-1, len(names)):
            for oc0 in (8, 4):
                if cfg >= 0 and not (gpu_lib.vgh_conv_cfg_ok(cfg, k, stride, Cout, int(oc0 == 8), 0) and ok_res[oc0](cfg)):
                    continue
                out, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=1, res=c["res"], alpha=c["alpha"], cfg=cfg, out_coff=oc0)
                _check(out, [(o0, y_res)], cx.BF16, f"{shape} residual, tile {_tile(names, cfg)} out_coff={oc0}")
                n_res += 1
            if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, k, stride, Cout, 1, 0):
                continue
            if cfg < 0 or ok_seg(cfg):  # first h rows at offset h + 8, the rest at offset 0
                out, _, _, _ = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=1, split=(h, h + 8, 0), cfg=cfg)
                _check(out, [(h + 8, y_relu[..., :h]), (0, y_relu[..., h:])], cx.BF16, f"{shape} two segments, tile {_tile(names, cfg)}")
                n_seg += 1
            if cfg < 0 or ok_in(cfg):
                out, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=1, in_coff=32, in_pitch=Cin + 64, cfg=cfg)
                _check(out, [(o0, y_relu)], cx.BF16, f"{shape} input view at channel 32, tile {_tile(names, cfg)}")
                n_in += 1
    finally:
        for p_ in list(ok_res.values()) + [ok_seg, ok_in]:
            p_.close()
    # the launch-time predicate may refuse the r / w / s tiles (conditions on the map and the input channels) and, with a residual, the streaming t tiles -- nothing else:
    # the automatic tile and every other admitted tile ran
    free = lambda fast, cond: sum(1 for i, n in enumerate(names) if n[0] not in cond and gpu_lib.vgh_conv_cfg_ok(i, k, stride, Cout, fast, 0))
    assert free(1, "rws") >= 10 and n_res >= 2 + free(1, "rwst") + free(0, "rwst") and n_seg >= 1 + free(1, "rws") and n_in >= 1 + free(1, "rws"), (n_res, n_seg, n_in)


@pytest.mark.parametrize("rows", [69, 13])
def test_fp32_outputs_equal_the_float64_reference_through_both_fp32_epilogues(gpu_lib, rows):
    """Prediction convs: 69 and 13 live channels of a padded 96 / 32, fp32 store.  out_coff 8: the transposed float4 epilogue; out_coff 5: the general one."""
    from test_gpu_parity import _run_conv

    shape = (2, 12, 12, 64, rows, 1, 1)
    c = cx.exact_case(*shape, 0, cx.BF16)
    y = cx.reference(c).float()
    names = _names(gpu_lib)
    rp = (rows + 31) // 32 * 32
    n = 0
    for cfg in range(-1, len(names)):
        if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, 1, 1, rp, 0, 0):
            continue
        for oc0 in (8, 5):
            out, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], 1, 1, act=0, out_f32=True, out_coff=oc0, cfg=cfg)
            _check(out, [(oc0, y)], None, f"fp32 output, {rows} channels, tile {_tile(names, cfg)} out_coff={oc0}")
            n += 1
    assert n >= 6, n


def test_pixel_shuffle_store_is_exact_under_every_tile(gpu_lib):
    """ConvTranspose2d(k=2, s=2) as four pointwise GEMMs + the pixel-shuffle store: 4 x 96 rows -> 96 channels on the doubled map, both epilogues."""
    from test_gpu_parity import _run_conv

    Ct = 96
    shape = (2, 12, 12, 96, 4 * Ct, 1, 1)
    c = cx.exact_case(*shape, 0, cx.BF16)
    y = cx.pixel_shuffle(cx.reference(c).float())
    names = _names(gpu_lib)
    n = 0
    for oc0 in (8, 4):
        for cfg in range(-1, len(names)):
            if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, 1, 1, 4 * Ct, int(oc0 == 8), 1):
                continue
            out, _, _, _ = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], 1, 1, act=0, shuffle=True, out_coff=oc0, cfg=cfg)
            _check(out, [(oc0, y)], cx.BF16, f"pixel shuffle, tile {_tile(names, cfg)} out_coff={oc0}")
            n += 1
    assert n >= 4, n


# ======================================================================================================
# the parity (two-plane) formats and the single-plane fp16 mode
# ======================================================================================================
@pytest.mark.parametrize("fmt", ["f16x2", "bf16x2"])
@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_split_tiles_hold_the_exact_sum_in_their_two_planes(gpu_lib, shape, fmt):
    """Integers below 2^16 fit the 16 significand bits of two bf16 planes (and the 22 of two fp16 planes): the joined output IS the float64 reference.  A forced
    tile that the launch refuses runs the launcher's own pick under that name -- the same bits are due either way."""
    import test_gpu_split as ts

    fmt = {"f16x2": ts.FMT_F16X2, "bf16x2": ts.FMT_BF16X2}[fmt]
    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.BF16)
    y = cx.reference(c)
    rp = (Cout + 31) // 32 * 32
    out_f32 = Cout % 4 != 0  # 16-bit planes are written in groups of 4 channels
    n_cfg = gpu_lib.vgh_conv_split_num_cfgs() - 3  # (the last three are the single-plane fp16 ping-pong tiles)
    tested = 0
    for cfg in range(-1, n_cfg):
        if cfg >= 0 and not gpu_lib.vgh_conv_split_cfg_ok(cfg, k, stride, rp, int(Cout % 8 == 0 and not out_f32), 0, 0):
            continue
        out, _, st, o0 = ts._run_conv_split(gpu_lib, fmt, c["x"], c["W"], c["bias"], k, stride, act=0, out_f32=out_f32, cfg=cfg)
        name = gpu_lib.vgh_conv_split_cfg_name(cfg).decode() if cfg >= 0 else "auto"
        got = out[..., o0 : o0 + st].double()
        bad = got != y
        assert not bool(bad.any()), f"{shape} fmt {fmt} tile {name}: {int(bad.sum())} of {bad.numel()} differ, first {bad.nonzero()[:5].tolist()}, got {got[bad][:5].tolist()} want {y[bad][:5].tolist()}"
        assert bool((out[..., :o0] == SENTINEL).all()) and bool((out[..., o0 + st :] == SENTINEL).all()), f"{shape} fmt {fmt} tile {name}: guard channels overwritten"
        tested += 1
    assert tested >= 3, tested


F16_RESIDUAL_SHAPES = ((2, 11, 13, 96, 96, 3, 1), (2, 40, 40, 64, 128, 3, 1))  # a ragged map; a map that the fp16 ping-pong tiles take


@pytest.mark.parametrize("shape", cx.SHAPES, ids=_ids)
def test_single_plane_fp16_tiles_store_the_nearest_even_rounding(gpu_lib, shape):
    """VGH_FMT_F16 under the fp16 bias table (ties from |y| = 2048 on, everything far below 65 504); the per-op power-of-two weight prescale keeps integer weights
    exact.  Two shapes again with ReLU and + 0.5 * residual before the one rounding."""
    import test_gpu_fp16 as tf

    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.FP16)
    rp = (Cout + 31) // 32 * 32
    out_f32 = Cout % 4 != 0
    names = [gpu_lib.vgh_conv_split_cfg_name(i).decode() for i in range(gpu_lib.vgh_conv_split_num_cfgs())]
    variants = [(0, False)] + ([(1, True)] if shape in F16_RESIDUAL_SHAPES else [])
    tested = pp = 0
    for act, with_res in variants:
        y = cx.reference(c, act, with_res).float()
        for cfg in range(-1, len(names)):
            if cfg >= 0 and not gpu_lib.vgh_conv_split_cfg_ok(cfg, k, stride, rp, int(Cout % 8 == 0 and not out_f32), 0, 0):
                continue
            if cfg >= len(names) - 3 and (k != 3 or stride != 1 or rp != Cout):
                continue
            out, _, st, o0 = tf._run_conv_f16(gpu_lib, c["x"], c["W"], c["bias"], k, stride, act=act, res=c["res"] if with_res else None, alpha=c["alpha"] if with_res else 0.0,
                                              cfg=cfg, out_f32=out_f32)
            assert st == Cout
            _check(out, [(o0, y)], None if out_f32 else cx.FP16, f"{shape} fp16 act={act} res={with_res} tile {_tile(names, cfg)}")
            tested += 1
            pp += cfg >= len(names) - 3
    assert tested >= 3 * len(variants) and (pp >= 1 or not (k == 3 and stride == 1 and Cout % 64 == 0))


# ======================================================================================================
# images and pixels are independent
# ======================================================================================================
def _poisoned(c, shape):
    """(x, res, untouched): four pixels of image 0 set in a few channels to +Inf, -Inf, NaN and bf16's largest finite value -- two of them on the map's border,
    one the last pixel of the image -- and a NaN in one pixel of the residual; untouched [B,Ho,Wo,Cout] marks every output whose receptive field holds none of them."""
    B, H, W, Cin, Cout, k, stride = shape
    Ho, Wo = cx.out_hw(H, W, k, stride)
    x, res = c["x"].clone(), c["res"].clone()
    big = float(torch.tensor(float.fromhex("0x1.fep127")).to(torch.bfloat16))
    # (the first at odd coordinates: under stride 2 four outputs read it)
    pix = [((H // 2 | 1, W // 2 | 1), float("inf")), ((0, W // 3), float("-inf")), ((H // 3, W - 2), float("nan")), ((H - 1, W - 1), big)]
    hit = torch.zeros(1, 1, H, W)
    for i, ((py, px), v) in enumerate(pix):
        x[0, py, px, [3 + i, Cin // 2, Cin - 1 - i]] = v
        hit[0, 0, py, px] = 1.0
    field = F.conv2d(hit, torch.ones(1, 1, k, k), stride=stride, padding=k // 2)[0, 0] > 0  # [Ho,Wo]: the outputs that read a planted pixel
    untouched = torch.ones(B, Ho, Wo, Cout, dtype=torch.bool)
    untouched[0] = ~field[..., None]
    ry, rx = Ho - 1, Wo // 2
    res[0, ry, rx, 5:9] = float("nan")
    untouched_res = untouched.clone()
    untouched_res[0, ry, rx, 5:9] = False
    return x, res, untouched, untouched_res


@pytest.mark.parametrize("shape", [(2, 11, 13, 96, 96, 3, 1), (2, 32, 48, 96, 192, 3, 2)], ids=_ids)
def test_non_finite_pixels_change_only_their_own_receptive_fields(gpu_lib, shape):
    """Linear pixel tiles straddle images and halo patches read neighbours; a tile that lets a value leak (a product with a zero that should have been a skipped
    load: Inf x 0 = NaN) shows here.  Every tile runs with the residual where it takes one and without where it does not (the r tile).  What lies inside the
    receptive fields is not compared: the kernels' fmaxf ReLU and torch's treat NaN differently on purpose."""
    from test_gpu_parity import _LaunchPredicate, _run_conv

    B, H, W, Cin, Cout, k, stride = shape
    c = cx.exact_case(*shape, 0, cx.BF16)
    x_bad, res_bad, untouched, untouched_res = _poisoned(c, shape)
    assert float(untouched[0].float().mean()) > 0.5 and bool(untouched[1:].all()) and int((~untouched[0, ..., 0]).sum()) >= 4
    names = _names(gpu_lib)
    ok = {r: _LaunchPredicate(gpu_lib, B, H, W, Cin, Cout, k, stride, res=r) for r in (True, False)}
    tested = 0
    try:
        for cfg in range(-1, len(names)):
            if cfg >= 0 and not gpu_lib.vgh_conv_cfg_ok(cfg, k, stride, Cout, 1, 0):
                continue
            with_res = cfg < 0 or ok[True](cfg)
            if not with_res and not ok[False](cfg):
                continue
            kw = dict(act=1, cfg=cfg)
            clean, _, st, o0 = _run_conv(gpu_lib, c["x"], c["W"], c["bias"], k, stride, res=c["res"] if with_res else None, alpha=c["alpha"] if with_res else 0.0, **kw)
            dirty, _, _, _ = _run_conv(gpu_lib, x_bad, c["W"], c["bias"], k, stride, res=res_bad if with_res else None, alpha=c["alpha"] if with_res else 0.0, **kw)
            _check(clean, [(o0, cx.reference(c, 1, with_res).float())], cx.BF16, f"{shape} clean run, tile {_tile(names, cfg)} res={with_res}")
            keep = torch.ones(clean.shape, dtype=torch.bool)  # the guard channels count: nothing may reach them either
            keep[..., o0 : o0 + st] = untouched_res if with_res else untouched
            bad = (_bits(clean) != _bits(dirty)) & keep
            assert not bool(bad.any()), (f"{shape} tile {_tile(names, cfg)} res={with_res}: {int(bad.sum())} outputs outside every receptive field changed, "
                                         f"{int(bad[1:].sum())} of them in image 1; first {bad.nonzero()[:5].tolist()}")
            assert bool((_bits(clean) != _bits(dirty))[0].any())  # (the planted values did arrive)
            tested += 1
    finally:
        for p_ in ok.values():
            p_.close()
    assert tested >= MIN_RUNS[shape] // 2, tested
