"""GPU (-m gpu): the 8-bit g-tile variants of csrc/conv_pp.hip (e4m3: F8 / O8 = 1, int8: F8 / O8 = 2, the diagonal bypass DG) on the exact-arithmetic operands of
tests/conv_q8_exact_cases.py, through vgh_conv2d.  Operands are their own codes in every format on the path, every factor g[c] is a power of two and the bias is an
integer in accumulator units, so a correct tile holds one fp32 value before its store and every comparison here is an equality of bytes (8-bit outputs) or of bf16
bits: the clamp on the right side of the rounding, ties to even, the half-wave exchanges that put 16 consecutive couts into one 16-byte store, the int32 bias, the
bypass's exchange and sign extension, the two-segment stores.  A failure says how many values differ, where, and which wrong store (truncate, half away, half up,
a clamp at -128, a NaN code instead of saturation), if any, reproduces the output.  tests/test_conv_q8_exact_cases_host.py shows on the CPU that the cases can
tell these apart.

Every run: in_coff = out_coff = 16 inside wider pixels, the output's guard channels prefilled (0x5A bytes / -768) and required untouched, the input's guard channels
filled with a valid non-zero code; the automatic tile and every g tile whose cout tile divides Cout, with the grid uncapped and capped to 2 workgroups per XCD.

The e4m3-input cases rest on v_mfma_f32_32x32x64_f8f6f4 accumulating integer-valued products (multiples of 64, absolute sums below 2^21) exactly, as the bf16 MFMA is
shown to by tests/test_gpu_conv_exact.py.  It does: on the MI355X every e4m3-input case below, K = 4608 included, equals its float64 reference bit for bit under
every g tile, so these cases carry no tolerance either."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as cx
import conv_q8_exact_cases as q8

pytestmark = pytest.mark.gpu

COFF = 16  # in_coff = out_coff, and the width of every guard band
GUARD_CODE = 7.0  # the input's guard channels: a value that is its own code in int8, e4m3 and bf16
SENTINEL = {"i8": 0x5A, "f8": 0x5A, "bf16": -768.0}
# tiles per Cout: the automatic one + every g tile (64, 96, 128 couts) that divides it -- counted from the tile table as it stands; each runs uncapped and capped
TILES = {64: 2, 96: 2, 256: 3, 128: 3, 192: 3}
BYPASS_TILES = {64: 2, 96: 2, 128: 2, 192: 3}  # (no 128-cout bypass tile)


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _g_tiles(lib, Cout, bypass=False):
    """[(cfg index, name, cout tile)]: the automatic tile first, then every g tile whose cout tile divides Cout (the bypass has no 128-cout variant)"""
    names = [lib.vgh_conv_cfg_name(i).decode() for i in range(lib.vgh_conv_num_cfgs())]
    t = [(i, n, lib.vgh_conv_cfg_cout_tile(i)) for i, n in enumerate(names) if n[0] == "g"]
    return [(-1, "auto", 0)] + [(i, n, bc) for i, n, bc in t if Cout % bc == 0 and not (bypass and bc == 128)]


_PACKS = {}


def _weights(lib, c):
    """the device weight image of a case, packed once per (shape, input format) by the library's own packer; the scales the cases count on are checked again"""
    from head_detector_amd import _lib
    from test_gpu_fp8 import _pack_fp8
    from test_gpu_int8 import _pack_i8

    src = c["link"].split("_")[0]
    key = (c["shape"], src, id(c["W"]))
    if key not in _PACKS:
        W = c["W"]
        if src == "i8":
            pack, ws = _pack_i8(lib, W)
            assert bool((ws == 1.0).all())
            d = torch.from_numpy(pack).to(_dev())
        elif src == "f8":
            pack, ws = _pack_fp8(lib, W)
            assert bool((ws == q8.F8_WSCALE).all())
            d = torch.from_numpy(pack).to(_dev())
        else:
            pk = np.zeros(W.numel(), dtype=np.uint16)
            _lib.check(lib.vgh_pack_conv_weights(_lib.ptr(np.ascontiguousarray(W.numpy())), W.shape[0], 3, W.shape[3], _lib.ptr(pk)))
            d = torch.from_numpy(pk.view(np.int16)).to(_dev())
        _PACKS[key] = d
    return _PACKS[key]


def _to_codes(x, fmt, lead=COFF, tail=COFF, fill=GUARD_CODE):
    """[B,H,W,C] float32 values -> the device tensor of that format with `lead` / `tail` guard channels around the C live ones"""
    B, H, W, Cn = x.shape
    t = torch.full((B, H, W, lead + Cn + tail), fill, dtype=torch.float32)
    t[..., lead : lead + Cn] = x
    if fmt == "i8":
        assert float(t.abs().max()) <= 127 and torch.equal(t, t.round())
        return t.to(torch.int8).to(_dev())
    if fmt == "f8":
        assert torch.equal(t.to(q8.E4M3).float(), t)
        return t.to(q8.E4M3).view(torch.uint8).to(_dev())
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    return t.to(torch.bfloat16).to(_dev())


def _new_out(B, H, W, pitch, out):
    if out == "bf16":
        return torch.full((B, H, W, pitch), SENTINEL[out], dtype=torch.bfloat16, device=_dev())
    return torch.full((B, H, W, pitch), SENTINEL[out], dtype=torch.uint8, device=_dev())


def _fetch(d_out, out):
    """the whole output buffer on the host: int16 codes (int8), uint8 bytes (e4m3) or float32 (bf16)"""
    if out == "i8":
        return d_out.cpu().view(torch.int8).to(torch.int16)
    return d_out.cpu() if out == "f8" else d_out.float().cpu()


def _launch(lib, c, d_in, d_out, *, act, cfg, cap, out_coff=COFF, split=None, res=None, diag=False, in_pitch=None, in_coff=COFF):
    """one vgh_conv2d of the case's weights, bias and factors on the given device buffers.  split = (out_split, out_coff2); res = (device bf16 tensor, pitch, coff)"""
    from head_detector_amd import _lib

    B, H, W, Cin, Cout, _, _ = c["shape"]
    src, out = c["link"].split("_")
    d_w = _weights(lib, c)
    d_bias, d_g = q8.kernel_bias(c).to(_dev()), q8.kernel_gscale(c).to(_dev())
    d_diag = q8.kernel_diag(c).to(_dev()) if diag else None
    call = _lib.ConvCall(in_dev=d_in.data_ptr(), in_pitch=in_pitch or d_in.shape[-1], in_coff=in_coff, cin=Cin, B=B, H=H, W=W, wpack_dev=d_w.data_ptr(), bias_dev=d_bias.data_ptr(),
                         out_dev=d_out.data_ptr(), out_pitch=d_out.shape[-1], out_coff=out_coff, cout_pad=Cout, cout_store=Cout, out_split=split[0] if split else Cout,
                         out_coff2=split[1] if split else 0, out_f32=0, res_dev=res[0].data_ptr() if res else None, res_pitch=res[1] if res else 0, res_coff=res[2] if res else 0,
                         alpha=c["alpha"] if res else 0.0, ksize=3, stride=1, act=act, shuffle=0, force_cfg=cfg,
                         fmt={"i8": _lib.VGH_FMT_I8, "f8": _lib.VGH_FMT_FP8, "bf16": _lib.VGH_FMT_BF16}[src], out_fp8={"bf16": 0, "f8": 1, "i8": 2}[out], gscale_dev=d_g.data_ptr(),
                         diag_dev=d_diag.data_ptr() if diag else None)
    try:
        assert lib.vgh_conv_set_max_blocks_per_xcd(cap) == 0
        _lib.check(lib.vgh_conv2d(C.byref(call), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        lib.vgh_conv_set_max_blocks_per_xcd(0)


def _run(lib, c, *, act, cfg, cap, with_res=False, diag=False, x=None):
    """the case (or `x` in place of its input) through one launch with the standard geometry; returns the whole output buffer on the host"""
    B, H, W, Cin, Cout, _, _ = c["shape"]
    src, out = c["link"].split("_")
    d_in = _to_codes(c["x"] if x is None else x, src)
    d_out = _new_out(B, H, W, Cout + 2 * COFF, out)
    d_res = c["res"].to(torch.bfloat16).to(_dev()).contiguous() if with_res else None
    _launch(lib, c, d_in, d_out, act=act, cfg=cfg, cap=cap, res=(d_res, Cout, 0) if with_res else None, diag=diag)
    return _fetch(d_out, out)


def _stored(v, out, act, how="rne"):
    """what a store `how` leaves of the float64 value v, in _fetch's representation"""
    if out == "bf16":
        v32 = q8.exact_f32(v)
        return cx.rne(v32, cx.BF16) if how == "rne" else cx.WRONG_ROUNDINGS[how](v32, cx.BF16)
    return q8.STORE[out](v, act, how)


def _eq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _ne(a, b):
    return a.view(torch.int32) != b.view(torch.int32) if a.dtype == torch.float32 else a != b


def _check(got, parts, out, act, where):
    """got: the whole output buffer [B,H,W,pitch] (_fetch); parts: [(channel offset, float64 value [B,H,W,n])]: those channels hold the correct store of the value,
    byte for byte (bf16: bit for bit), every other channel still holds the sentinel."""
    def build(how):
        t = torch.full_like(got, SENTINEL[out])
        for off, v in parts:
            t[..., off : off + v.shape[-1]] = _stored(v, out, act, how).to(t.dtype)
        return t

    want = build("rne")
    if _eq(got, want):
        return
    live = torch.zeros(got.shape[-1], dtype=torch.bool)
    for off, v in parts:
        live[off : off + v.shape[-1]] = True
    bad = _ne(got, want)
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    msg = [f"{where}: {int(bad.sum())} of {int(live.sum()) * bad[..., 0].numel()} stored values differ, {int(bad[..., ~live].sum())} outside the stored channels; "
           f"first {idx[:5].tolist()} (b, y, x, channel of the buffer); at {first} got {got[first].item()!r} want {want[first].item()!r}"]
    wrong = q8.WRONG_STORES[out] if out != "bf16" else tuple(cx.WRONG_ROUNDINGS)
    hit = [how for how in wrong if _eq(got, build(how))]
    msg.append(f"reproduced exactly by: {', '.join(hit)}" if hit else f"reproduced by none of {' / '.join(wrong)}")
    pix = (idx[:, 1] * got.shape[2] + idx[:, 2]) % 32
    msg.append(f"pixel%32 hist {torch.bincount(pix, minlength=32).tolist()}; chan%32 hist {torch.bincount(idx[:, 3] % 32, minlength=32).tolist()}; "
               f"image hist {torch.bincount(idx[:, 0], minlength=got.shape[0]).tolist()}")
    raise AssertionError("\n".join(msg))


def _range_asserts(got, out, act, Cout, where, off=COFF):
    """8-bit outputs: the top clamp was hit, nothing below the format's most negative code (int8: -128 never written; e4m3: neither NaN code)"""
    live = got[..., off : off + Cout]
    if out == "i8":
        assert int(live.max()) == 127 and int(live.min()) == (0 if act else -127), (where, int(live.min()), int(live.max()))
    elif out == "f8":
        assert not bool(((live & 0x7F) == 0x7F).any()), f"{where}: a NaN code (0x7F / 0xFF) was stored"
        assert bool((live == 0x7E).any()) and (act == 1 or bool((live == 0xFE).any())), f"{where}: the clamp was not reached"
        assert act == 0 or int(live.max()) <= 0x7E, f"{where}: a negative value under the ReLU"


def _sweep(lib, c, variants, where, bypass=False):
    """every tile x both caps x every (act, with_res, diag) variant of one case, each compared with its own float64 reference; returns (runs, cout tiles forced)"""
    Cout = c["shape"][4]
    out = c["link"].split("_")[1]
    runs, widths = 0, set()
    for act, with_res, diag in variants:
        v = q8.value(c, act, with_res, diag)
        for cfg, name, bc in _g_tiles(lib, Cout, bypass):
            for cap in (0, 2):
                w = f"{where} act={act} res={with_res} diag={diag} tile {name} cap={cap}"
                got = _run(lib, c, act=act, cfg=cfg, cap=cap, with_res=with_res, diag=diag)
                _check(got, [(COFF, v)], out, act, w)
                _range_asserts(got, out, act, Cout, w)
                runs += 1
                widths.add(bc)
    return runs, widths


# ======================================================================================================
# 1 / 2: int8 -> bf16, plain, ReLU, ReLU + residual; the diagonal bypass
# ======================================================================================================
@pytest.mark.parametrize("shape", q8.SHAPES, ids=_ids)
def test_int8_to_bf16_stores_the_nearest_even_rounding_of_the_exact_value(gpu_lib, shape):
    """float(int32 sum that started at the int32 bias) * g[c], ReLU, + 0.5 * (integer bf16 residual) in fp32 (the RES branch and its exchange), one rounding to bf16."""
    c = q8.q8_link(shape, "i8_bf16")
    # the bias is read as an int32 bit pattern: as floats these patterns are denormals (positive biases) or NaNs (negative ones), so a tile that read them as fp32
    # would store the values of a zero bias, or NaN -- and three quarters of the channels have a bias that moves the stored value
    kb = q8.kernel_bias(c)
    assert bool(((kb.abs() < 1e-38) | torch.isnan(kb)).all()) and float((c["bias"] != 0).float().mean()) >= 0.75 and bool(torch.isnan(kb).any())
    no_bias = dict(c, bias=torch.zeros_like(c["bias"]))
    assert float((_stored(q8.value(no_bias), "bf16", 0) != _stored(q8.value(c), "bf16", 0)).float().mean()) > 0.5
    runs, widths = _sweep(gpu_lib, c, [(0, False, False), (1, False, False), (1, True, False)], f"{shape} int8 -> bf16")
    assert runs >= 3 * 2 * TILES[shape[4]], runs
    assert widths >= {bc for bc in (64, 96, 128) if shape[4] % bc == 0}, widths


BYPASS_SHAPES = [s for s in q8.SHAPES if s[3] >= s[4]]


@pytest.mark.parametrize("shape", BYPASS_SHAPES, ids=_ids)
def test_int8_to_bf16_with_the_diagonal_bypass_is_exact(gpu_lib, shape):
    """+ dvec[c] * code(input pixel, channel c) before the activation, on the 64- and 96-cout tiles that carry the bypass: load_diag's 16-byte loads, its two
    half-wave exchanges and the sign extension of the codes -- the +-127 codes lie on the diagonal channels of every shape here."""
    c = q8.q8_link(shape, "i8_bf16")
    dx = c["x"][..., : shape[4]]
    assert bool((dx == 127).any()) and bool((dx == -127).any())
    assert len(BYPASS_SHAPES) >= 3 and {s[4] for s in BYPASS_SHAPES} >= {64, 96, 192}
    runs, widths = _sweep(gpu_lib, c, [(0, False, True), (1, True, True)], f"{shape} int8 -> bf16 bypass", bypass=True)
    assert runs >= 2 * 2 * BYPASS_TILES[shape[4]], runs
    assert 128 not in widths and widths >= {bc for bc in (64, 96) if shape[4] % bc == 0}, widths


# ======================================================================================================
# 3: int8 outputs
# ======================================================================================================
@pytest.mark.parametrize("shape,link", [(s, "i8_i8") for s in q8.SHAPES] + [(q8.BF16_IN_SHAPE, "bf16_i8")], ids=_ids)
def test_int8_outputs_are_clamped_then_rounded_to_even(gpu_lib, shape, link):
    """pack_i8x4: clamp to [lo, 127] (lo = 0 under ReLU, else -127), rintf, four bytes per dword; two half-wave exchanges, one 16-byte store of 16 consecutive couts."""
    c = q8.q8_link(shape, link)
    runs, widths = _sweep(gpu_lib, c, [(0, False, False), (1, False, False)], f"{shape} {link}")
    assert runs >= 2 * 2 * TILES[shape[4]], runs
    assert widths >= {bc for bc in (64, 96, 128) if shape[4] % bc == 0}, widths


# ======================================================================================================
# 4: e4m3 inputs and outputs
# ======================================================================================================
@pytest.mark.parametrize("shape", q8.SHAPES, ids=_ids)
def test_e4m3_to_bf16_stores_the_nearest_even_rounding_of_the_exact_value(gpu_lib, shape):
    """one v_mfma_f32_32x32x64_f8f6f4 per pair on codes that hold x and 64 * w, the fp32 accumulator starting at 64 * bias: every partial sum is a multiple of 64 below
    2^21, exact in fp32 in any order -- IF the instruction adds such products exactly, which is what the equality below also establishes."""
    c = q8.q8_link(shape, "f8_bf16")
    runs, widths = _sweep(gpu_lib, c, [(0, False, False), (1, False, False), (1, True, False)], f"{shape} e4m3 -> bf16")
    assert runs >= 3 * 2 * TILES[shape[4]], runs
    assert widths >= {bc for bc in (64, 96, 128) if shape[4] % bc == 0}, widths


@pytest.mark.parametrize("shape,link", [(s, "f8_f8") for s in q8.SHAPES] + [(q8.BF16_IN_SHAPE, "bf16_f8")], ids=_ids)
def test_e4m3_outputs_saturate_at_448_and_round_to_even(gpu_lib, shape, link):
    """pack_fp8x4: clamp to [lo, 448], cvt_pk_fp8_f32 -- bytes equal to torch.float8_e4m3fn's of the clamped value; 0x7F and 0xFF never appear.  The bf16 -> e4m3 case
    holds the store to the bit on an accumulator that tests/test_gpu_conv_exact.py already shows exact."""
    c = q8.q8_link(shape, link)
    runs, widths = _sweep(gpu_lib, c, [(0, False, False), (1, False, False)], f"{shape} {link}")
    assert runs >= 2 * 2 * TILES[shape[4]], runs
    assert widths >= {bc for bc in (64, 96, 128) if shape[4] % bc == 0}, widths


# ======================================================================================================
# 5: two output segments
# ======================================================================================================
@pytest.mark.parametrize("link", ["i8_i8", "f8_f8"])
def test_8bit_outputs_in_two_segments(gpu_lib, link):
    """(2, 9, 19, 128, 256): couts 0 .. 127 at channel 160 of the output pixel, couts 128 .. 255 at channel 16 -- the second segment BELOW the first, whole cout tiles
    per segment (out_split a multiple of the tile), so the second tile's 16-byte stores carry the negative segment shift."""
    shape = (2, 9, 19, 128, 256)
    assert shape in q8.SHAPES
    c = q8.q8_link(shape, link)
    B, H, W, Cin, Cout = shape
    out = link.split("_")[1]
    half = Cout // 2
    first, second, pitch = 2 * COFF + half, COFF, 3 * COFF + Cout  # guards: [0, 16), [144, 160), [288, 304)
    runs, widths = 0, set()
    for act in (0, 1):
        v = q8.value(c, act)
        for cfg, name, bc in _g_tiles(gpu_lib, Cout):
            assert half % max(bc, 1) == 0
            for cap in (0, 2):
                d_in, d_out = _to_codes(c["x"], link.split("_")[0]), _new_out(B, H, W, pitch, out)
                _launch(gpu_lib, c, d_in, d_out, act=act, cfg=cfg, cap=cap, out_coff=first, split=(half, second))
                got = _fetch(d_out, out)
                w = f"{shape} {link} two segments act={act} tile {name} cap={cap}"
                _check(got, [(first, v[..., :half]), (second, v[..., half:])], out, act, w)
                _range_asserts(got, out, act, half, w, off=first)
                runs += 1
                widths.add(bc)
    assert runs >= 2 * 2 * 3 and widths >= {64, 128}, (runs, widths)


@pytest.mark.parametrize("link", ["i8_bf16", "f8_bf16"])
def test_8bit_inputs_with_a_segment_boundary_inside_the_cout_tile(gpu_lib, link):
    """The non-`simple` store path of the 8-bit-input variants: 64 couts, out_split = 40 -- the boundary falls inside every tile, so each 16-byte vector picks its own
    segment.  Couts 0 .. 39 at channel 56, couts 40 .. 63 at channel 16."""
    shape = q8.SHAPES[0]
    c = q8.q8_link(shape, link)
    B, H, W, Cin, Cout = shape
    cut = 40
    first, second, pitch = 2 * COFF + (Cout - cut), COFF, 3 * COFF + Cout
    runs = 0
    for act, with_res in ((0, False), (1, True)):
        v = q8.value(c, act, with_res)
        for cfg, name, bc in _g_tiles(gpu_lib, Cout):
            for cap in (0, 2):
                d_in, d_out = _to_codes(c["x"], link.split("_")[0]), _new_out(B, H, W, pitch, "bf16")
                d_res = c["res"].to(torch.bfloat16).to(_dev()).contiguous() if with_res else None
                _launch(gpu_lib, c, d_in, d_out, act=act, cfg=cfg, cap=cap, out_coff=first, split=(cut, second), res=(d_res, Cout, 0) if with_res else None)
                _check(_fetch(d_out, "bf16"), [(first, v[..., :cut]), (second, v[..., cut:])], "bf16", act, f"{shape} {link} split inside the tile act={act} res={with_res} tile {name} cap={cap}")
                runs += 1
    assert runs >= 2 * 2 * TILES[Cout], runs


# ======================================================================================================
# 6: bf16 -> 8 bit -> bf16
# ======================================================================================================
@pytest.mark.parametrize("fmt", ["i8", "f8"])
def test_two_op_chain_through_an_8bit_link_equals_the_composed_reference(gpu_lib, fmt):
    """Op 1 (bf16 -> 8 bit, ReLU) writes the link; op 2 (8 bit -> bf16, ReLU, + 0.5 * residual) reads the very bytes op 1 wrote, inside the link's wider pixels, and takes
    its residual from op 1's INPUT buffer (a view at channel 16 of that buffer).  Expected: the float64 reference of op 2 evaluated on the exactly rounded codes of the
    float64 reference of op 1 -- nothing else enters."""
    shape = q8.BF16_IN_SHAPE
    B, H, W, Cin, Cout = shape
    assert Cin == Cout
    c1, c2 = q8.q8_link(shape, f"bf16_{fmt}"), q8.q8_link(shape, f"{fmt}_bf16")
    codes = q8.STORE[fmt](q8.value(c1, 1), 1)
    z = codes.float() if fmt == "i8" else codes.view(q8.E4M3).float()  # the link's values, in op 2's input units
    assert float(z.max()) == (127.0 if fmt == "i8" else 448.0) and float(z.min()) == 0.0
    v2 = q8.value(c2, 1, True, x=z, res=c1["x"])
    q8.exact_f32(v2)
    assert q8.abs_sum_bound(dict(c2, x=z)) * (64.0 if fmt == "f8" else 1.0) < 2 ** 30  # int32 / multiples of 64 in fp32
    runs = 0
    for cfg, name, bc in _g_tiles(gpu_lib, Cout):
        for cap in (0, 2):
            d_x = _to_codes(c1["x"], "bf16")
            d_link = _new_out(B, H, W, Cout + 2 * COFF, fmt)
            d_out = _new_out(B, H, W, Cout + 2 * COFF, "bf16")
            _launch(gpu_lib, c1, d_x, d_link, act=1, cfg=cfg, cap=cap)
            _launch(gpu_lib, c2, d_link, d_out, act=1, cfg=cfg, cap=cap, res=(d_x, d_x.shape[-1], COFF))
            w = f"{shape} chain bf16 -> {fmt} -> bf16 tile {name} cap={cap}"
            _check(_fetch(d_link, fmt), [(COFF, q8.value(c1, 1))], fmt, 1, w + " (link)")
            _check(_fetch(d_out, "bf16"), [(COFF, v2)], "bf16", 1, w)
            runs += 1
    assert runs >= 2 * TILES[Cout], runs


# ======================================================================================================
# 7: images and pixels are independent
# ======================================================================================================
@pytest.mark.parametrize("shape,link", [(q8.SHAPES[0], "i8_i8"), (q8.SHAPES[0], "f8_f8"), (q8.SHAPES[4], "i8_bf16"), (q8.SHAPES[4], "f8_bf16")], ids=_ids)
def test_a_saturated_pixel_changes_only_its_own_receptive_fields(gpu_lib, shape, link):
    """The format's largest codes (+-127 / +-448, signs alternating by channel) over one whole pixel of image 0.  Against a clean run only the outputs whose 3x3
    receptive field holds that pixel may differ, guard channels included; and the run with the planted pixel equals its own float64 reference."""
    B, H, W, Cin, Cout = shape
    src, out = link.split("_")
    c = q8.q8_link(shape, link)
    big = 127.0 if src == "i8" else 448.0
    py, px = H // 2, W - 2
    x_bad = c["x"].clone()
    x_bad[0, py, px, :] = torch.where(torch.arange(Cin) % 2 == 0, big, -big)
    hit = torch.zeros(1, 1, H, W)
    hit[0, 0, py, px] = 1.0
    field = F.conv2d(hit, torch.ones(1, 1, 3, 3), padding=1)[0, 0] > 0
    assert int(field.sum()) == 9
    with_res = out == "bf16"
    v_bad = q8.value(c, 1, with_res, x=x_bad)
    q8.exact_f32(v_bad)
    runs = 0
    for cfg, name, bc in _g_tiles(gpu_lib, Cout):
        for cap in (0, 2):
            w = f"{shape} {link} planted pixel, tile {name} cap={cap}"
            clean = _run(gpu_lib, c, act=1, cfg=cfg, cap=cap, with_res=with_res)
            dirty = _run(gpu_lib, c, act=1, cfg=cfg, cap=cap, with_res=with_res, x=x_bad)
            _check(dirty, [(COFF, v_bad)], out, 1, w)
            keep = torch.ones(clean.shape, dtype=torch.bool)
            keep[0, :, :, COFF : COFF + Cout] = ~field[..., None]
            bad = _ne(clean, dirty) & keep
            assert not bool(bad.any()), f"{w}: {int(bad.sum())} outputs outside every receptive field changed, {int(bad[1:].sum())} of them in another image; first {bad.nonzero()[:5].tolist()}"
            assert bool(_ne(clean, dirty)[0].any())  # (the planted codes did arrive)
            runs += 1
    assert runs >= 2 * TILES[Cout], runs
