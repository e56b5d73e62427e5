"""Head textures on the MI355X: csrc/texture.hip (libvghtex.so) against the reference's own C++ -- its recorded outputs (tests/golden/texture.npz) and,
where oracle/_ref provides it, the live library (otherwise the CPU restatement tests/texture_ref.py, which tests/test_texture_host.py holds to the same
outputs).  Every comparison is np.array_equal / torch.equal: there is no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import texture_ref as tr  # noqa: E402

from head_detector_amd import texture  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _live():
    return tr.live() is not None


def _render(kw, **more):
    """``texture.render_texture`` with the keyword arguments of ``texture_ref.compose`` -> dict(image, depth, triangle, head)."""
    kw = dict(kw, **more)
    out = texture.render_texture(kw["heads_vertices"], kw["triangles"], kw["textures"], kw["tex_coords"], kw["H"], kw["W"], tex_triangles=kw.get("tex_triangles"),
                                 image=kw.get("image"), channels=kw["c"], mapping=kw["mapping"], occlusion=kw.get("occlusion", "order"), z_sign=kw.get("z_sign", 1.0),
                                 with_buffers=True)
    return dict(zip(tr.FIELDS, out))


def _check(kw, what, want=None):
    """The kernel against the reference composition (and ``want``, a recorded result): all four outputs, the inputs untouched."""
    before = {k: np.array(v, copy=True) for k, v in kw.items() if isinstance(v, np.ndarray)}
    got = _render(kw)
    for k, v in before.items():
        assert np.array_equal(kw[k], v, equal_nan=v.dtype.kind == "f"), (what, k, "modified")
    ref = tr.compose(use_live=_live(), **kw)
    if want is not None:
        tr.same(got, want, (what, "recorded"))
    tr.same(got, ref, what)
    assert np.array_equal(texture.render_texture(kw["heads_vertices"], kw["triangles"], kw["textures"], kw["tex_coords"], kw["H"], kw["W"], tex_triangles=kw.get("tex_triangles"),
                                                 image=kw.get("image"), channels=kw["c"], mapping=kw["mapping"], occlusion=kw.get("occlusion", "order"),
                                                 z_sign=kw.get("z_sign", 1.0)), got["image"]), (what, "the image alone")
    return got


@pytest.fixture(scope="module")
def g():
    return np.load(tr.GOLDEN)


def test_recorded_wrap_cases(gpu_lib, g):
    """Both image sizes, both atlases, 1, 5 and 12 heads, c = 1, 3, 4 with tex_c > c, u8 and f32 textures, shared and per-head textures and coordinates, both
    mappings, both modes, a texture topology of its own, a background, exact halves and integers, a zero-determinant triangle."""
    want = {}
    for name, kw in tr.cases().items():
        want[name] = tr.golden_case(g, name, kw.get("image"), want.get(tr.BASES.get(name)))
        _check(kw, name, want[name])
    assert int((want["corner"]["triangle"] == 5).sum()) == 49


def test_texture_formats_and_sharing(gpu_lib, g):
    cases = tr.cases()
    # a u8 texture gives what the same texels give as floats, shared or per head; float64 and int64 inputs are converted
    b = cases["B_order"]
    want = tr.golden_case(g, "B_order")
    n = len(b["heads_vertices"])
    as_float = dict(b, textures=b["textures"].astype(np.float32))
    per_head = dict(b, textures=np.stack([b["textures"]] * n))
    wide = dict(b, heads_vertices=b["heads_vertices"].astype(np.float64), tex_coords=b["tex_coords"].astype(np.float64), triangles=b["triangles"].astype(np.int64),
                tex_triangles=b["tex_triangles"].astype(np.int64), textures=b["textures"].astype(np.float64))
    for what, kw in (("as float", as_float), ("per head", per_head), ("wide dtypes", wide)):
        tr.same(_render(kw), want, what)
    # per-head u8 textures and shared coordinates, bilinear, every channel count of the texture
    a = cases["A_order"]
    tex = tr.random_texture(7, a["textures"].shape, np.uint8)
    for c in (1, 3, 4):
        for mode in ("order", "depth"):
            _check(dict(a, textures=tex, c=c, occlusion=mode, mapping="nearest" if c == 1 else "bilinear"), ("u8 per head", c, mode))
    # tex_triangles left out = the mesh's list
    tr.same(_render(dict(a, tex_triangles=a["triangles"])), tr.golden_case(g, "A_order"), "tex_triangles given")


def test_head_counts_small_meshes_and_stale_scratch(gpu_lib, g):
    _, tri, uv = tr.patch_mesh()
    (H, W), (th, tw) = tr.SHAPE_B, tr.ATLAS_B
    tex, coords = tr.random_texture(8, (th, tw, 3), np.float32), tr.wrap_coords(8, None, uv, th, tw)
    bg = tr.random_texture(9, (H, W, 3), np.float32)
    base = dict(triangles=tri, textures=tex, tex_coords=coords, H=H, W=W, c=3, mapping="bilinear", image=bg)
    for mode in ("order", "depth"):
        none = _check(dict(base, heads_vertices=tr.heads(31, 0, H, W), occlusion=mode), ("n = 0", mode))  # no heads: the background, untouched
        assert np.array_equal(none["image"], bg) and (none["triangle"] == -1).all() and (none["head"] == -1).all() and (none["depth"] == np.float32(-1e8)).all()
        empty = _check(dict(base, heads_vertices=tr.heads(31, 5, H, W), triangles=tri[:0], occlusion=mode), ("T = 0", mode))  # a 0-triangle mesh
        assert np.array_equal(empty["image"], bg) and (empty["triangle"] == -1).all()
        # a 2-triangle mesh, three copies that overlap: two shifted by whole pixels, the nearer one first
        ver, qtri, qc = tr.quad_case(0.5)
        three = np.stack([ver + np.float32([0, 0, 5]), ver + np.float32([2, 1, 0]), ver + np.float32([-2, 3, 2.5])])
        for mapping in ("nearest", "bilinear"):
            got = _check(dict(heads_vertices=three, triangles=qtri, textures=tr.random_texture(5, (9, 10, 3), np.float32), tex_coords=qc, H=16, W=16, c=2, mapping=mapping,
                              occlusion=mode), ("quads", mode, mapping))
            assert sorted(np.unique(got["head"]).tolist()) == [-1, 0, 1, 2]
        for n in (1, 5):
            _check(dict(base, heads_vertices=tr.heads(32, n, H, W), occlusion=mode, z_sign=-1.0), ("n", n, mode))
    # [V, 3] is one head; heads wholly outside the image paint nothing
    one = tr.heads(33, 1, H, W)
    tr.same(_render(dict(base, heads_vertices=one[0])), _render(dict(base, heads_vertices=one)), "[V, 3]")
    away = _render(dict(base, heads_vertices=tr.heads(32, 2, H, W) + np.float32([10000, 0, 0])))
    assert np.array_equal(away["image"], bg) and (away["head"] == -1).all()
    # consecutive calls of different sizes: no scratch of one is seen by the next
    cases = tr.cases()
    first = _render(cases["A_depth"])
    _render(cases["quad_half"])
    tr.same(_render(cases["A_depth"]), first, "repeatable")
    tr.same(first, tr.golden_case(g, "A_depth", None, tr.golden_case(g, "A_order")), "A_depth")


def test_unwrap_and_the_way_back(gpu_lib, g):
    for name, kw in tr.unwrap_cases().items():
        want = tr.golden_case(g, name)
        before = kw["image"].copy(), kw["heads_vertices"].copy()
        got = texture.unwrap_heads(kw["image"], kw["heads_vertices"], kw["triangles"], kw["uv"], (kw["th"], kw["tw"]), mapping=kw["mapping"])
        assert np.array_equal(kw["image"], before[0]) and np.array_equal(kw["heads_vertices"], before[1])
        assert isinstance(got, texture.HeadTextures) and got.texture.dtype == np.float32 and got.triangle.dtype == np.int32 and got.written.dtype == bool
        assert np.array_equal(got.texture, want["image"]) and np.array_equal(got.triangle, want["triangle"]) and np.array_equal(got.written, want["triangle"] >= 0)
        assert got.mask is got.written and 0 < got.written.sum() < got.written.size
        ref = tr.unwrap(use_live=_live(), **kw)
        assert np.array_equal(got.texture, ref["image"]) and np.array_equal(got.triangle, ref["triangle"])
        # a float photograph with the bytes' values gives the same atlas; one head alone is its slice
        if kw["image"].dtype == np.uint8:
            same = texture.unwrap_heads(kw["image"].astype(np.float64), kw["heads_vertices"], kw["triangles"], kw["uv"], (kw["th"], kw["tw"]), mapping=kw["mapping"])
            assert np.array_equal(same.texture, got.texture) and np.array_equal(same.triangle, got.triangle)
        solo = texture.unwrap_heads(kw["image"], kw["heads_vertices"][1], kw["triangles"], kw["uv"], (kw["th"], kw["tw"]), mapping=kw["mapping"])
        assert solo.texture.shape[0] == 1 and np.array_equal(solo.texture[0], got.texture[1]) and np.array_equal(solo.triangle[0], got.triangle[1])
    # a square atlas given by its side; no heads
    kw = tr.unwrap_cases()["unwrap_B"]
    assert kw["th"] == kw["tw"]
    side = texture.unwrap_heads(kw["image"], kw["heads_vertices"], kw["triangles"], kw["uv"], kw["th"], mapping=kw["mapping"])
    assert np.array_equal(side.texture, tr.golden_case(g, "unwrap_B")["image"])
    none = texture.unwrap_heads(kw["image"], kw["heads_vertices"][:0], kw["triangles"], kw["uv"], 16)
    assert none.texture.shape == (0, 16, 16, 1) and none.triangle.shape == (0, 16, 16) and none.written.shape == (0, 16, 16)
    # unwrap, then wrap, through the device = the same two steps through the reference
    img, ver, tri, uv, (th, tw) = tr.roundtrip_scene()
    dev_img, dev_ver = torch.from_numpy(img).to(_dev()), torch.from_numpy(ver).to(_dev())
    keep = dev_img.clone(), dev_ver.clone()
    tex = texture.unwrap_heads(dev_img, dev_ver, tri, uv, (th, tw), to_host=False)  # device tensors in, device tensors out, inputs untouched
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (tex.texture, tex.triangle, tex.written, tex.mask)) and tex.written.dtype == torch.bool
    back = texture.render_texture(dev_ver, tri, tex.texture[0], tr.atlas_vertices(uv, th, tw), img.shape[0], img.shape[1], to_host=False, with_buffers=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in back) and [t.dtype for t in back] == [torch.float32, torch.float32, torch.int32, torch.int32]
    assert torch.equal(dev_img, keep[0]) and torch.equal(dev_ver, keep[1])
    got = dict(zip(tr.FIELDS, (t.cpu().numpy() for t in back)))
    tr.same(got, tr.golden_case(g, "roundtrip"), "roundtrip, recorded")
    ref = tr.roundtrip(_live())
    tr.same(got, ref, "roundtrip")
    assert int(tex.written.sum()) == ref["texels"]
    # a device image as the background is copied, not painted
    bg = torch.full((img.shape[0], img.shape[1], 3), 7.0, device=_dev())
    over = texture.render_texture(dev_ver, tri, tex.texture, tr.atlas_vertices(uv, th, tw), img.shape[0], img.shape[1], image=bg, to_host=False)
    assert (bg == 7.0).all() and over.data_ptr() != bg.data_ptr()
    cov = got["triangle"] >= 0
    assert np.array_equal(over.cpu().numpy()[cov], got["image"][cov]) and (over.cpu().numpy()[~cov] == 7.0).all()


def test_prediction_result_textures(gpu_lib, g):
    image, heads, faces, uv, (th, tw) = tr.result_scene()
    n = len(heads)
    hs = [sr.make_head(h) for h in heads]
    res = PredictionResult(image, hs, faces=faces)
    unwrapped = tr.golden_case(g, "unwrap_A")
    for occ in ("order", "depth"):
        mask = np.unpackbits(g[f"result.mask_{occ}"])[: n * th * tw].astype(bool).reshape(n, th, tw)
        got = res.get_textures(uv, size=(th, tw), occlusion=occ)
        assert isinstance(got, texture.HeadTextures) and len(got) == n
        assert np.array_equal(got.texture, unwrapped["image"]) and np.array_equal(got.triangle, unwrapped["triangle"])
        assert np.array_equal(got.written, unwrapped["triangle"] >= 0) and np.array_equal(got.mask, mask)
        ref = tr.get_textures(image, heads, faces, uv, th, tw, "bilinear", True, occ, _live())
        for k in ("texture", "triangle", "written", "mask"):
            assert np.array_equal(getattr(got, k), ref[k]), (occ, k)
        painted = res.render_texture(got, uv, occlusion=occ)  # a HeadTextures, or its array
        assert painted.dtype == np.uint8 and painted.shape == image.shape and np.array_equal(painted, g[f"result.painted_{occ}"])
        assert np.array_equal(res.render_texture(got.texture, uv, occlusion=occ), painted)
        assert np.array_equal(painted, tr.paint(image, heads, faces, got.texture, uv, "bilinear", occ, _live()))
    every = res.get_textures(uv, size=(th, tw), visible_only=False, mapping="nearest")
    ref = tr.get_textures(image, heads, faces, uv, th, tw, "nearest", False)
    assert np.array_equal(every.mask, every.written) and np.array_equal(every.texture, ref["texture"]) and np.array_equal(every.written, ref["written"])
    for h, v in zip(hs, heads):
        assert np.array_equal(h.vertices_3d, v)  # unlike get_pncc, no z flip is left behind
    assert np.array_equal(res.original_image, tr.result_scene()[0])
    # one shared u8 texture for every head, values outside [0, 255] are clamped, an explicit triangle list
    shared = tr.random_texture(10, (th, tw, 3), np.uint8)
    assert np.array_equal(res.render_texture(shared, uv, mapping="nearest"), tr.paint(image, heads, faces, shared, uv, "nearest", "order", _live()))
    wild = tr.random_texture(11, (n, th, tw, 4), np.float32) * np.float32(2) - np.float32(130)  # -136 .. 390
    out = res.render_texture(wild, uv, faces=faces[::2])
    assert np.array_equal(out, tr.paint(image, heads, faces[::2], wild, uv, "bilinear", "order", _live()))
    raw = tr.compose(heads, faces[::2], wild, tr.atlas_vertices(uv, th, tw), image.shape[0], image.shape[1], 3, "bilinear", "order", -1.0, image=image.astype(np.float32),
                     use_live=_live())["image"]
    assert (raw < 0).any() and (raw > 255).any() and (out[raw < 0] == 0).all() and (out[raw > 255] == 255).all()  # the clamp had something to do
    # on the device
    dres = PredictionResult(torch.from_numpy(image).to(_dev()), hs, faces=faces)
    dev = dres.get_textures(uv, size=(th, tw), to_host=False)
    mask = np.unpackbits(g["result.mask_order"])[: n * th * tw].astype(bool).reshape(n, th, tw)
    assert dev.texture.is_cuda and dev.mask.dtype == torch.bool and torch.equal(dev.mask.cpu(), torch.from_numpy(mask)) and torch.equal(dev.texture.cpu(), torch.from_numpy(unwrapped["image"]))
    dp = dres.render_texture(dev, uv, to_host=False)
    assert dp.is_cuda and dp.dtype == torch.uint8 and torch.equal(dp.cpu(), torch.from_numpy(g["result.painted_order"])) and torch.equal(dres.original_image.cpu(), torch.from_numpy(image))
    # no heads: empty textures, a copy of the image
    none = PredictionResult(image, [], faces=faces)
    t0 = none.get_textures(uv, size=(th, tw))
    assert t0.texture.shape == (0, th, tw, 3) and t0.mask.shape == (0, th, tw)
    p0 = none.render_texture(shared, uv)
    assert np.array_equal(p0, image) and p0 is not image
