"""Head textures, the host side (no GPU): the CPU restatement of tests/texture_ref.py against the outputs recorded from the reference's own C++
(tests/golden/texture.npz, tests/golden/make_golden_texture.py) and against the live library where oracle/_ref provides it; what the fixture exercises; the
ABI of libvghtex.so and its argument checks; ``cylindrical_uv``; the errors of the public interface, raised before a GPU is looked for."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shade_ref as sr  # noqa: E402
import texture_ref as tr  # noqa: E402

from head_detector_amd import _lib, _lib_tex, _lib_view, _lib_vis, texture  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return np.load(tr.GOLDEN)


def _sources():
    return [False] + ([True] if tr.live() is not None else [])  # the restatement always; the reference's own C++ where it can be had


def _golden_cases(g):
    out = {}
    for name, kw in tr.cases().items():
        out[name] = tr.golden_case(g, name, kw.get("image"), out.get(tr.BASES.get(name)))
    return out


# ---- tests/texture_ref.py ---------------------------------------------------------------------------------------------------------------------
def test_wrap_cases_equal_the_recorded_reference(g):
    want = _golden_cases(g)
    for name, kw in tr.cases().items():
        before = np.array(kw["heads_vertices"], copy=True)
        for use_live in _sources():
            tr.same(tr.compose(use_live=use_live, **kw), want[name], (name, use_live))
        assert np.array_equal(kw["heads_vertices"], before)
        bg = want[name]["triangle"] < 0
        assert np.array_equal(bg, want[name]["head"] < 0) and (want[name]["depth"][bg] == np.float32(-1e8)).all()
        assert np.array_equal(want[name]["image"][bg], (np.zeros_like(want[name]["image"]) if kw.get("image") is None else kw["image"])[bg])  # unpainted pixels keep their value


def test_unwrap_roundtrip_and_result_cases_equal_the_recorded_reference(g):
    for name, kw in tr.unwrap_cases().items():
        want = tr.golden_case(g, name)
        for use_live in _sources():
            tr.same(tr.unwrap(use_live=use_live, **kw), want, (name, use_live))
        assert want["image"].shape == (len(kw["heads_vertices"]), kw["th"], kw["tw"], kw["image"].shape[2]) and np.isfinite(want["image"]).all()
    back = tr.golden_case(g, "roundtrip")
    for use_live in _sources():
        tr.same(tr.roundtrip(use_live), back, ("roundtrip", use_live))
    image, heads, faces, uv, (th, tw) = tr.result_scene()
    unwrapped = tr.golden_case(g, "unwrap_A")
    for occ in ("order", "depth"):
        mask = np.unpackbits(g[f"result.mask_{occ}"])[: len(heads) * th * tw].astype(bool).reshape(len(heads), th, tw)
        for use_live in _sources():
            got = tr.get_textures(image, heads, faces, uv, th, tw, "bilinear", True, occ, use_live)
            assert np.array_equal(got["texture"], unwrapped["image"]) and np.array_equal(got["triangle"], unwrapped["triangle"]) and np.array_equal(got["mask"], mask)
            assert np.array_equal(got["written"], unwrapped["triangle"] >= 0)
            assert np.array_equal(tr.paint(image, heads, faces, got["texture"], uv, "bilinear", occ, use_live), g[f"result.painted_{occ}"])
        assert (mask <= (unwrapped["triangle"] >= 0)).all() and 0 < mask.sum() < (unwrapped["triangle"] >= 0).sum()


def test_the_fixture_is_not_trivial(g):
    want, cases = _golden_cases(g), tr.cases()
    # the frame rule paints pixels on every border that the plain inside rule leaves alone, and nowhere else
    a = cases["A_order"]
    H, W = a["H"], a["W"]
    only = (want["A_order"]["triangle"] >= 0) & (tr.compose(frame=False, **a)["triangle"] < 0)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    borders = [xx < 2, xx > W - 3, yy < 2, yy > H - 3]
    assert all(int((only & b).sum()) > 0 for b in borders) and not (only & ~(borders[0] | borders[1] | borders[2] | borders[3])).any()
    # clamped positions, exact halves, integer positions, a zero-determinant triangle
    stats = {name: {} for name in ("A_order", "B_order", "quad_half", "quad_integer", "corner")}
    for name in stats:
        tr.same(tr.compose(stats=stats[name], **cases[name]), want[name], name)
    assert stats["A_order"]["clamped"] > 100 and stats["B_order"]["clamped"] > 10 and stats["quad_half"]["half"] > 20 and stats["quad_integer"]["integer"] == 72
    assert stats["corner"]["zero_det"] > 0 and int((want["corner"]["triangle"] == 5).sum()) == 49 and cases["corner"]["triangles"][5].tolist() == [4, 4, 1]
    # halves round away from zero: rounding them to even would read other texels
    ver, tri, coords = tr.quad_case(0.5)
    tex = cases["quad_half"]["textures"]
    x, y = 6, 7  # the position (1 + 1.5, 1 + 1.5) = (2.5, 2.5) -> texel (3, 3), not (2, 2)
    assert np.array_equal(want["quad_half"]["image"][y, x], tex[3, 3]) and not np.array_equal(tex[3, 3], tex[2, 2])
    # the two modes differ, and a texture topology of its own shows the source's indexing
    for s, least in (("A", 1000), ("B", 100)):
        o, d = want[f"{s}_order"], want[f"{s}_depth"]
        assert int(((o["head"] != d["head"]) | (o["triangle"] != d["triangle"])).sum()) > least
    b = cases["B_order"]
    assert not np.array_equal(b["tex_triangles"], b["triangles"])
    proper = tr.compose(quirk=False, **b)
    assert np.array_equal(proper["triangle"], want["B_order"]["triangle"]) and int((proper["image"] != want["B_order"]["image"]).sum()) > 500
    # the third column of the texture coordinates is never read
    junk = dict(a, tex_coords=a["tex_coords"].copy())
    junk["tex_coords"][:, 2] = np.nan
    tr.same(tr.compose(**junk), want["A_order"], "third column")
    # unwrap leaves texels unwritten; painting the atlas back returns the photograph almost unchanged
    assert 0 < int((tr.golden_case(g, "unwrap_A")["triangle"] >= 0).sum()) < tr.golden_case(g, "unwrap_A")["triangle"].size
    back, img = tr.golden_case(g, "roundtrip"), tr.roundtrip_scene()[0].astype(np.float32)
    cov = back["triangle"] >= 0
    inner = cov.copy()
    inner[1:] &= cov[:-1]
    inner[:-1] &= cov[1:]
    inner[:, 1:] &= cov[:, :-1]
    inner[:, :-1] &= cov[:, 1:]
    assert int(inner.sum()) > 3000 and np.abs(back["image"][inner] - img[inner]).mean() < 1.0


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def test_texture_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_tex.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghtex_[a-z0-9_]+)\s*\(", hdr))
    want = {"vghtex_version", "vghtex_last_error", "vghtex_render_texture"}
    assert declared == want and set(_lib_tex.SYMBOLS) == want and _exported(_lib_tex.LIB_PATH) == want  # exactly 3
    assert _lib_tex.load().vghtex_version().startswith(b"vghtex")
    fields = re.search(r"typedef struct vghtex_job \{(.*?)\} vghtex_job;", hdr, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    J = _lib_tex.Job
    assert names == [f[0] for f in J._fields_], names
    ints = ["height", "width", "channels", "n_heads", "n_vertices", "n_triangles", "n_tex_vertices", "tex_height", "tex_width", "tex_channels", "tex_dtype", "tex_per_head",
            "tex_coords_per_head", "dst_per_head", "mapping", "mode", "z_sign"]
    pointers = ["verts_dev", "triangles", "tex_coords_dev", "tex_triangles", "texture_dev", "bounds", "dst_dev", "depth_dev", "triangle_dev", "head_dev"]
    offsets = {f[0]: getattr(J, f[0]).offset for f in J._fields_}
    assert offsets == {**{k: 4 * i for i, k in enumerate(ints)}, **{k: 72 + 8 * i for i, k in enumerate(pointers)}}, offsets
    assert C.sizeof(J) == 152
    for name, value in (("VGHTEX_MAX_SIDE", _lib_tex.MAX_SIDE), ("VGHTEX_MAX_HEADS", _lib_tex.MAX_HEADS), ("VGHTEX_MAX_CHANNELS", _lib_tex.MAX_CHANNELS),
                        ("VGHTEX_MODE_ORDER", _lib_tex.MODES["order"]), ("VGHTEX_MODE_DEPTH", _lib_tex.MODES["depth"]), ("VGHTEX_MAP_NEAREST", _lib_tex.MAPPINGS["nearest"]),
                        ("VGHTEX_MAP_BILINEAR", _lib_tex.MAPPINGS["bilinear"]), ("VGHTEX_TEX_F32", _lib_tex.TEX_DTYPES["float32"]), ("VGHTEX_TEX_U8", _lib_tex.TEX_DTYPES["uint8"])):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    # the other three libraries are what they were, and none of them knows of this one
    core = {s for s in _exported(_lib.LIB_PATH) if s.startswith("vgh")}
    assert core == set(_lib.SYMBOLS) and len(core) == 86
    assert _exported(_lib_view.LIB_PATH) == set(_lib_view.SYMBOLS) and len(_lib_view.SYMBOLS) == 6
    assert _exported(_lib_vis.LIB_PATH) == set(_lib_vis.SYMBOLS) and len(_lib_vis.SYMBOLS) == 3
    for path in (_lib.LIB_PATH, _lib_view.LIB_PATH, _lib_vis.LIB_PATH):
        dyn = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        assert "vghtex_" not in dyn and b"libvghtex" not in open(path, "rb").read()
    own = subprocess.run(["nm", "-D", "--undefined-only", _lib_tex.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bvgh(v|vis)?_", own)  # it links no object of the other three


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib_tex.load()
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    bounds = np.array([[0, 0, 7, 7]], np.int32)

    def job(**kw):
        j = _lib_tex.Job()
        j.height, j.width, j.channels, j.n_heads, j.n_vertices, j.n_triangles, j.n_tex_vertices = 8, 8, 3, 1, 4, 2, 4
        j.tex_height, j.tex_width, j.tex_channels, j.tex_dtype, j.tex_per_head, j.tex_coords_per_head, j.dst_per_head, j.mapping, j.mode, j.z_sign = 5, 6, 3, 0, 0, 0, 0, 1, 0, 1.0
        j.verts_dev, j.triangles, j.tex_coords_dev, j.tex_triangles, j.texture_dev, j.bounds = 4096, tri.ctypes.data, 8192, tri.ctypes.data, 12288, bounds.ctypes.data
        j.dst_dev, j.depth_dev, j.triangle_dev, j.head_dev = 16384, 20480, 24576, 28672
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(what, **kw):
        assert lib.vghtex_render_texture(job(**kw), None) == -1, what  # VGHTEX_ERR_INVALID
        assert what.encode() in lib.vghtex_last_error(), lib.vghtex_last_error()

    def arr(rows):
        a = np.array(rows, np.int32)
        keep.append(a)
        return a.ctypes.data

    keep = []
    refused("height x width 0 x 8", height=0)
    refused("height x width 8 x 40000", width=40000)
    refused("channels 0", channels=0)
    refused("channels 17", channels=17, tex_channels=17)
    refused("n_heads", n_heads=-1)
    refused("n_heads", n_heads=65537)
    refused("n_vertices -1", n_vertices=-1)
    refused("n_triangles -1", n_triangles=-1)
    refused("n_tex_vertices -1", n_tex_vertices=-1)
    refused("n_vertices 0 with 2 triangles", n_vertices=0)
    refused("n_tex_vertices 0 with 2 triangles", n_tex_vertices=0)
    refused("tex_height x tex_width 0 x 6", tex_height=0)
    refused("tex_height x tex_width 5 x 32768", tex_width=32768)
    refused("tex_channels 2 below channels 3", tex_channels=2)
    refused("tex_dtype 2", tex_dtype=2)
    refused("tex_per_head 2", tex_per_head=2)
    refused("tex_coords_per_head -1", tex_coords_per_head=-1)
    refused("dst_per_head 3", dst_per_head=3)
    refused("mapping 2", mapping=2)
    refused("mapping -1", mapping=-1)
    refused("mode 2", mode=2)
    refused("z_sign", z_sign=0.5)
    refused("z_sign", z_sign=float("nan"))
    for p in ("dst_dev", "depth_dev", "verts_dev", "triangles", "tex_coords_dev", "tex_triangles", "texture_dev", "bounds"):
        refused(f"null {p}", **{p: None})
    refused("triangles: triangle 1: index 4 outside the 4 vertices", triangles=arr([[0, 1, 2], [1, 4, 2]]))
    refused("triangles: triangle 1: index -1 outside the 4 vertices", triangles=arr([[0, 1, 2], [1, -1, 2]]))
    refused("triangles: triangle 1: index 3 outside the 3 texture coordinates", n_tex_vertices=3, tex_triangles=arr([[0, 1, 2], [1, 0, 2]]))  # y is read through the mesh's index
    refused("tex_triangles: triangle 0: index 5 outside the 5 texture coordinates", n_tex_vertices=5, tex_triangles=arr([[0, 5, 2], [1, 3, 2]]))
    refused("tex_triangles: triangle 1: index -2 outside the 4 texture coordinates", tex_triangles=arr([[0, 1, 2], [1, -2, 2]]))
    for b in ([0, 0, 8, 7], [0, 0, 7, 8], [-1, 0, 7, 7], [0, -1, 7, 7]):
        refused("bounds: head 0: (%d, %d, %d, %d) outside the image" % tuple(b), bounds=arr([b]))
    refused("exceed one launch", n_heads=65536, n_triangles=1 << 20)
    refused("destination pixels exceed one launch", n_heads=65536, dst_per_head=1, height=32767, width=32767)
    for optional in ("triangle_dev", "head_dev"):  # an optional output left out changes no check
        refused("null depth_dev", depth_dev=None, **{optional: None})
        refused("index 4 outside the 4 vertices", triangles=arr([[0, 1, 2], [1, 4, 2]]), **{optional: None})
    assert lib.vghtex_render_texture(None, None) == -1 and b"null job" in lib.vghtex_last_error()


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_cylindrical_uv():
    unit, tri = sr.ellipsoid(11, 16)  # a closed sphere; FLAME's axes: y up, the face looks along +z
    ver = unit[:, [0, 2, 1]] * np.array([1.0, 1.3, 0.9]) + np.array([0.1, -0.2, 0.3])
    before = ver.copy()
    uv, keep = texture.cylindrical_uv(ver, tri)
    assert np.array_equal(ver, before) and uv.dtype == np.float32 and uv.shape == (ver.shape[0], 2) and keep.dtype == bool and keep.shape == (tri.shape[0],)
    assert uv.min() >= 0 and uv.max() <= 1
    top, bottom, front = ver[:, 1].argmax(), ver[:, 1].argmin(), (ver[:, 2] - 10 * np.abs(ver[:, 0] - 0.1) - 10 * np.abs(ver[:, 1] + 0.2)).argmax()
    assert uv[top, 1] == 0 and uv[bottom, 1] == 1 and abs(uv[front, 0] - 0.5) < 1e-6  # the top of the head at v = 0, the face in the middle of the atlas
    span = uv[:, 0][tri].max(axis=1) - uv[:, 0][tri].min(axis=1)
    ring = ~np.isin(tri, [top, bottom]).any(axis=1)  # a pole lies on the axis, where u means nothing
    assert np.array_equal(keep, span < 0.5) and 0 < int((~keep).sum()) < tri.shape[0] // 4 and span[keep & ring].max() < 0.2  # only the seam's triangles go
    right = ver[:, 0] > 0.1 + 0.5
    assert (uv[right, 0] > 0.5).all()  # +x to the right of the face
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        texture.cylindrical_uv(ver[:, :2], tri)
    with pytest.raises(ValueError, match="triangle index"):
        texture.cylindrical_uv(ver, np.array([[0, 1, ver.shape[0]]]))
    uv2, keep2 = texture.cylindrical_uv(ver, tri[:0])
    assert np.array_equal(uv2, uv) and keep2.shape == (0,)


def test_public_argument_errors_come_before_the_gpu():
    image, heads, faces, uv, (th, tw) = tr.result_scene()
    H, W = image.shape[:2]
    hs = [sr.make_head(h) for h in heads]
    res = PredictionResult(image, hs, faces=faces)
    tex = np.zeros((th, tw, 3), np.uint8)
    # the PredictionResult methods fail cleanly without faces, like render_mesh and get_visibility
    for r in (PredictionResult(image, hs), PredictionResult(image, [])):
        with pytest.raises(ValueError, match="no triangle list"):
            r.get_textures(uv)
        with pytest.raises(ValueError, match="no triangle list"):
            r.render_texture(tex, uv)
    for kw, msg in ((dict(mapping="cubic"), "mapping"), (dict(occlusion="painter"), "occlusion"), (dict(size=0), "size"), (dict(size=(8, 40000)), "size")):
        with pytest.raises(ValueError, match=msg):
            res.get_textures(uv, **kw)
    with pytest.raises(ValueError, match=r"uv must be \[169, 2\]"):
        res.get_textures(uv[:-1])
    with pytest.raises(ValueError, match="triangle index"):
        res.get_textures(uv, faces=np.array([[0, 1, heads.shape[1]]]))
    for kw, msg in ((dict(mapping="cubic"), "mapping"), (dict(occlusion="painter"), "occlusion")):
        with pytest.raises(ValueError, match=msg):
            res.render_texture(tex, uv, **kw)
    with pytest.raises(ValueError, match="at least 3 channels"):
        res.render_texture(tex[:, :, :2], uv)
    with pytest.raises(ValueError, match="holds 2 textures for 5 heads"):
        res.render_texture(np.zeros((2, th, tw, 3), np.float32), uv)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        PredictionResult(image[:, :, :1], hs, faces=faces).render_texture(tex, uv)
    # texture.render_texture / unwrap_heads
    coords = tr.atlas_vertices(uv, th, tw)
    ok = dict(vertices=heads, triangles=faces, texture=tex, tex_coords=coords, height=H, width=W)
    for kw, msg in ((dict(mapping="cubic"), "mapping"), (dict(occlusion="painter"), "occlusion"), (dict(z_sign=0.0), "z_sign"), (dict(height=0), "height x width"),
                    (dict(width=32768), "height x width"), (dict(vertices=heads[:, :, :2]), r"\[n, V, 3\]"), (dict(texture=tex[0]), "texture must be"),
                    (dict(texture=np.zeros((3, th, tw, 3))), "holds 3 textures for 5 heads"), (dict(tex_coords=coords[:, :2]), r"\[n, Vt, 3\]"),
                    (dict(tex_coords=np.stack([coords] * 2)), "holds 2 sets for 5 heads"), (dict(triangles=np.array([[0, 1, 169]])), "triangle index"),
                    (dict(tex_coords=coords[:100]), "triangle index"), (dict(tex_triangles=np.array([[0, 1, 169]])), "tex_triangles"),
                    (dict(tex_triangles=faces[:5]), "shape of triangles"), (dict(channels=4), "channels"), (dict(channels=0), "channels"),
                    (dict(image=np.zeros((H, W + 1, 3), np.float32)), "image must be"), (dict(image=np.zeros((H, W, 3), np.float32), channels=2), "channels = 2"),
                    (dict(image=np.zeros((H, W, 4), np.float32)), "channels")):
        with pytest.raises(ValueError, match=msg):
            texture.render_texture(**dict(ok, **kw))
    with pytest.raises(ValueError, match="GPU"):
        texture.render_texture(**dict(ok, vertices=torch.zeros(1, 169, 3)))
    for kw, msg in ((dict(image=image[0]), r"\[H, W, C\]"), (dict(uv=uv[:, :1]), "uv must be"), (dict(size=-1), "size"), (dict(mapping="x"), "mapping"),
                    (dict(triangles=np.array([[0, 1, -1]])), "triangle index"), (dict(vertices=heads[0, :, 0]), r"\[n, V, 3\]")):
        with pytest.raises(ValueError, match=msg):
            texture.unwrap_heads(**dict(dict(image=image, vertices=heads, triangles=faces, uv=uv, size=(th, tw)), **kw))
    if not torch.cuda.is_available():  # no CPU path: a missing GPU is an error, never another implementation
        with pytest.raises(_lib.VghError, match="GPU"):
            res.get_textures(uv, size=(th, tw))
        with pytest.raises(_lib.VghError, match="GPU"):
            res.render_texture(tex, uv)
        with pytest.raises(_lib.VghError, match="GPU"):
            texture.render_texture(**ok)
        with pytest.raises(_lib.VghError, match="GPU"):
            texture.unwrap_heads(image, heads, faces, uv, (th, tw))


def test_head_textures_class():
    t = texture.HeadTextures(np.zeros((2, 4, 5, 3), np.float32), np.full((2, 4, 5), -1, np.int32), np.zeros((2, 4, 5), bool))
    assert len(t) == 2 and t.mask is t.written and "size=(4, 5)" in repr(t) and "channels=3" in repr(t)
    m = np.ones((2, 4, 5), bool)
    assert texture.HeadTextures(t.texture, t.triangle, t.written, m).mask is m
