"""Planted cases for head anonymisation in YUV 4:2:0 planes and for the RGB packer (include/vgh_video.h), on small frames, and what the restatement
(tests/yuv_anonymize_ref.py) makes of each.  Two kinds, as in tests/anonymize_cases.py:

  api cases   heads with the public parameters; they run through ``video.anonymize_frame`` AND through the C call, whose rows are then built from the
              restatement's own arithmetic (``rows_of``), never from the product's plan
  raw cases   hand-made rows the public interface cannot produce (chroma boxes that are not derived from the luma boxes, cell sides and tap tables chosen
              freely); through the C call only

A frame lives in one decoder surface (tests/yuv_ref.py ``surface``): every byte that belongs to no sample -- between width and pitch, the rows of an aligned
luma height, the tail -- is a seeded random sentinel, so a surface compares whole."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_cases as ac  # noqa: E402
import anonymize_ref as ref  # noqa: E402
import visibility_ref as vr  # noqa: E402
import yuv_anonymize_ref as yref  # noqa: E402
import yuv_ref  # noqa: E402

from anonymize_cases import EDGE_BOXES, ODD_BOXES, OVERLAP_BOXES, OWNER_BOXES, head  # noqa: E402,F401

LAYOUTS = ("nv12", "nv21", "i420")


def api_case(shape, boxes, method, region, layout, *, pitched=True, content="random", margin=0.1, cells=8, strength=0.1, color=(0, 0, 0), owner=None, matrix="bt709",
             full_range=False, seed=0, faces=None, heads=None):
    return dict(kind="api", shape=shape, heads=[head(b) for b in boxes] if heads is None else heads, method=method, region=region, layout=layout, pitched=pitched, content=content,
                margin=margin, cells=cells, strength=strength, color=color, owner=owner, matrix=matrix, full_range=full_range, seed=seed, faces=faces)


def raw_case(shape, luma_boxes, chroma_boxes, method, region, layout, *, pitched=True, content="random", luma_cell=None, chroma_cell=None, luma_taps=None, chroma_taps=None,
             color_yuv=(0, 0, 0), owner=None, seed=0):
    """Boxes are geometry boxes (x0, y0, x1, y1) of their own plane here."""
    return dict(kind="raw", shape=shape, luma_boxes=[tuple(b) for b in luma_boxes], chroma_boxes=[tuple(b) for b in chroma_boxes], method=method, region=region, layout=layout,
                pitched=pitched, content=content, luma_cell=luma_cell, chroma_cell=chroma_cell, luma_taps=luma_taps, chroma_taps=chroma_taps, color_yuv=color_yuv, owner=owner,
                seed=seed)


def _small_owner(h, w):
    """A caller's map on a tiny frame: head 1 everywhere but one pixel of an out-of-range value."""
    o = np.full((h, w), 1, dtype=np.int32)
    o[0, 0] = 9
    return o


def cases():
    out = {}
    k = 0
    for method in ("fill", "pixelate", "blur"):
        for region in ("box", "ellipse"):
            lay = lambda j: LAYOUTS[(k + j) % 3]  # noqa: E731  every layout meets every method and region over the three families
            out[f"edges_{method}_{region}"] = api_case((97, 131), EDGE_BOXES, method, region, lay(0), color=(255, 0, 128), full_range=bool(k % 2))
            out[f"odd_{method}_{region}"] = api_case((97, 131), ODD_BOXES, method, region, lay(1), content="saturating" if region == "box" else "random", strength=0.02, color=(1, 2, 3),
                                                     pitched=bool(k % 2), matrix="bt601")
            out[f"overlap_{method}_{region}"] = api_case((96, 130), OVERLAP_BOXES, method, region, lay(2), pitched=not k % 2, margin=0.0, cells=5, strength=0.03, color=(40, 200, 90),
                                                         full_range=not k % 2, matrix="bt2020")
            k += 1
        # a caller's map with -1, values outside [-1, n) and pixels outside their owner's box
        out[f"owner_{method}"] = api_case((97, 131), OWNER_BOXES, method, "box", LAYOUTS[k % 3], margin=0.0, cells=6, strength=0.04, color=(0, 255, 0), owner=ac._planted_owner())
        # the smallest frames: one sample a plane, one chroma sample under four (and under two) luma pixels, one row
        out[f"tiny_1x1_{method}"] = api_case((1, 1), [(0, 0, 1, 1)], method, "box", LAYOUTS[k % 3], margin=0.0, color=(200, 10, 10), pitched=False)
        out[f"tiny_2x2_{method}"] = api_case((2, 2), [(0, 0, 2, 2), (1, 1, 1, 1)], method, "box", LAYOUTS[(k + 1) % 3], margin=0.0, color=(0, 0, 255), pitched=False, cells=1,
                                             strength=0.3)
        out[f"tiny_1x7_{method}"] = api_case((1, 7), [(2, 0, 3, 1), (6, 0, 5, 1)], method, "box", LAYOUTS[(k + 2) % 3], margin=0.0, color=(9, 9, 9), cells=2, strength=0.3,
                                             owner=_small_owner(1, 7) if method == "fill" else None)
    # pixelate: cell side 1 in both planes (the identity), ragged cells, 64 cells
    out["pixelate_identity"] = api_case((97, 131), [(20, 30, 8, 5)], "pixelate", "box", "nv12", margin=0.0, cells=8)
    out["pixelate_ragged"] = api_case((97, 131), [(13, 17, 50, 31)], "pixelate", "box", "i420", content="saturating", margin=0.0, cells=7)
    out["pixelate_64"] = api_case((96, 130), [(-5, 3, 140, 90)], "pixelate", "ellipse", "nv21", margin=0.0, cells=64)
    # blur: r = 0, a radius wider than a wave, a radius larger than the frame in both planes (every tap clamps somewhere)
    out["blur_r0"] = api_case((97, 131), [(20, 30, 40, 30)], "blur", "box", "nv21", margin=0.0, strength=0.0)
    out["blur_r70"] = api_case((97, 131), [(10, 2, 93, 80)], "blur", "ellipse", "nv12", content="saturating", margin=0.0, strength=0.25)
    out["blur_all_clamp"] = api_case((97, 131), [(-30, -10, 200, 110)], "blur", "box", "i420", margin=0.0, strength=0.25)
    out["no_heads"] = api_case((97, 131), [], "pixelate", "ellipse", "nv12")
    rng = np.random.default_rng(11)
    many = [(int(x), int(y), int(w), int(h)) for x, y, w, h in zip(rng.integers(-6, 60, 300), rng.integers(-6, 60, 300), rng.integers(1, 16, 300), rng.integers(1, 16, 300))]
    for j, method in enumerate(("fill", "pixelate", "blur")):
        out[f"many_heads_{method}"] = api_case((64, 64), many, method, "ellipse", LAYOUTS[j], cells=4, strength=0.1, color=(7, 7, 7), seed=3, pitched=bool(j % 2))
    # the mesh silhouettes of tests/anonymize_cases.py as the luma owner map
    mesh = ac._mesh_case("pixelate")
    out["mesh_pixelate"] = api_case((19, 23), [], "pixelate", "mesh", "nv12", cells=3, color=(9, 200, 31), seed=5, faces=mesh["faces"], heads=mesh["heads"])
    # raw: rows the plan never makes.  The chroma boxes are the caller's: smaller than what the head owns (the rest stays unchanged), or shifted
    out["raw_free_chroma_fill"] = raw_case((97, 131), [(10, 10, 60, 50), (50, 30, 120, 90)], [(8, 8, 20, 20), (30, 10, 70, 40)], "fill", "box", "nv12", color_yuv=(3, 250, 77))
    out["raw_free_chroma_cells"] = raw_case((97, 131), [(10, 10, 60, 50), (50, 30, 120, 90)], [(5, 5, 31, 24), (20, 16, 66, 49)], "pixelate", "map", "nv21", luma_cell=[7, 64],
                                            chroma_cell=[64, 3], owner=ac._planted_owner())
    out["raw_free_chroma_taps"] = raw_case((96, 130), [(15, 12, 100, 80), (60, 40, 140, 110)], [(7, 6, 50, 40), (31, 19, 70, 55)], "blur", "ellipse", "i420", content="saturating",
                                           luma_taps=[[65534, 1], [2, 32767]], chroma_taps=[[65536 - 2 * 6553 * 4, 6553, 6553, 6553, 6553], [65536]])
    return out


# ---- a case's frame -------------------------------------------------------------------------------------------------------------------------------
def planes_of(case):
    """The dense planes (y, u, v) of the case's picture."""
    h, w = case["shape"]
    return yuv_ref.picture(h, w, case["seed"] + 100, saturating=case["content"] == "saturating")


def geometry_of(case, layout=None):
    """(pitch, extra_rows) of the case's surface: pitched surfaces have 10 (I420: 5) sentinel bytes after every row and 3 sentinel luma rows."""
    h, w = case["shape"]
    cw = (w + 1) // 2
    return (2 * cw + 10, 3) if case["pitched"] else (2 * cw, 0)


def surface_of(case, planes=None, layout=None):
    """(buffer uint8 [n], pitch, uv_offset): the surface that holds ``planes`` (default: the case's picture) in ``layout`` (default: the case's)."""
    pitch, extra = geometry_of(case)
    y, u, v = planes_of(case) if planes is None else planes
    return yuv_ref.surface(case["layout"] if layout is None else layout, y, u, v, pitch=pitch, extra_rows=extra, seed=case["seed"] + 7)


def frame_of(case, buffer, layout=None, **kw):
    """The YUV420Frame over ``buffer`` (a torch tensor holding ``surface_of``'s bytes, on any device): views, no copy."""
    from head_detector_amd.video import YUV420Frame

    h, w = case["shape"]
    pitch, extra = geometry_of(case)
    layout = case["layout"] if layout is None else layout
    make = {"nv12": YUV420Frame.from_nv12, "nv21": YUV420Frame.from_nv21, "i420": YUV420Frame.from_i420}[layout]
    kw.setdefault("matrix", case.get("matrix", "bt709"))
    kw.setdefault("full_range", case.get("full_range", False))
    return make(buffer, h, w, pitch=pitch, uv_offset=pitch * (h + extra), **kw)


# ---- what the restatement makes of it ---------------------------------------------------------------------------------------------------------------
def rows_of(case):
    """dict(luma_boxes, chroma_boxes, luma_cell, chroma_cell, luma_taps, chroma_taps, color_yuv) of a case by the restatement's own arithmetic."""
    if case["kind"] == "raw":
        n = len(case["luma_boxes"])
        return dict(luma_boxes=case["luma_boxes"], chroma_boxes=case["chroma_boxes"], luma_cell=case["luma_cell"] or [1] * n, chroma_cell=case["chroma_cell"] or [1] * n,
                    luma_taps=case["luma_taps"] or [[ref.TAP_SUM]] * n, chroma_taps=case["chroma_taps"] or [[ref.TAP_SUM]] * n, color_yuv=case["color_yuv"])
    h, w = case["shape"]
    if case["region"] == "mesh":
        luma = [ref.mesh_box(hd.vertices_3d, case["faces"], h, w) for hd in case["heads"]]
    else:
        luma = [ref.geometry_box(hd.bbox, case["margin"]) for hd in case["heads"]]
    chroma = [yref.chroma_box(b) for b in luma]
    blur = case["method"] == "blur"
    one = [[ref.TAP_SUM]] * len(luma)
    return dict(luma_boxes=luma, chroma_boxes=chroma, luma_cell=[ref.cell_side(b, case["cells"]) for b in luma], chroma_cell=[ref.cell_side(b, case["cells"]) for b in chroma],
                luma_taps=[ref.taps(*ref.blur_radius(b, case["strength"])) for b in luma] if blur else one,
                chroma_taps=[ref.taps(*ref.blur_radius(b, case["strength"])) for b in chroma] if blur else one,
                color_yuv=yref.pixel_yuv(case["color"], yref.coefficients(case["matrix"], case["full_range"])))


def owner_of(case, luma_boxes):
    """The LUMA owner map the restatement uses: the caller's, the meshes', or painted from the luma boxes."""
    h, w = case["shape"]
    if case["owner"] is not None:
        return case["owner"]
    if case["region"] == "mesh":
        return vr.compose(np.stack([hd.vertices_3d for hd in case["heads"]]), case["faces"], h, w, "order", -1.0)["head_index"]
    return ref.owner_map(h, w, luma_boxes, case["region"])


_EXPECTED = {}


def expected(name, case):
    """The restatement's planes (Y, U, V) of a case, computed once and never modified (read-only arrays)."""
    if name not in _EXPECTED:
        r = rows_of(case)
        y, u, v = planes_of(case)
        want = yref.render_frame(y, u, v, r["luma_boxes"], owner_of(case, r["luma_boxes"]), case["method"], luma_cell=r["luma_cell"], chroma_cell=r["chroma_cell"],
                                 luma_taps=r["luma_taps"], chroma_taps=r["chroma_taps"], chroma_boxes=r["chroma_boxes"], color_yuv=r["color_yuv"])
        for p in want:
            p.setflags(write=False)
        _EXPECTED[name] = want
    return _EXPECTED[name]
