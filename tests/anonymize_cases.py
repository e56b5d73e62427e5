"""Planted cases for head anonymisation (include/vgh_anon.h) at the smallest shapes where a kernel can still go wrong, and what the restatement
(tests/anonymize_ref.py) makes of each.  Two kinds:

  api cases   heads (bbox, and vertices for the mesh case) with the public parameters; they run through ``anonymize_heads`` AND through the C call, whose rows
              are then built from the restatement's own arithmetic (``rows_of``), never from the product's plan
  raw cases   hand-made rows and tap tables the public interface cannot produce (an asymmetric-mass table, a radius chosen freely); through the C call only

The 97 x 131 image is odd, no multiple of any tile, and a pitched view of a wider buffer that starts 21 bytes into a row."""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import anonymize_ref as ref  # noqa: E402
import visibility_ref as vr  # noqa: E402

from head_detector_amd.head_info import Bbox  # noqa: E402

H, W, PITCH_W, LEFT = 97, 131, 150, 7


def buffer_of(kind: str, h: int = H, w: int = PITCH_W, seed: int = 0) -> np.ndarray:
    """The wider buffer [h, w, 3]: "random" bytes or a saturating 0 / 255 checkerboard (per pixel and channel)."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return (((x + y + c) % 2) * 255).astype(np.uint8)


def view_of(buffer, width: int = W):
    """The image: columns LEFT .. LEFT + width of the buffer (NumPy array or GPU tensor): rows 3 * PITCH_W bytes apart."""
    return buffer[:, LEFT:LEFT + width]


def head(bbox, vertices=None):
    return types.SimpleNamespace(bbox=Bbox(*(int(v) for v in bbox)), vertices_3d=None if vertices is None else np.array(vertices, dtype=np.float32))


# bboxes (x, y, w, h) on the 97 x 131 image; with margin 0.1 their geometry boxes are what the names say
EDGE_BOXES = [(-9, 20, 30, 25), (110, 30, 40, 22), (40, -8, 33, 21), (50, 85, 27, 30)]  # crossing the left, right, top and bottom edge
ODD_BOXES = [(200, 10, 20, 20), (-60, -60, 30, 30), (30, 40, 0, 17), (60, 50, 9, 0), (70, 60, 1, 1), (-20, -15, 180, 140)]  # outside (2), zero side (2), 1 x 1, larger than the image
OVERLAP_BOXES = [(10, 10, 100, 70), (20, 20, 50, 40), (45, 35, 50, 40), (40, 30, 20, 15)]  # three nested in the first; 1 and 2 overlap; 3 lies across both


def api_case(kind, boxes, method, region, *, margin=0.1, cells=8, strength=0.1, color=(0, 0, 0), owner=None, shape=(H, W), seed=0):
    h, w = shape
    return dict(kind="api", buffer=buffer_of(kind, h, w + PITCH_W - W, seed), width=w, heads=[head(b) for b in boxes], method=method, region=region, margin=margin, cells=cells,
                strength=strength, color=color, owner=owner, faces=None)


def raw_case(kind, boxes, method, region, *, cell=None, tap_tables=None, color=(0, 0, 0), owner=None):
    """``boxes`` are geometry boxes (x0, y0, x1, y1) here."""
    return dict(kind="raw", buffer=buffer_of(kind), width=W, boxes=[tuple(b) for b in boxes], method=method, region=region, cell=cell, tap_tables=tap_tables, color=color, owner=owner)


def _planted_owner():
    """A caller's map for three heads with boxes (10, 10, 60, 50), (50, 30, 120, 90), (0, 60, 40, 97): -1, an out-of-range value, and pixels outside their
    owner's box."""
    o = np.full((H, W), -1, dtype=np.int32)
    o[5:55, 5:70] = 0  # spills over head 0's box on every side: those pixels stay unchanged
    o[40:80, 60:110] = 1
    o[70:97, 0:30] = 2
    o[20:30, 20:30] = 7  # out of range: counts as -1
    o[25:28, 40:50] = -5
    o[0:3, 100:131] = 1  # far outside head 1's box
    return o


OWNER_BOXES = [(10, 10, 50, 40), (50, 30, 70, 60), (0, 60, 40, 37)]  # bboxes; margin 0 in the owner cases


def _mesh_case(method):
    """Two small planted meshes with overlapping silhouettes, as tests/test_gpu_visibility.py builds its two grids: the integer grid mesh and a copy shifted
    by (2, 1)."""
    ver, tri = vr.integer_grid_mesh()
    two = np.stack([ver, ver + np.float32([2, 1, 0.5])])
    c = api_case("random", [(0, 0, 1, 1), (0, 0, 1, 1)], method, "mesh", cells=3, strength=0.05, color=(9, 200, 31), shape=(19, 23), seed=5)
    c["heads"] = [head((0, 0, 1, 1), v) for v in two]
    c["faces"] = tri
    return c


def cases():
    out = {}
    for method in ("fill", "pixelate", "blur"):
        for region in ("box", "ellipse"):
            out[f"edges_{method}_{region}"] = api_case("random", EDGE_BOXES, method, region, color=(255, 0, 128))
            out[f"odd_{method}_{region}"] = api_case("checker" if region == "box" else "random", ODD_BOXES, method, region, strength=0.02, color=(1, 2, 3))
            out[f"overlap_{method}_{region}"] = api_case("random", OVERLAP_BOXES, method, region, margin=0.0, cells=5, strength=0.03)
        out[f"mesh_{method}"] = _mesh_case(method)
        out[f"owner_{method}"] = api_case("random", OWNER_BOXES, method, "box", margin=0.0, cells=6, strength=0.04, color=(0, 255, 0), owner=_planted_owner())
    # pixelate: cell side 1 (the identity), a side that does not divide the box, cells = 64
    out["pixelate_identity"] = api_case("random", [(20, 30, 8, 5)], "pixelate", "box", margin=0.0, cells=8)
    out["pixelate_ragged"] = api_case("checker", [(13, 17, 50, 31)], "pixelate", "box", margin=0.0, cells=7)  # side 8: 7 columns of cells, the last 2 wide; 4 rows, the last 7 tall
    out["pixelate_64"] = api_case("random", [(-5, 3, 140, 90)], "pixelate", "ellipse", margin=0.0, cells=64)
    # blur: r = 0, 1, 70 (wider than a 64-lane segment), larger than both image sides (every tap clamps somewhere)
    out["blur_r0"] = api_case("random", [(20, 30, 40, 30)], "blur", "box", margin=0.0, strength=0.0)
    out["blur_r1"] = api_case("checker", [(20, 30, 30, 20)], "blur", "box", margin=0.0, strength=0.01)
    out["blur_r70"] = api_case("checker", [(10, 2, 93, 80)], "blur", "ellipse", margin=0.0, strength=0.25)
    out["blur_all_clamp"] = api_case("random", [(-30, -10, 200, 110)], "blur", "box", margin=0.0, strength=0.25)
    # head counts
    out["no_heads"] = api_case("random", [], "pixelate", "ellipse")
    out["one_head"] = api_case("random", [(40, 30, 33, 41)], "pixelate", "ellipse")
    rng = np.random.default_rng(11)
    many = [(int(x), int(y), int(w), int(h)) for x, y, w, h in zip(rng.integers(-6, 60, 300), rng.integers(-6, 60, 300), rng.integers(1, 16, 300), rng.integers(1, 16, 300))]
    for method in ("fill", "pixelate", "blur"):
        out[f"many_heads_{method}"] = api_case("random", many, method, "ellipse", cells=4, strength=0.1, color=(7, 7, 7), shape=(64, 64), seed=3)
    # raw: hand-made tables the plan never makes
    box = (15, 12, 100, 80)
    out["raw_asymmetric_mass"] = raw_case("checker", [box], "blur", "box", tap_tables=[[65534, 1]])  # so little mass beside the centre that 8 bits do not show it
    out["raw_side_mass"] = raw_case("random", [box], "blur", "box", tap_tables=[[2, 32767]])  # and nearly all of it beside the centre
    out["raw_flat_table"] = raw_case("random", [box, (60, 40, 140, 110)], "blur", "ellipse", tap_tables=[[65536 - 2 * 6553 * 4, 6553, 6553, 6553, 6553], [65536]])
    out["raw_owner_free_cells"] = raw_case("random", [(10, 10, 60, 50), (50, 30, 120, 90)], "pixelate", "map", cell=[7, 64], owner=_planted_owner())
    return out


def rows_of(case):
    """(boxes, cell, tap_tables) of a case by the restatement's own arithmetic."""
    if case["kind"] == "raw":
        n = len(case["boxes"])
        return case["boxes"], case["cell"] or [1] * n, case["tap_tables"] or [[ref.TAP_SUM]] * n
    h, w = case["buffer"].shape[0], case["width"]
    if case["region"] == "mesh":
        boxes = [ref.mesh_box(hd.vertices_3d, case["faces"], h, w) for hd in case["heads"]]
    else:
        boxes = [ref.geometry_box(hd.bbox, case["margin"]) for hd in case["heads"]]
    cell = [ref.cell_side(b, case["cells"]) for b in boxes]
    tap_tables = [ref.taps(*ref.blur_radius(b, case["strength"])) for b in boxes] if case["method"] == "blur" else [[ref.TAP_SUM]] * len(boxes)
    return boxes, cell, tap_tables


def owner_of(case, boxes):
    """The owner map the restatement uses: the caller's, the meshes' (the CPU composition of tests/visibility_ref.py), or painted from the boxes."""
    h, w = case["buffer"].shape[0], case["width"]
    if case["owner"] is not None:
        return case["owner"]
    if case["region"] == "mesh":
        return vr.compose(np.stack([hd.vertices_3d for hd in case["heads"]]), case["faces"], h, w, "order", -1.0)["head_index"]
    return ref.owner_map(h, w, boxes, case["region"])


_EXPECTED = {}


def expected(name, case):
    """The restatement's picture of a case, computed once and never modified (read-only array)."""
    if name not in _EXPECTED:
        boxes, cell, tap_tables = rows_of(case)
        image = view_of(case["buffer"], case["width"])
        want = ref.render(image, boxes, owner_of(case, boxes), case["method"], cell=cell, tap_tables=tap_tables, color=case["color"])
        want.setflags(write=False)
        _EXPECTED[name] = want
    return _EXPECTED[name]
