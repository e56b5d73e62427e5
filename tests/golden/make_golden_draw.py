#!/usr/bin/env python3
"""Generate tests/golden/draw_heads.npz by RUNNING THE REFERENCE's own ``PredictionResult.draw(method)``.

Run from the repo root:  python tests/golden/make_golden_draw.py
Needs the reference checkout (REF below); the tests never run this -- only the committed vectors travel.

What is real reference code here and what is stubbed (same manner as make_golden_aligned.py):
  * head_detector/head_info.py, utils.py, draw_utils.py, detection_result.py   imported as they lie -> the real draw, DRAW_MAPPING, draw_bboxes,
                                  draw_3d_landmarks, draw_2d_landmarks, draw_points: which indices, which order, the truncations, the radius, the colours
  * ``cv2``                      := a module whose circle / polylines / rectangle are tests/draw_ref.py (cv2 is not installed; the restatement is
                                  pinned against cv2 itself wherever cv2 exists, see tests/test_draw_host.py)
  * ``draw_utils.TRIANGLES / HEAD_INDICES / FACE_INDICES``   := synthetic topology on the synthetic meshes' V = 300 vertices
  * mesh assets read by PredictionResult.__init__ (PNCCProcessor, MeshSaver): ``np.load`` patched with a four-vertex stand-in
No reference *source* is copied; the fixture holds inputs and recorded outputs only.  To stay small it records every result image as
``result XOR original`` (zero wherever nothing was painted; lossless: the tests XOR the formula image back in).

So the fixture pins the ORCHESTRATION against the reference; the pixel rules of the three primitives are tests/draw_ref.py's (PARITY UNPINNED
against cv2 itself).  No libm value is involved: every truncation is float32 -> int, exact on every machine.

Images are the integer formula of the aligned-head fixture at half its sizes.  The situations the fixture exists for are asserted below.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))

import draw_ref  # noqa: E402

V = 300
SHAPES = {"A": (243, 326), "B": (321, 239)}  # (h, w)
METHODS = ("full", "bbox", "landmarks", "points")
SHARED = 10  # vertices 0 .. 9 are in HEAD_INDICES and in FACE_INDICES: the ones the cases below place by hand


def formula_image(h: int, w: int) -> np.ndarray:
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((x * 7 + y * 13 + c * 71 + (x * y) % 251 + ((x >> 3) ^ (y >> 3)) * 5) & 255).astype(np.uint8)


def cases(H, W):
    """name, centre, radii, vertices placed by hand {index: (x, y)}, bbox override or None."""
    return [
        ("plain", (W * 0.40, H * 0.45), (38.0, 46.0), {}, None),
        ("box_over_plain", (W * 0.52, H * 0.50), (30.0, 33.0), {}, None),  # its box crosses the wire and the dots of "plain"
        ("over_left_trunc_toward_zero", (6.0, H * 0.30), (31.0, 27.0), {0: (-0.7, H * 0.30 + 0.5), 1: (-0.2, -0.9 + H * 0.25), 2: (-0.99, H * 0.35)}, None),
        ("over_top", (W * 0.70, 4.0), (29.0, 24.0), {0: (W * 0.70, -0.4), 1: (W * 0.72, -0.99)}, None),
        ("over_right", (W - 5.0, H * 0.60), (26.0, 30.0), {0: (W - 1 + 0.3, H * 0.60), 1: (W + 0.6, H * 0.62)}, None),
        ("over_bottom", (W * 0.30, H - 3.0), (33.0, 25.0), {0: (W * 0.30, H - 1 + 0.8), 1: (W * 0.31, H + 0.2)}, None),
        ("over_corner", (W - 2.0, H - 2.0), (45.0, 41.0), {}, None),  # segments that need the y step AND the x step of the clip
        ("degenerate", (W * 0.20, H * 0.75), (22.0, 20.0), {5: (W * 0.20, H * 0.75), 6: (W * 0.20, H * 0.75)}, None),  # triangle (5, 6, 7): two equal points
        ("box_w0", (W * 0.80, H * 0.30), (18.0, 21.0), {}, (int(W * 0.80), int(H * 0.30) - 20, 0, 40)),
        ("box_w0_h0_outside", (W * 0.10, H * 0.10), (9.0, 8.0), {}, (-1, int(H * 0.10), 0, 0)),
    ]


def _stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.circle, cv2.polylines, cv2.rectangle = draw_ref.circle, draw_ref.polylines, draw_ref.rectangle
    sys.modules["cv2"] = cv2
    sys.modules["torchvision"] = types.ModuleType("torchvision")  # utils.py imports it for nms(), which is not used here
    pkg = types.ModuleType("head_detector")
    pkg.__path__ = [os.path.join(REF, "head_detector")]
    sys.modules["head_detector"] = pkg
    sim = types.ModuleType("head_detector.Sim3DR")  # pncc_processor.py imports the rasteriser; draw never renders
    sim.rasterize = None
    sys.modules["head_detector.Sim3DR"] = sim
    pkg.Sim3DR = sim


def _load(name):
    spec = importlib.util.spec_from_file_location(f"head_detector.{name}", os.path.join(REF, "head_detector", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[f"head_detector.{name}"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    _stub_modules()
    head_info = _load("head_info")
    _load("utils")
    du = _load("draw_utils")
    _load("pncc_processor")
    det = _load("detection_result")

    rng = np.random.default_rng(2025)
    rest = np.arange(SHARED, V)
    head_indices = np.array(sorted(range(SHARED)) + sorted(rng.choice(rest, 110, replace=False).tolist()))
    face_indices = np.array(sorted(range(SHARED)) + sorted(rng.choice(rest, 70, replace=False).tolist()))
    start = rng.integers(0, V - 24, 180)
    triangles = np.stack([start, start + rng.integers(1, 12, 180), start + rng.integers(12, 24, 180)], axis=1)
    triangles = np.concatenate([triangles, [[5, 6, 7], [9, 9, 9], [0, 1, 2], [299, 0, 150]]]).astype(np.int32)  # two equal points; one point three times
    du.TRIANGLES, du.HEAD_INDICES, du.FACE_INDICES = triangles, head_indices, face_indices
    fake = {"full_faces.npy": np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int64), "v_template.npy": np.eye(4, 3), "head_w_ears.npy": np.arange(4)}
    real_load = np.load

    out = {"triangles": triangles, "head_indices": head_indices, "face_indices": face_indices, "methods": np.array(METHODS)}
    for letter, (H, W) in SHAPES.items():
        image = formula_image(H, W)
        names, verts, boxes, heads = [], [], [], []
        for k, (name, (cx, cy), (rx, ry), placed, box) in enumerate(cases(H, W)):
            r = np.random.default_rng([2025, ord(letter), k])
            ang, rad = r.uniform(0, 2 * np.pi, V), np.sqrt(r.uniform(0, 1, V))
            v = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang), np.round(r.normal(0, 20, V))], axis=1).astype(np.float32)  # z is not drawn
            for i, (px, py) in placed.items():
                v[i, :2] = (px, py)
            if box is None:
                x0, y0, x1, y1 = int(v[:, 0].min()), int(v[:, 1].min()), int(v[:, 0].max()), int(v[:, 1].max())
                box = (x0, y0, x1 - x0, y1 - y0)
            fp = head_info.FlameParams.from_3dmm(torch.zeros(1, 413))
            heads.append(head_info.HeadMetadata(bbox=head_info.Bbox(*box), score=1.0, flame_params=fp, vertices_3d=v.copy(), head_pose=head_info.RPY(0.0, 0.0, 0.0)))
            names.append(name), verts.append(v), boxes.append(box)
        np.load = lambda path, *a, **k: fake[os.path.basename(str(path))]  # det.np and pncc_processor.np are this module
        try:
            pr = det.PredictionResult(image, heads)
        finally:
            np.load = real_load
        results = {m: pr.draw(method=m) for m in METHODS}
        assert np.array_equal(pr.original_image, formula_image(H, W)) and all(np.array_equal(h.vertices_3d, v) for h, v in zip(heads, verts)), "draw modifies no input"

        # ---- the situations the fixture exists for ----
        P = np.trunc(np.stack(verts)[:, :, :2]).astype(np.int64)
        B = np.array(boxes)
        # (1) a later head's box covers an earlier head's wire and dots
        only0 = det.PredictionResult.__new__(det.PredictionResult)
        only0.original_image, only0.heads = image, heads[:1]
        first = only0.draw(method="full")
        final = results["full"]
        red = (final == draw_ref.BOX_COLOUR).all(axis=2)
        assert ((first == draw_ref.WIRE_COLOUR).all(axis=2) & (first != image).any(axis=2) & red).sum() >= 3, "box over wire"
        assert ((first == draw_ref.DOT_COLOUR).all(axis=2) & (first != image).any(axis=2) & red).sum() >= 1, "box over dots"
        # (2) clipped segments at every edge, with the y step, the x step and both
        t = triangles.astype(np.int64)
        edges = {"left": 0, "right": 0, "top": 0, "bottom": 0, "both": 0}
        for h in range(len(heads)):
            a, b, c = P[h][t[:, 0]], P[h][t[:, 1]], P[h][t[:, 2]]
            s, e = np.concatenate([c, a, b]), np.concatenate([a, b, c])
            drawn, x1, y1, x2, y2, moved = draw_ref.clip_lines(W, H, s[:, 0], s[:, 1], e[:, 0], e[:, 1])
            xs, ys = np.stack([s[:, 0], e[:, 0]]), np.stack([s[:, 1], e[:, 1]])
            edges["left"] += int((moved & (xs < 0).any(axis=0)).sum())
            edges["right"] += int((moved & (xs > W - 1).any(axis=0)).sum())
            edges["top"] += int((moved & (ys < 0).any(axis=0)).sum())
            edges["bottom"] += int((moved & (ys > H - 1).any(axis=0)).sum())
            edges["both"] += int((moved & ((xs < 0) | (xs > W - 1)).any(axis=0) & ((ys < 0) | (ys > H - 1)).any(axis=0)).sum())
        assert all(v >= 1 for v in edges.values()), edges
        # (3) clipped dots and clipped bands at every edge (R = 1: a plus whose centre is on the edge pixel, or one pixel outside)
        R = max(1, int(min(H, W) * 0.001))
        assert R == 1
        for idx in (head_indices, face_indices):
            c = P[:, idx].reshape(-1, 2)
            inx, iny = (c[:, 0] >= 0) & (c[:, 0] < W), (c[:, 1] >= 0) & (c[:, 1] < H)
            assert (iny & (c[:, 0] - R < 0) & (c[:, 0] + R >= 0)).any() and (iny & (c[:, 0] + R > W - 1) & (c[:, 0] - R <= W - 1)).any()
            assert (inx & (c[:, 1] - R < 0) & (c[:, 1] + R >= 0)).any() and (inx & (c[:, 1] + R > H - 1) & (c[:, 1] - R <= H - 1)).any()
        x, y, x2, y2 = B[:, 0], B[:, 1], B[:, 0] + B[:, 2], B[:, 1] + B[:, 3]
        assert ((x < 0) & (x2 > 0)).any() and ((x2 > W - 1) & (x < W - 1)).any() and ((y < 0) & (y2 > 0)).any() and ((y2 > H - 1) & (y < H - 1)).any()
        # (4) coordinates between -1 and 0: truncation toward zero (floor would give -1), (5) a zero-length segment, (6) a box with w == 0
        xy = np.stack(verts)[:, :, :2]
        assert ((xy > -1) & (xy < 0)).sum() >= 4 and (np.trunc(xy)[(xy > -1) & (xy < 0)] == 0).all()
        assert (P[names.index("degenerate"), 5] == P[names.index("degenerate"), 6]).all() and (triangles == [5, 6, 7]).all(axis=1).any() and (triangles == [9, 9, 9]).all(axis=1).any()
        assert (B[:, 2] == 0).any() and ((B[:, 2] == 0) & (B[:, 3] == 0)).any()
        painted = {m: int((results[m] != image).any(axis=2).sum()) for m in METHODS}
        assert all(v > 50 for v in painted.values()), painted
        print(letter, (H, W), "clipped segments", edges, "painted pixels", painted)
        out.update({f"shape_{letter}": np.array((H, W)), f"names_{letter}": np.array(names), f"vertices_{letter}": np.stack(verts), f"bbox_{letter}": B.astype(np.int32)})
        for m in METHODS:
            out[f"delta_{letter}_{m}"] = results[m] ^ image
    path = os.path.join(OUT, "draw_heads.npz")
    np.savez_compressed(path, **out)
    print("draw_heads.npz", os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
