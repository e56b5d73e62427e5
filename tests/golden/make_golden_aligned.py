#!/usr/bin/env python3
"""Generate tests/golden/aligned_heads.npz by RUNNING THE REFERENCE's own ``PredictionResult.get_aligned_heads()``.

Run from the repo root:  python tests/golden/make_golden_aligned.py
Needs the reference checkout (REF below); the GPU tests never run this -- only the committed vectors travel.

What is real reference code here and what is stubbed (same manner as make_golden.py):
  * head_detector/head_info.py, utils.py, detection_result.py   imported as they lie -> the real get_aligned_heads, vertically_align,
                                  flame_params_skull_center, get_rotation_mat, refined_head_bbox, extend_bbox, extend_to_rect
  * ``cv2``                      := a module whose getRotationMatrix2D / warpAffine / INTER_LINEAR are tests/warp_affine_ref.py (cv2 is not
                                  installed; the restatement is pinned against cv2 itself wherever cv2 exists, see that file)
  * ``utils.HEAD_INDICES``       := a synthetic subset of the synthetic meshes' V = 300 vertices
  * mesh assets read by PredictionResult.__init__ (PNCCProcessor, MeshSaver): ``np.load`` patched with a four-vertex stand-in; Sim3DR and
                                  draw_utils are not touched by get_aligned_heads
No reference *source* is copied; the fixture holds inputs and recorded outputs only.

Images are an integer formula of (x, y, c) -- ``formula_image`` below, restated in the tests -- one landscape with even sides (A) and one portrait
with odd sides (B).

ROBUSTNESS MARGINS (asserted below): cos / sin may differ by an ulp between machines, so
  * every value that the reference passes through ``int()`` or ``.astype("int32")`` is >= 1e-6 away from an integer, and
  * every value that the warp tables pass through ``rint`` is >= 1e-6 away from a half.
One class of values cannot have the first margin and does not need it: the canvas bounds at roll 0 and roll 90, ``int(h*|sin| + w*|cos|)`` with
one of |sin|, |cos| exactly 1 and the other exactly 0 or ~6e-17 -- an integer plus a non-negative term below 1e-9, whose truncation no libm can change
(cos(0) = 1, sin(0) = 0, sin(pi/2 rounded to double) = 1 are exact in every correctly-rounded or 1-ulp libm, and abs() keeps the small term >= 0).
For those the generator asserts exactly that shape instead.
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

import warp_affine_ref as war  # noqa: E402

V = 300
SHAPE_A, SHAPE_B = (486, 652), (641, 479)  # (h, w): landscape with even sides, portrait with odd sides


def formula_image(h: int, w: int) -> np.ndarray:
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((x * 7 + y * 13 + c * 71 + (x * y) % 251 + ((x >> 3) ^ (y >> 3)) * 5) & 255).astype(np.uint8)


# name, image, head centre, radii, roll, yaw, translation (padded-640 space; it decides the skull centre = the centre of rotation)
CASES = [
    ("pos_roll_tall", "A", (300.0, 240.0), (33.0, 47.0), 17.3, 10.0, (294.9, 399.1)),
    ("neg_roll_wide", "A", (180.0, 150.0), (49.0, 31.0), -23.7, -30.0, (176.3, 309.2)),
    ("yaw_75_no_warp", "A", (500.0, 300.0), (36.0, 41.0), 12.0, 75.0, (490.0, 455.0)),
    ("yaw_60_exactly_no_warp", "A", (100.0, 380.0), (41.0, 33.0), -8.0, 60.0, (98.0, 530.0)),
    ("roll_0_even_sides", "A", (400.0, 200.0), (31.0, 38.0), 0.0, 5.0, (392.2, 358.6)),
    ("roll_90", "A", (320.0, 240.0), (29.0, 44.0), 90.0, -15.0, (313.7, 398.3)),
    ("rotated_clipped_far_edge", "A", (632.0, 470.0), (37.0, 43.0), 5.2, 20.0, (320.4, 402.7)),
    ("no_warp_negative_y_empty", "A", (250.0, 28.0), (32.0, 39.0), 3.0, -70.0, (245.0, 190.0)),
    ("no_warp_negative_x_empty", "A", (24.0, 250.0), (36.0, 33.0), -4.0, 80.0, (24.0, 410.0)),
    ("roll_0_odd_sides", "B", (240.0, 320.0), (34.0, 39.0), 0.0, 0.0, (401.3, 319.7)),
    ("pos_roll_wide_portrait", "B", (200.0, 400.0), (46.0, 32.0), 31.9, 45.0, (361.2, 399.2)),
    ("roll_90_portrait", "B", (260.0, 200.0), (31.0, 36.0), 90.0, 20.0, (421.6, 199.3)),
    ("no_warp_clipped_far_edge", "B", (452.0, 612.0), (33.0, 37.0), 9.0, 65.0, (612.0, 611.0)),
]


def _stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.INTER_LINEAR = war.getRotationMatrix2D, war.warpAffine, war.INTER_LINEAR
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")  # utils.py imports it for nms(), which is not used here
    sys.modules["torchvision"] = tv
    pkg = types.ModuleType("head_detector")
    pkg.__path__ = [os.path.join(REF, "head_detector")]
    sys.modules["head_detector"] = pkg
    sim = types.ModuleType("head_detector.Sim3DR")  # pncc_processor.py imports the rasteriser; get_aligned_heads never renders
    sim.rasterize = None
    sys.modules["head_detector.Sim3DR"] = sim
    pkg.Sim3DR = sim


def _load(name):
    spec = importlib.util.spec_from_file_location(f"head_detector.{name}", os.path.join(REF, "head_detector", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[f"head_detector.{name}"] = mod
    spec.loader.exec_module(mod)
    return mod


class _Recorder:
    """Stands in for ``int`` and ``np`` inside the reference's utils module: same results, every truncated value is written down."""

    def __init__(self):
        self.truncated = []  # (function name, value)

    def int(self, v):
        self.truncated.append((sys._getframe(1).f_code.co_name, float(v)))
        return int(v)

    def numpy_proxy(self):
        rec = self

        class Checked(np.ndarray):
            def astype(self, dtype, *a, **k):
                if str(dtype) == "int32":
                    rec.truncated.extend(("astype_int32", float(v)) for v in np.asarray(self).ravel())
                return np.asarray(self).astype(dtype, *a, **k)

        class Proxy:
            def __getattr__(self, name):
                return getattr(np, name)

            def array(self, *a, **k):
                r = np.array(*a, **k)
                return r.view(Checked) if r.dtype.kind == "f" else r

        return Proxy()


def _int_margin(v: float) -> float:
    return abs(v - round(v))


def main():
    _stub_modules()
    head_info = _load("head_info")
    utils = _load("utils")
    _load("draw_utils")
    _load("pncc_processor")
    det = _load("detection_result")

    rng = np.random.default_rng(2024)
    head_indices = np.array(sorted(rng.choice(V, 120, replace=False).tolist()))
    utils.HEAD_INDICES = head_indices
    rec = _Recorder()
    utils.int = rec.int
    utils.np = rec.numpy_proxy()
    calls = {"rot": [], "rect": []}
    real_rot, real_rect = utils.get_rotation_mat, det.extend_to_rect

    def get_rotation_mat(img, center, angle):
        m, b = real_rot(img, center, angle)
        calls["rot"].append((m.copy(), tuple(int(v) for v in b), tuple(center)))
        return m, b

    def extend_to_rect(bbox):
        r = real_rect(bbox)
        calls["rect"].append((np.asarray(r).copy(), bool(bbox[2] > bbox[3])))
        return r

    utils.get_rotation_mat, det.extend_to_rect = get_rotation_mat, extend_to_rect
    fake = {"full_faces.npy": np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int64), "v_template.npy": np.eye(4, 3), "head_w_ears.npy": np.arange(4)}
    real_load = np.load
    images = {"A": formula_image(*SHAPE_A), "B": formula_image(*SHAPE_B)}
    assert SHAPE_A[0] % 2 == 0 and SHAPE_A[1] % 2 == 0 and SHAPE_A[1] > SHAPE_A[0] and SHAPE_B[0] % 2 == 1 and SHAPE_B[1] % 2 == 1 and SHAPE_B[0] > SHAPE_B[1]

    out = {"head_indices": head_indices, "names": np.array([c[0] for c in CASES]), "image": np.array([c[1] for c in CASES]),
           "shape_A": np.array(SHAPE_A), "shape_B": np.array(SHAPE_B)}
    verts_all, trans, roll, yaw, rotated, matrix, bounds, rect, shapes, crops, centres = [], [], [], [], [], [], [], [], [], [], []
    seen = set()
    try:
        for case in CASES:
            name, im, (cx, cy), (rx, ry), r, yw, t = case
            # the mesh of a head is the first of its seeded draws for which the robustness margins hold (e.g. a bbox side that is a multiple of 5
            # makes w * 1.2 an integer up to rounding): the head parameters are CHOSEN so that the margins hold, as the fixture requires
            for attempt in range(64):
                rng = np.random.default_rng([2024, CASES.index(case), attempt])
                ang, rad = rng.uniform(0, 2 * np.pi, V), np.sqrt(rng.uniform(0, 1, V))
                v = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang), rng.normal(0, 20, V)], axis=1).astype(np.float32)
                fp = head_info.FlameParams.from_3dmm(torch.zeros(1, 413))
                fp.translation = torch.tensor([[t[0], t[1], 0.0]], dtype=torch.float32)
                head = head_info.HeadMetadata(bbox=head_info.Bbox(0, 0, 1, 1), score=1.0, flame_params=fp, vertices_3d=v.copy(), head_pose=head_info.RPY(roll=r, pitch=0.0, yaw=yw))
                image = images[im]
                H, W = image.shape[:2]
                rec.truncated.clear()
                calls["rot"].clear()
                calls["rect"].clear()
                war.STATS = {}
                np.load = lambda path, *a, **k: fake[os.path.basename(str(path))]  # det.np and pncc_processor.np are this module
                try:
                    pr = det.PredictionResult(image, [head])
                finally:
                    np.load = real_load
                (crop,) = pr.get_aligned_heads()
                assert np.array_equal(head.vertices_3d, v) and np.array_equal(pr.original_image, images[im]), "the reference does not modify its inputs"
                is_rot = len(calls["rot"]) == 1
                assert is_rot == (abs(yw) < 60)
                m, b, centre = calls["rot"][0] if is_rot else (np.array([[1.0, 0, 0], [0, 1.0, 0]]), (W, H), (0, 0))
                (rc, wide), = calls["rect"]
                x, y, w, h = (int(q) for q in rc)
                # ---- margins ----
                axis_aligned = r in (0.0, 90.0)
                ok = True
                for fn, val in rec.truncated:
                    if fn == "get_rotation_mat" and axis_aligned:
                        assert 0 <= val - np.floor(val) < 1e-9, (name, fn, val)
                    else:
                        ok = ok and _int_margin(val) >= 1e-6
                if is_rot:
                    ok = ok and war.STATS["half_margin"] >= 1e-6
                if ok:
                    break
            else:
                raise AssertionError(f"{name}: no mesh draw satisfies the margins")
            # ---- which of the required situations this head is ----
            if is_rot and r > 0 and not axis_aligned:
                seen.add("positive roll")
            if is_rot and r < 0:
                seen.add("negative roll")
            if abs(yw) > 60:
                seen.add("abs(yaw) > 60")
            if yw == 60:
                seen.add("yaw == 60")
            if is_rot and r == 0:
                shift = m[0, 2]
                assert m[0, 0] == 1 and m[0, 1] == 0
                seen.add("roll 0, integer shift" if shift == int(shift) and m[1, 2] == int(m[1, 2]) else "roll 0, half-pixel shift")
                assert (shift == int(shift) and m[1, 2] == int(m[1, 2])) == (H % 2 == 0 and W % 2 == 0)
                assert H % 2 == 0 or (abs(shift * 2 % 2) == 1 and abs(m[1, 2] * 2 % 2) == 1)
            if is_rot and r == 90:
                seen.add("roll 90")
            seen.add("extend_to_rect w > h" if wide else "extend_to_rect w <= h")
            if crop.size and (x + w > b[0] or y + h > b[1]) and x >= 0 and y >= 0:
                seen.add("clipped at the far edge, rotated" if is_rot else "clipped at the far edge, un-rotated")
                assert crop.shape[0] < h or crop.shape[1] < w
            if not is_rot and (x < 0 or y < 0) and crop.size == 0:
                seen.add("negative start, empty crop " + str(crop.shape))
            print(f"{name:28s} rot={int(is_rot)} bounds={b} rect={(x, y, w, h)} crop={crop.shape} int-margin={min(_int_margin(q) for _, q in rec.truncated):.2e} "
                  f"half-margin={war.STATS.get('half_margin', float('nan')):.2e} draw={attempt}")
            verts_all.append(v), trans.append(t), roll.append(r), yaw.append(yw), rotated.append(is_rot), matrix.append(m), bounds.append(b), rect.append((x, y, w, h))
            shapes.append(crop.shape), crops.append(np.ascontiguousarray(crop).reshape(-1)), centres.append(centre)
    finally:
        war.STATS = None
    need = {"positive roll", "negative roll", "abs(yaw) > 60", "yaw == 60", "roll 0, integer shift", "roll 0, half-pixel shift", "roll 90", "extend_to_rect w > h",
            "extend_to_rect w <= h", "clipped at the far edge, rotated", "negative start, empty crop"}
    missing = {n for n in need if not any(s.startswith(n) for s in seen)}
    assert not missing, missing
    empties = sorted(s for s in seen if s.startswith("negative start"))
    assert any("(0, " in s for s in empties) and any(", 0, 3)" in s for s in empties), empties
    out.update(vertices=np.stack(verts_all), translation=np.array(trans, dtype=np.float32), roll=np.array(roll), yaw=np.array(yaw), rotated=np.array(rotated),
               matrix=np.stack(matrix), bounds=np.array(bounds), rect=np.array(rect), crop_shape=np.array(shapes), skull_centre=np.array(centres),
               crop_bytes=np.concatenate(crops))
    path = os.path.join(OUT, "aligned_heads.npz")
    np.savez_compressed(path, **out)
    print("aligned_heads.npz", os.path.getsize(path) // 1024, "KiB;", sorted(seen))


if __name__ == "__main__":
    main()
