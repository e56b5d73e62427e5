"""Records tests/golden/visibility.npz by RUNNING THE REFERENCE'S C++ (oracle/_ref/libsim3dr_ref.so, built by oracle/build_ref.py from the reference's
sources where they lie): ``_rasterize_triangles`` through ``ref_rasterize_triangles``, composed as tests/visibility_ref.py states.  Inputs are generated
from seeds and not stored; depth and weights are stored for owned pixels only (visibility_ref.encode).  Run from the repository root:
python tests/golden/make_golden_visibility.py

Before anything is written the generator shows that the inputs bite: heads hidden partly and wholly, modes that differ, a degenerate triangle that owns
pixels, an integer-grid mesh on which the two inside rules own different pixels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import visibility_ref as vr  # noqa: E402


def main():
    assert vr.live() is not None, "the reference library is needed to record the fixture"
    out = {}

    def put(name, res, base=None):
        enc = vr.encode(res, base)
        vr.same(vr.decode(enc, base), res, name)  # the encoding loses nothing (w0 is float32(float32(1 - u) - v) in the C++ too)
        for k, a in enc.items():
            out[f"{name}.{k}"] = a

    for letter in ("A", "B"):
        (H, W), heads, tri = vr.scene(letter)
        order = vr.compose(heads, tri, H, W, "order", vr.SCENE_Z_SIGN, True)
        depth = vr.compose(heads, tri, H, W, "depth", vr.SCENE_Z_SIGN, True)
        differ = int(((order["head_index"] != depth["head_index"]) | (order["triangle_index"] != depth["triangle_index"])).sum())
        print(f"scene {letter}: covered {order['covered_pixels'].tolist()}")
        for mode, res in (("order", order), ("depth", depth)):
            vis, cov = res["visible_pixels"], res["covered_pixels"]
            print(f"  {mode}: visible {vis.tolist()}, partly hidden {int(((vis > 0) & (vis < cov)).sum())}, wholly hidden {int(((cov > 0) & (vis == 0)).sum())}, "
                  f"visible vertices {res['vertex_visible'].sum(1).tolist()}")
            assert int(((vis > 0) & (vis < cov)).sum()) >= 6  # partly occluded: a wholly hidden head does not count
        print(f"  the modes differ on {differ} pixels")
        assert differ > (1000 if letter == "A" else 100)
        put(f"scene_{letter}_order", order)
        put(f"scene_{letter}_depth", depth, order)
    for name, (ver, tri, (H, W)) in vr.single_cases().items():
        res = vr.compose(ver, tri, H, W, "order", 1.0, True)
        other = vr.compose(ver, tri, H, W, "order", 1.0, False, rule="gt")
        diff = int(((res["triangle_index"] >= 0) != (other["triangle_index"] >= 0)).sum())
        print(f"{name}: {int(res['covered_pixels'][0])} covered pixels; the > 0 rule covers {int(other['covered_pixels'][0])}, {diff} pixels differ in coverage")
        if name == "corner":
            block = res["triangle_index"] == 5
            print(f"  the zero-determinant triangle 5 owns {int(block.sum())} pixels")
            assert block.sum() > 0 and np.array_equal(res["barycentric"][block], np.tile(np.float32([1, 0, 0]), (int(block.sum()), 1)))
        if name == "grid":
            assert diff > 0
        if name.startswith("edge_"):
            xy, side = ver[tri.reshape(-1)][:, :2], name[5:]
            assert {"left": xy[:, 0].min() < 0, "right": xy[:, 0].max() > W - 1, "top": xy[:, 1].min() < 0, "bottom": xy[:, 1].max() > H - 1}[side], side
            assert res["covered_pixels"][0] > 300
        put(name, res)
    np.savez_compressed(vr.GOLDEN, **out)
    print(vr.GOLDEN, os.path.getsize(vr.GOLDEN), "bytes")
    assert os.path.getsize(vr.GOLDEN) < 400 * 1024


if __name__ == "__main__":
    main()
