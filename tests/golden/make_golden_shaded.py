"""Records tests/golden/shaded_mesh.npz by RUNNING THE REFERENCE'S C++ (oracle/_ref/libsim3dr_ref.so, built by oracle/build_ref.py from the reference's
sources where they lie): ``_get_normal`` through its mangled symbol and ``_rasterize`` with ``alpha``.  Inputs are generated from seeds by
tests/shade_ref.py and not stored; images are stored as ``result XOR source``.  Run from the repository root: python tests/golden/make_golden_shaded.py

Before anything is written the generator shows that the inputs bite: the blended mesh paints >= 1 000 pixels at least twice and >= 300 at least three
times and its image depends on the triangle order; the scenes have >= 500 pixels covered by two heads and depend on the head order."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import shade_ref as sr  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402


def main():
    assert sr.live() is not None, "the reference library is needed to record the fixture"
    out = {}
    # ---- normals ----
    for seed in sr.NORMAL_SEEDS:
        ver, tri, _ = ro.random_mesh(seed)
        out[f"normals_seed{seed}"] = sr.normals(ver, tri, True)
    ver, tri = sr.corner_case_mesh()
    out["normals_corner"] = sr.normals(ver, tri, True)
    assert not out["normals_corner"][7].any()  # the vertex no triangle names
    unit, tri = sr.ellipsoid()
    assert unit.shape[0] == 5002 and tri.shape[0] == 10000
    head = sr.ellipsoid_heads(np.random.default_rng(11), 1, 400, 400, 200.0, 200.0, unit)[0]
    out["normals_ellipsoid"] = sr.normals(head, tri, True)

    # ---- one blended mesh: every alpha, both row orders ----
    ver, tri, col = ro.random_mesh(2)
    bg = sr.background(2, sr.BLEND_SHAPE)
    counts = np.zeros(sr.BLEND_SHAPE[:2], dtype=np.int64)
    sr.rasterize(bg.copy(), ver, tri, col, 0.6, False, counts)
    twice, thrice = int((counts >= 2).sum()), int((counts >= 3).sum())
    print(f"random_mesh(2): {int((counts >= 1).sum())} covered pixels, {twice} painted at least twice, {thrice} at least three times")
    assert twice >= 1000 and thrice >= 300
    for i, alpha in enumerate(sr.ALPHAS):
        for rev in (0, 1):
            img = sr.blend(bg.copy(), ver, tri, col, alpha, rev, True)
            out[f"blend_a{i}_r{rev}"] = img ^ bg
    flipped = sr.blend(bg.copy(), ver, tri[::-1].copy(), col, 0.6, 0, True)
    changed = int((flipped != (out["blend_a2_r0"] ^ bg)).any(axis=2).sum())
    print(f"reversing the triangle order changes {changed} pixels")
    assert changed >= 1000
    assert not out["blend_a0_r0"].any()  # alpha = 0 leaves every byte: (unsigned char)(1 * byte + 0)

    # ---- a mesh hanging over each edge of an image whose sides are not multiples of 16 ----
    for k, side in enumerate(sr.EDGE_CENTRES):
        ver, tri, col = sr.edge_mesh(side)
        bg = sr.background(10 + k, sr.EDGE_SHAPE)
        xy = ver[tri.reshape(-1)][:, :2]
        over = {"left": xy[:, 0].min() < 0, "right": xy[:, 0].max() > sr.EDGE_SHAPE[1] - 1, "top": xy[:, 1].min() < 0, "bottom": xy[:, 1].max() > sr.EDGE_SHAPE[0] - 1}[side]
        assert over, side
        img = sr.blend(bg.copy(), ver, tri, col, 0.6, k % 2, True)
        assert (img != bg).any()
        out[f"edge_{side}"] = img ^ bg

    # ---- render_mesh: two scenes of 8 overlapping heads ----
    for letter in sr.SCENE_SHAPES:
        bg, heads, tri = sr.scene(letter)
        img = sr.render_mesh(bg, heads, tri, True)
        cover = np.zeros(bg.shape[:2], dtype=np.int64)
        for h in heads:
            v = h.copy()
            v[:, 2] *= -1
            c = np.zeros(bg.shape[:2], dtype=np.int64)
            sr.rasterize(bg.copy(), v, tri, np.ones_like(v), 0.5, False, c)
            cover += c > 0
        both = int((cover >= 2).sum())
        order = int((sr.render_mesh(bg, heads[::-1], tri, True) != img).any(axis=2).sum())
        print(f"scene {letter}: {int((cover >= 1).sum())} covered pixels, {both} by two heads or more, {order} change with the head order")
        assert both >= 500 and order >= 500
        out[f"scene_{letter}"] = img ^ bg
    path = sr.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
