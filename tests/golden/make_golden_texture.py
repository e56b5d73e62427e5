"""Records tests/golden/texture.npz by RUNNING THE REFERENCE'S C++ (oracle/_ref/libsim3dr_ref.so, built by oracle/build_ref.py from the reference's sources
where they lie): ``_render_texture_core``, taken by its mangled name and composed as tests/texture_ref.py states.  Inputs are generated from seeds and not
stored; colour and depth are stored for written pixels only (texture_ref.encode).  Run from the repository root:
python tests/golden/make_golden_texture.py

Before anything is written the generator shows that the inputs bite; every count it prints must be above zero."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import texture_ref as tr  # noqa: E402
import visibility_ref as vr  # noqa: E402


def bite(what: str, count: int) -> None:
    print(f"  {what}: {int(count)}")
    assert count > 0, what


def main():
    assert tr.live() is not None and vr.live() is not None, "the reference library is needed to record the fixture"
    out = {}
    results = {}
    stats = {}
    cases = tr.cases()
    for name, kw in cases.items():
        res = tr.compose(use_live=True, **kw)
        stats[name] = {}
        tr.same(tr.compose(stats=stats[name], **kw), res, (name, "the restatement against the reference's C++"))
        results[name] = res
        base = results.get(tr.BASES.get(name))
        enc = tr.encode(res, base)
        tr.same(tr.decode(enc, kw.get("image"), base), res, (name, "the encoding loses nothing"))
        for k, a in enc.items():
            out[f"{name}.{k}"] = a
        print(f"{name}: {int((res['triangle'] >= 0).sum())} of {res['triangle'].size} pixels written, {stats[name]}")

    print("the inputs bite:")
    a = cases["A_order"]
    plain = tr.compose(frame=False, **a)
    only = (results["A_order"]["triangle"] >= 0) & (plain["triangle"] < 0)
    H, W = a["H"], a["W"]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for side, sel in (("left", xx < 2), ("right", xx > W - 3), ("top", yy < 2), ("bottom", yy > H - 3)):
        bite(f"pixels covered only because of the frame rule, {side} border", (only & sel).sum())
    assert not (only & ~((xx < 2) | (xx > W - 3) | (yy < 2) | (yy > H - 3))).any()
    bite("clamped texture positions (A)", stats["A_order"]["clamped"])
    bite("clamped texture positions (B)", stats["B_order"]["clamped"])
    bite("nearest lookups at exactly .5", stats["quad_half"]["half"])
    bite("bilinear lookups at integer coordinates", stats["quad_integer"]["integer"])
    bite("pixels of a zero-determinant triangle", stats["corner"]["zero_det"])
    bite("pixels of the zero-determinant triangle that stay", (results["corner"]["triangle"] == 5).sum())
    for s in ("A", "B"):
        o, d = results[f"{s}_order"], results[f"{s}_depth"]
        bite(f"pixels where ORDER and DEPTH differ ({s})", ((o["head"] != d["head"]) | (o["triangle"] != d["triangle"])).sum())
    b = cases["B_order"]
    proper = tr.compose(quirk=False, **b)
    bite("pixels where reading texture y through the mesh's index changes the result", (proper["image"] != results["B_order"]["image"]).any(axis=-1).sum())
    assert np.array_equal(proper["triangle"], results["B_order"]["triangle"])  # the geometry is the same, only the colours differ

    for name, kw in tr.unwrap_cases().items():
        res = tr.unwrap(use_live=True, **kw)
        tr.same(tr.unwrap(**kw), res, (name, "the restatement against the reference's C++"))
        enc = tr.encode(res)
        tr.same(tr.decode(enc), res, (name, "the encoding loses nothing"))
        for k, a in enc.items():
            out[f"{name}.{k}"] = a
        results[name] = res
        print(f"{name}: {(res['triangle'] >= 0).sum(axis=(1, 2)).tolist()} of {res['triangle'][0].size} texels written, finite: {bool(np.isfinite(res['image']).all())}")
        plain = tr.unwrap(frame=False, **kw)
        print(f"  texels whose triangle the frame rule changes: {int((res['triangle'] != plain['triangle']).sum())}")

    back = tr.roundtrip(True)
    tr.same(tr.roundtrip(False), back, "roundtrip: the restatement against the reference's C++")
    img = tr.roundtrip_scene()[0]
    cov = back["triangle"] >= 0
    inner = cov.copy()  # without the mesh's outline, where the bilinear lookup mixes in texels that nothing wrote
    inner[1:] &= cov[:-1]
    inner[:-1] &= cov[1:]
    inner[:, 1:] &= cov[:, :-1]
    inner[:, :-1] &= cov[:, 1:]
    err, err_inner = (np.abs(back["image"][m] - img[m].astype(np.float32)).mean() for m in (cov, inner))
    print(f"roundtrip: {back['texels']} texels, {int(cov.sum())} pixels covered, mean absolute error {err:.3f} grey levels, {err_inner:.3f} without the outline")
    assert err_inner < 1.0  # a smooth photograph comes back almost unchanged
    for k, a in tr.encode(back).items():
        out[f"roundtrip.{k}"] = a

    image, heads, faces, uv, (th, tw) = tr.result_scene()
    for occ in ("order", "depth"):
        got = tr.get_textures(image, heads, faces, uv, th, tw, "bilinear", True, occ, use_live=True)
        again = tr.get_textures(image, heads, faces, uv, th, tw, "bilinear", True, occ, use_live=False)
        assert all(np.array_equal(got[k], again[k]) for k in got)
        assert np.array_equal(got["texture"], results["unwrap_A"]["image"]) and np.array_equal(got["triangle"], results["unwrap_A"]["triangle"])
        vis = vr.compose(heads, faces, image.shape[0], image.shape[1], occ, -1.0, True)
        partly = (vis["visible_pixels"] > 0) & (vis["visible_pixels"] < vis["covered_pixels"])
        removed = (got["written"] & ~got["mask"]).sum(axis=(1, 2))
        print(f"get_textures, {occ}: visible {vis['visible_pixels'].tolist()} of {vis['covered_pixels'].tolist()} pixels, texels removed {removed.tolist()}")
        bite("texels of a partly hidden head that visible_only removes", removed[partly].sum())
        out[f"result.mask_{occ}"] = np.packbits(got["mask"])
        painted = tr.paint(image, heads, faces, got["texture"], uv, "bilinear", occ, use_live=True)
        assert np.array_equal(painted, tr.paint(image, heads, faces, got["texture"], uv, "bilinear", occ, use_live=False))
        out[f"result.painted_{occ}"] = painted
        print(f"  painted back: {int((painted != image).any(axis=-1).sum())} pixels differ from the photograph")
    np.savez_compressed(tr.GOLDEN, **out)
    print(tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes")
    assert os.path.getsize(tr.GOLDEN) < 400 * 1024


if __name__ == "__main__":
    main()
