"""Host half of sliced detection (head_detector_amd/sliced.py, include/vgh_merge.h): the tile plan against brute force, the FlameParams conversion against a
direct projection, the two forms of the merge restatement (tests/slice_merge_ref.py) against each other and against what every planted family is meant to
contain, argument errors, and the ABI of libvghmerge.so.  No GPU."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slice_merge_ref as ref  # noqa: E402

from head_detector_amd import _lib_merge, sliced  # noqa: E402
from head_detector_amd.letterbox import geometry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------
def test_axis_rule_by_brute_force():
    """Every pixel is covered, the last tile ends at L, and every interval of length <= t - stride - 2 m lies inside some tile at least m from that tile's
    interior edges (m = the merge's border: a head that small is seen whole, and not as truncated, by at least one tile)."""
    cases = 0
    for L in list(range(1, 81)) + [97, 128, 200]:
        for t in (8, 16, 31):
            for overlap in (0.0, 0.25, 0.5, 0.8):
                offs = sliced.axis_offsets(L, t, overlap)
                if L <= t:
                    assert offs == [0]
                    continue
                stride = max(1, int(t * (1 - overlap)))
                assert offs == [min(k * stride, L - t) for k in range(math.ceil((L - t) / stride) + 1)]
                assert offs[0] == 0 and offs[-1] + t == L and all(b > a for a, b in zip(offs, offs[1:]))
                covered = np.zeros(L, bool)
                for o in offs:
                    covered[o:o + t] = True
                assert covered.all()
                for m in (0, 1, 2):
                    span = t - stride - 2 * m
                    for length in range(1, span + 1):
                        for a in range(0, L - length + 1):
                            b = a + length
                            assert any((a >= o + m or o == 0) and (b <= o + t - m or o + t == L) and a >= o and b <= o + t for o in offs), (L, t, overlap, m, a, b)
                            cases += 1
    assert cases > 100000


def test_plan_tables():
    plan = sliced.plan_slices(3000, 4000, 640, overlap=0.25)
    assert plan.n_tiles == 8 * 6 + 1 and plan.tiles.dtype == np.int32 and plan.tiles.shape == (49, 8)
    assert plan.scale.dtype == np.float32 and plan.interior.dtype == np.uint8 and plan.unpad.dtype == np.float32 and plan.unpad.shape == (49, 3)
    assert plan.tiles[0].tolist() == [0, 0, 4000, 3000, 0, 80, 640, 480] and plan.interior[0] == 0 and plan.scale[0] == np.float32(0.16)
    assert sorted(set(plan.tiles[1:, 0].tolist())) == [0, 480, 960, 1440, 1920, 2400, 2880, 3360] and sorted(set(plan.tiles[1:, 1].tolist())) == [0, 480, 960, 1440, 1920, 2360]
    assert plan.tiles[1:9, 0].tolist() == [0, 480, 960, 1440, 1920, 2400, 2880, 3360] and set(plan.tiles[1:9, 1].tolist()) == {0}  # row-major
    assert (plan.tiles[1:, 2:] == [640, 640, 0, 0, 640, 640]).all() and (plan.scale[1:] == 1).all()
    for t in range(plan.n_tiles):
        x, y, w, h, px, py, nw, nh = plan.tiles[t].tolist()
        assert (nh, nw, px, py) == geometry(h, w, 640)[:4] and plan.scale[t] == np.float32(geometry(h, w, 640)[4])
        want = 0 if t == 0 else (x > 0) | (y > 0) << 1 | (x + w < 4000) << 2 | (y + h < 3000) << 3
        assert plan.interior[t] == want
        s = 640 / max(h, w)
        assert np.array_equal(plan.unpad[t], np.float32([px - x * s, py - y * s, s]))
    last = plan.tiles[-1].tolist()  # the shifted last tile: 2360 + 640 = 3000, not 5 * 480 = 2400
    assert last[:4] == [3360, 2360, 640, 640] and plan.interior[-1] == 1 | 2 and np.array_equal(plan.unpad[-1], np.float32([-3360, -2360, 1]))
    # an image smaller than a tile: the tile IS the whole image and is dropped as a duplicate; without include_full it stays, with no interior edge
    small = sliced.plan_slices(300, 500, 640)
    assert small.n_tiles == 1 and small.tiles[0].tolist() == [0, 0, 500, 300, 0, 128, 640, 384] and small.interior[0] == 0
    assert np.array_equal(small.unpad[0], np.float32([0, 128, 640 / 500]))
    alone = sliced.plan_slices(300, 500, 640, include_full=False)
    assert alone.n_tiles == 1 and np.array_equal(alone.tiles, small.tiles) and alone.interior[0] == 0
    # smaller than a tile along one axis only: tiles of 640 x 300, letterboxed with padding, edges top and bottom on the image boundary
    strip = sliced.plan_slices(300, 1500, 640, include_full=False)
    assert strip.tiles[:, :4].tolist() == [[0, 0, 640, 300], [480, 0, 640, 300], [860, 0, 640, 300]] and strip.interior.tolist() == [4, 1 | 4, 1]
    assert (strip.tiles[:, 4:] == [0, 170, 640, 300]).all() and np.array_equal(strip.unpad[2], np.float32([-860, 170, 1]))
    # several sizes, one set per entry; only the whole image
    two = sliced.plan_slices(1000, 1000, 640, tile_sizes=(640, 320), overlap=0.5)
    assert two.n_tiles == 1 + 9 + 36 and (two.tiles[1:10, 2] == 640).all() and (two.tiles[10:, 2] == 320).all() and (two.scale[10:] == 2).all()
    only = sliced.plan_slices(900, 1300, 640, tile_sizes=())
    assert only.n_tiles == 1 and only.interior[0] == 0
    assert sliced.plan_slices(900, 1300, 640).n_tiles == 6 + 1


def test_image_boxes_are_clipped_to_the_image_but_for_the_whole_image_tile():
    plan = sliced.plan_slices(300, 1500, 640)  # tile 0 the whole image, tiles 1 .. 3 of 640 x 300 with a letterbox border above and below
    full = np.float32([[-3.4, -20.5, 1510.2, 310.5], [-3.4, -20.5, 650.5, 310.5], [10.5, 11.5, 12.4, 299.6]])
    assert sliced.image_boxes(full, [0, 1, 3], plan).tolist() == [[-3, -20, 1510, 310], [0, 0, 650, 300], [10, 12, 12, 300]]  # rint: halves to even
    assert sliced.image_boxes(full[:0], [], plan).shape == (0, 4)


def test_plan_argument_errors():
    for bad in (-0.1, 0.95, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            sliced.plan_slices(100, 100, 64, overlap=bad)
    for bad in (0, -8, 7.5):
        with pytest.raises(ValueError, match="tile size"):
            sliced.plan_slices(100, 100, 64, tile_sizes=(bad,))
    with pytest.raises(ValueError, match="elongated"):
        sliced.plan_slices(1, 4000, 640, tile_sizes=())  # the whole image: 1 x 4000, what the raw-image path rejects
    with pytest.raises(ValueError, match="elongated"):
        sliced.plan_slices(1, 4000, 640, include_full=False, tile_sizes=(1000,))  # tiles of 1000 x 1
    with pytest.raises(ValueError, match="no tile"):
        sliced.plan_slices(100, 100, 64, tile_sizes=(), include_full=False)


# ---- FlameParams in the convention of a whole-image detection ------------------------------------------------------------------------------------------
def test_flame_params_conversion_round_trips_in_float64():
    """A vertex projected by the tile's network parameters and un-padded with the tile's row lands where the converted parameters put it when they are read the
    way a whole-image detection's are (translation in the whole image's padded space, scale already divided by the whole image's letterbox scale)."""
    rng = np.random.default_rng(0)
    H, W, S = 3000, 4000, 640
    plan = sliced.plan_slices(H, W, S, tile_sizes=(640, 1000))
    _, _, fpx, fpy, s_f = geometry(H, W, S)
    for t in (0, 1, 7, 30, plan.n_tiles - 1):
        x, y, w, h, px, py, _, _ = plan.tiles[t].tolist()
        s_t = S / max(h, w)
        v = rng.normal(size=(50, 3))
        tr, sc = rng.uniform(100, 500, 3), rng.uniform(50, 200)
        direct = (v * sc + tr - [px, py, 0]) / s_t + [x, y, 0]  # image coordinates, the way the decode kernel un-pads: (x - pad) / s, z / s
        assert np.allclose(direct[:, :2], (v * sc + tr)[:, :2] / plan.unpad[t, 2] - plan.unpad[t, :2].astype(np.float64) / plan.unpad[t, 2], atol=1e-2)
        tr2, sc2 = sliced.to_whole_image_params(tr.copy(), sc, plan.tiles[t], H, W, S)
        whole = (v * (sc2 * s_f) + tr2 - [fpx, fpy, 0]) / s_f
        np.testing.assert_allclose(whole, direct, rtol=1e-12, atol=1e-9)
        if t == 0:
            assert tr2 is not None and np.array_equal(tr2, tr) and sc2 == sc / s_f  # passed through untouched
    tr = torch.tensor([[320.0, 200.0, 50.0]])
    out, sc = sliced.to_whole_image_params(tr, torch.tensor([[100.0]]), plan.tiles[1], H, W, S)
    assert out.dtype == torch.float32 and out.shape == (1, 3) and torch.equal(tr, torch.tensor([[320.0, 200.0, 50.0]])) and float(sc) == 100.0
    assert torch.allclose(out, torch.tensor([[320 * 0.16, 200 * 0.16 + 80, 50 * 0.16]]))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def _existing_status(case, out):
    return [int(out["status"][r]) for r in case["rows"]]


def test_planted_cases_hold_what_they_are_meant_to():
    cases = ref.planted_cases()
    assert {"chain", "same_tile_pair", "equal_scores_identical_boxes", "exact_threshold", "zero_area", "ios_nested", "border", "everything_dropped", "cap"} <= set(cases)
    for name, c in cases.items():
        loop = ref.merge_loop(c["boxes"], c["scores"], c["counts"], c["plan"], **c["kwargs"])
        vec = ref.merge_vec(c["boxes"], c["scores"], c["counts"], c["plan"], **c["kwargs"])
        assert ref.same_bytes(loop, vec) is None, (name, ref.same_bytes(loop, vec))
        got = _existing_status(c, loop)
        if c["expect"] is not None:
            assert got == c["expect"], (name, got)
        assert c["must_have"] <= set(got), (name, got)
        assert int((loop["status"] != 0).sum()) == int(c["counts"].sum())
        n = int(loop["n_heads"][0])
        assert n == sum(s == 1 for s in got) and int(loop["n_kept_uncapped"][0]) == sum(s in (1, 4) for s in got)
        assert (loop["head_row"][n:] == -1).all() and not loop["boxes_full"][n:].any()
    got = _existing_status(cases["border"], ref.merge_loop(**{k: cases["border"][k] for k in ("boxes", "scores", "counts", "plan")}))
    assert [s == 2 for s in got] == ref.border_expectation()
    c = cases["chain"]
    out = ref.merge_loop(c["boxes"], c["scores"], c["counts"], c["plan"])
    assert out["head_row"][:2].tolist() == [4, 16] and out["head_tile"][:2].tolist() == [1, 4] and out["boxes_full"][1].tolist() == [48, 38, 64, 54]
    c = cases["non_finite"]  # a positive NaN score goes first, +0 before -0, a negative NaN last; NaN / infinite coordinates are clipped
    out = ref.merge_loop(c["boxes"], c["scores"], c["counts"], c["plan"])
    assert out["head_row"][0] == 2 * 4 and np.isnan(out["scores"][0]) and out["head_row"][1] == 0 and np.isfinite(out["boxes_full"]).all()
    assert _existing_status(c, out)[2] == 2


def test_loop_form_equals_vectorised_form_on_random_families():
    plans = [ref.small_plan(), sliced.plan_slices(64, 64, 64), sliced.plan_slices(100, 150, 64, tile_sizes=(64, 40), overlap=0.5)]
    seen = set()
    for seed in range(12):
        plan = plans[seed % 3]
        keep_k = (13, 3, 5)[seed % 3]
        n_live = (seed * 37) % (plan.n_tiles * keep_k + 1)
        boxes, scores, counts = ref.random_family(plan, keep_k, n_live, seed, head_px=(8.0, 30.0))
        assert int(counts.sum()) == n_live
        for kw in (dict(), dict(metric="ios", match_thr=0.6, border=1.0, max_heads=5)):
            loop, vec = ref.merge_loop(boxes, scores, counts, plan, **kw), ref.merge_vec(boxes, scores, counts, plan, **kw)
            assert ref.same_bytes(loop, vec) is None, (seed, kw, ref.same_bytes(loop, vec))
            seen |= set(loop["status"].tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_merge_argument_errors_need_no_gpu():
    plan = ref.small_plan()
    b, s, c = torch.zeros(5, 4, 4), torch.zeros(5, 4), torch.zeros(5, dtype=torch.int32)
    for kw, words in ((dict(metric="giou"), "metric"), (dict(max_heads=0), "max_heads"), (dict(border=-1.0), "border"), (dict(border=float("inf")), "border"),
                      (dict(match_thr=float("nan")), "match_thr")):
        with pytest.raises(ValueError, match=words):
            sliced.merge_tiles(b, s, c, plan, **kw)
    for args, words in (((b.double(), s, c), "boxes"), ((b, s, c.long()), "counts"), ((b.numpy(), s, c), "boxes"), ((b[:4], s, c), r"T = 5"), ((b, s[:, :3], c), "scores"),
                        ((b, s, c[:3]), "counts"), ((b, s, c), "GPU")):
        with pytest.raises(ValueError, match=words):
            sliced.merge_tiles(*args, plan)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def test_merge_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_merge.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vghm_[a-z0-9_]+)\s*\(", code))
    want = {"vghm_version", "vghm_last_error", "vghm_merge_workspace_bytes", "vghm_merge_tiles"}
    assert declared == want == set(_lib_merge.SYMBOLS)
    exported = _exported(_lib_merge.LIB_PATH)
    assert exported == want, exported ^ want  # hidden visibility: nothing of companion_host.h, no kernel stub
    assert not [s for s in exported if s.startswith(("vgh_", "vghv_", "vghvis_", "vghtex_", "vghev_"))]
    lib = _lib_merge.load()
    assert lib.vghm_version().startswith(b"vghmerge")
    for name, value in (("VGHM_MAX_CANDIDATES", _lib_merge.MAX_CANDIDATES), ("VGHM_MAX_HEADS", _lib_merge.MAX_HEADS), ("VGHM_METRIC_IOU", _lib_merge.METRICS["iou"]),
                        ("VGHM_METRIC_IOS", _lib_merge.METRICS["ios"]), ("VGHM_STATUS_ABSENT", 0), ("VGHM_STATUS_KEPT", 1), ("VGHM_STATUS_TRUNCATED", 2),
                        ("VGHM_STATUS_SUPPRESSED", 3), ("VGHM_STATUS_OVER_CAP", 4)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    fields = re.search(r"typedef struct vghm_merge_job \{(.*?)\} vghm_merge_job;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _lib_merge.MergeJob._fields_]  # the struct, field for field
    # sizes: the match mask dominates, 32 MiB at the capacity; invalid sizes give 0; argument errors come before anything touches a GPU
    assert 32 << 20 <= lib.vghm_merge_workspace_bytes(128, 128) < 34 << 20
    assert lib.vghm_merge_workspace_bytes(164, 100) == 0 and lib.vghm_merge_workspace_bytes(0, 5) == 0 and lib.vghm_merge_workspace_bytes(5, 0) == 0
    assert lib.vghm_merge_workspace_bytes(1, 1) % 16 == 0
    assert lib.vghm_merge_tiles(None, None, None) == -1 and b"null job" in lib.vghm_last_error()
    job = _lib_merge.MergeJob(164, 100, 640, 10, 0, 2.0, 0.5, 0)
    assert lib.vghm_merge_tiles(_lib_merge.C.byref(job), None, None) == -1 and b"16400" in lib.vghm_last_error()
    for (T, K, mh), words in (((1, 0, 10), b"keep_k"), ((1, 4, 0), b"max_heads"), ((0, 4, 10), b"n_tiles"), ((1, 4, 10), b"null boxes_dev")):
        job = _lib_merge.MergeJob(T, K, 640, mh, 0, 2.0, 0.5, 0)
        assert lib.vghm_merge_tiles(_lib_merge.C.byref(job), None, None) == -1 and words in lib.vghm_last_error(), lib.vghm_last_error()
    # the library is claimed in the build (the core's source scans read every unclaimed file of csrc/) with the flags its arithmetic needs
    from head_detector_amd import build

    mine = [c for c in build.COMPANIONS if c.lib == "libvghmerge.so"]
    assert len(mine) == 1 and mine[0].sources == ["slice_merge.hip"] and mine[0].headers == build.HOST_HEADERS
    assert "-ffp-contract=off" in mine[0].flags and mine[0].public == "vgh_merge.h"
    src = open(os.path.join(ROOT, "head_detector_amd", "csrc", "slice_merge.hip")).read()
    assert '#include "companion_host.h"' in src and "static_assert(VGHM_OK == OK && VGHM_ERR_INVALID == ERR_INVALID && VGHM_ERR_HIP == ERR_HIP && VGHM_ERR_NOMEM == ERR_NOMEM," in src
    for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "hipMalloc(", "set_error(const char", "g_error", "asm", "dlopen"):
        assert by_hand not in src, by_hand
