"""Sliced detection on the MI355X: csrc/slice_merge.hip (libvghmerge.so) through ``head_detector_amd.sliced.merge_tiles`` against the NumPy restatement
tests/slice_merge_ref.py, and ``HeadDetector.detect_sliced`` against its recomputation by hand.  Every comparison is BITWISE: every float is a single IEEE
float32 operation in a stated order, the order of the candidates is a total order, so there is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slice_merge_ref as ref  # noqa: E402

from head_detector_amd import _lib, _lib_merge, sliced  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def gpu_merge(boxes, scores, counts, plan, **kw):
    out = sliced.merge_tiles(torch.from_numpy(boxes).to(_dev()), torch.from_numpy(scores).to(_dev()), torch.from_numpy(counts).to(_dev()), plan, want_status=True, **kw)
    torch.cuda.current_stream().synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in ref.OUTPUTS}


def same(got, want, what):
    bad = ref.same_bytes(got, want)
    if bad is not None:
        where = np.flatnonzero((np.asarray(got[bad]).reshape(-1) != np.asarray(want[bad]).reshape(-1)))
        raise AssertionError((what, bad, where[:8].tolist(), np.asarray(got[bad]).reshape(-1)[where[:8]].tolist(), np.asarray(want[bad]).reshape(-1)[where[:8]].tolist()))


_plans = {}


def plan_for(T):
    if T not in _plans:
        _plans[T] = {1: lambda: sliced.plan_slices(64, 64, 64), 2: lambda: sliced.plan_slices(64, 100, 64, include_full=False), 5: ref.small_plan,
                     49: lambda: sliced.plan_slices(3000, 4000, 640)}[T]()
        assert _plans[T].n_tiles == T
    return _plans[T]


SIZES = [(1, 1, 0), (1, 1, 1), (2, 8, 0), (2, 8, 1), (2, 8, 16), (5, 13, 0), (5, 13, 1), (5, 13, 63), (5, 13, 64), (5, 13, 65)] + \
        [(49, 100, n) for n in (0, 1, 63, 64, 65, 1024, 1025, 4096, 4097, 4900)]


@pytest.mark.parametrize("T,keep_k,n_live", SIZES)
def test_merge_equals_the_restatement_on_seeded_crowds(gpu_lib, T, keep_k, n_live):
    """Live candidate counts on either side of a wave, of the core NMS limit of 1 024 and of one LDS tile of the rank pass (4 096), up to every slot taken."""
    plan = plan_for(T)
    boxes, scores, counts = ref.random_family(plan, keep_k, n_live, seed=1000 * T + n_live, head_px=(12.0, 60.0) if T == 49 else (8.0, 30.0))
    assert int(counts.sum()) == n_live
    want = ref.merge_vec(boxes, scores, counts, plan)
    got = gpu_merge(boxes, scores, counts, plan)
    same(got, want, (T, keep_k, n_live))
    if n_live >= 1024:  # the comparison is not over an empty case
        assert {1, 2, 3} <= set(want["status"].tolist())
    if n_live >= 4096:  # more kept than the default max_heads
        assert int(want["n_heads"][0]) == 1000 < int(want["n_kept_uncapped"][0]) and 4 in want["status"]
    if n_live == 4900:
        assert not (want["status"] == 0).any()


@pytest.mark.parametrize("name", sorted(ref.planted_cases()))
def test_merge_equals_the_restatement_on_planted_cases(gpu_lib, name):
    """Chains across three tiles (the kept-only rule), pairs of one tile, equal scores and identical boxes, a pair exactly at the threshold, zero-area boxes, IoS with
    a nested box, boxes exactly on the border threshold on each side and on a non-interior edge, everything dropped, the cap, non-finite values.  What each case
    must contain is asserted on the restatement by tests/test_sliced_host.py."""
    c = ref.planted_cases()[name]
    want = ref.merge_loop(c["boxes"], c["scores"], c["counts"], c["plan"], **c["kwargs"])
    got = gpu_merge(c["boxes"], c["scores"], c["counts"], c["plan"], **c["kwargs"])
    same(got, want, name)
    if c["expect"] is not None:
        assert [int(got["status"][r]) for r in c["rows"]] == c["expect"]


def test_empty_tiles_cap_repeat_and_stream(gpu_lib):
    plan = plan_for(49)
    boxes, scores, counts = ref.random_family(plan, 100, 1025, seed=5)
    counts[::3] = 0  # tiles without a detection, the whole image among them
    for kw in (dict(), dict(max_heads=100), dict(metric="ios", match_thr=0.3, border=8.0, max_heads=7)):
        want = ref.merge_vec(boxes, scores, counts, plan, **kw)
        got = gpu_merge(boxes, scores, counts, plan, **kw)
        same(got, want, kw)
        again = gpu_merge(boxes, scores, counts, plan, **kw)  # two calls, equal bytes
        same(again, got, ("again", kw))
        if "max_heads" in kw:
            assert int(got["n_heads"][0]) == kw["max_heads"] < int(got["n_kept_uncapped"][0]) and int((got["status"] == 4).sum()) == int(got["n_kept_uncapped"][0]) - kw["max_heads"]
    assert (want["status"].reshape(49, 100)[::3] == 0).all()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = gpu_merge(boxes, scores, counts, plan)
    same(got, ref.merge_vec(boxes, scores, counts, plan), "side stream")


def test_invalid_jobs_return_before_anything_runs(gpu_lib):
    """T * keep_k = 16 400 is above the capacity: ERR_INVALID, and no output is touched; so for a misaligned workspace."""
    lib = _lib_merge.load()
    T, K, mh = 164, 100, 16
    i32, f32 = dict(dtype=torch.int32, device=_dev()), dict(dtype=torch.float32, device=_dev())
    boxes, scores, counts = torch.rand(T, K, 4, **f32) * 600, torch.rand(T, K, **f32), torch.full((T,), K, **i32)
    tiles = np.tile(np.int32([0, 0, 640, 640, 0, 0, 640, 640]), (T, 1))
    scale, interior = np.ones(T, np.float32), np.zeros(T, np.uint8)
    outs = [torch.full((mh,), 77, **i32), torch.full((mh,), 77, **i32), torch.full((mh, 4), 77.0, **f32), torch.full((mh,), 77.0, **f32), torch.full((1,), 77, **i32),
            torch.full((1,), 77, **i32)]
    ws = torch.zeros(40 << 20, dtype=torch.uint8, device=_dev())

    def call(n_tiles, ws_ptr):
        job = _lib_merge.MergeJob(n_tiles, K, 640, mh, 0, 2.0, 0.5, 0, boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), tiles.ctypes.data, scale.ctypes.data,
                                  interior.ctypes.data, *[o.data_ptr() for o in outs], None)
        return lib.vghm_merge_tiles(C.byref(job), ws_ptr, torch.cuda.current_stream().cuda_stream), lib.vghm_last_error().decode()

    rc, msg = call(T, ws.data_ptr())
    assert rc == -1 and "16400" in msg and "16384" in msg, msg
    rc, msg = call(4, ws.data_ptr() + 8)
    assert rc == -1 and "aligned" in msg, msg
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in outs) and not bool(ws.any())
    with pytest.raises(_lib.VghError, match="16400"):
        sliced.merge_tiles(boxes, scores, counts, sliced.SlicePlan(640, 640, 640, tiles, scale, interior, np.zeros((T, 3), np.float32)))
    rc, msg = call(4, ws.data_ptr())  # the same job within the capacity runs
    torch.cuda.synchronize()
    assert rc == 0 and K <= int(outs[5][0]) <= 4 * K and int(outs[4][0]) == mh  # no interior edge: nothing is dropped, and one tile's own candidates all stay


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd(gpu_lib, flame_model):
    """One detector, one seeded 900 x 1300 photograph (6 tiles + the whole image: two chunks of max_batch = 4), and a confidence threshold taken from a score
    of the run, so that every tile yields candidates."""
    import warnings

    from head_detector_amd.detector import HeadDetector

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        det = HeadDetector("vgg_heads_m", weights="synthetic", max_batch=4, flame_model=flame_model)
    image = np.random.default_rng(7).integers(0, 256, (900, 1300, 3), dtype=np.uint8)
    plan = sliced.plan_slices(900, 1300, 640)
    assert plan.n_tiles == 7
    photo = torch.from_numpy(image).to(_dev())
    views = [photo[y:y + h, x:x + w] for x, y, w, h in plan.tiles[:, :4].tolist()]
    conf = min(float(det.model.model(views[at:at + 4])[1][:, 10, 0].min()) for at in (0, 4))  # the 11th best score of the weakest tile
    return det, image, photo, views, plan, conf


def _slabs_by_hand(det, views, conf):
    parts = [det.model.detect(views[at:at + 4], confidence_threshold=conf, flame=None) for at in (0, 4)]
    return [torch.cat([getattr(p, f) for p in parts]) for f in ("boxes", "scores", "flame_params", "counts")]


def test_detect_sliced_equals_its_recomputation(crowd):
    det, image, photo, views, plan, conf = crowd
    result, info = det.detect_sliced(image, conf, return_info=True)
    boxes, scores, params, counts = _slabs_by_hand(det, views, conf)
    want = ref.merge_vec(boxes.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy(), plan)
    n = int(want["n_heads"][0])
    assert n >= 1 and int((counts > 0).sum()) >= 2, "no candidate survived: the comparison would be empty"
    merged = sliced.merge_tiles(boxes, scores, counts, plan, want_status=True)
    same({k: getattr(merged, k).cpu().numpy() for k in ref.OUTPUTS}, want, "merge of the real slabs")
    assert len(result.heads) == n and np.array_equal(info.plan.tiles, plan.tiles) and np.array_equal(info.head_tile, want["head_tile"][:n])
    assert info.status_counts == {name: int((want["status"] == s).sum()) for s, name in enumerate(sliced.STATUS_NAMES)} and info.n_kept_uncapped == int(want["n_kept_uncapped"][0])
    bb = np.rint(want["boxes_full"][:n]).astype(int)
    part = want["head_tile"][:n] != 0  # clipped to the image, but for the heads of the whole-image tile: those keep __call__'s box (sliced.image_boxes)
    bb[part] = bb[part].clip(0, [1300, 900, 1300, 900])
    assert (bb[part] >= 0).all() and part.any()
    rows, tile_of = torch.from_numpy(want["head_row"][:n]).long().to(_dev()), torch.from_numpy(want["head_tile"][:n]).long()
    P = det.model.program
    survivors = params.view(-1, params.shape[-1])[rows]
    _, _, verts = det._flame.decode(survivors, unpad=torch.from_numpy(plan.unpad)[tile_of].to(_dev()), shape_live=P.shape_c, expr_live=P.expr_c, want_vertices=False)
    verts, survivors = verts.cpu().numpy(), survivors.cpu()
    for i, head in enumerate(result.heads):
        assert (head.bbox.x, head.bbox.y, head.bbox.x + head.bbox.w, head.bbox.y + head.bbox.h) == tuple(bb[i])
        assert np.float32(head.score).tobytes() == want["scores"][i].tobytes()
        assert head.vertices_3d.tobytes() == verts[i].tobytes()  # the same kernel on the same inputs and head count
        tr, sc = sliced.to_whole_image_params(survivors[i:i + 1, 409:412].clone(), survivors[i:i + 1, 412:413], plan.tiles[tile_of[i]], 900, 1300, 640)
        assert torch.equal(head.flame_params.translation, tr) and torch.equal(head.flame_params.scale, sc)
        assert torch.equal(head.flame_params.shape, survivors[i:i + 1, :300]) and torch.equal(head.flame_params.rotation, survivors[i:i + 1, 403:409])
    # un-padded with its own tile's row, a head's mesh lies where its box is: the projected vertices of a tile head are in image coordinates
    assert len({int(t) for t in info.head_tile}) >= 2


def test_whole_image_plan_reproduces_call(crowd):
    det, image, _, _, _, conf = crowd
    plain = det(image, confidence_threshold=conf)
    only, info = det.detect_sliced(image, conf, tile_sizes=(), include_full=True, return_info=True)
    assert info.plan.n_tiles == 1 and len(plain.heads) == len(only.heads) >= 1
    assert info.status_counts["truncated"] == info.status_counts["suppressed"] == 0
    for a, b in zip(plain.heads, only.heads):
        assert (a.bbox.x, a.bbox.y, a.bbox.w, a.bbox.h) == (b.bbox.x, b.bbox.y, b.bbox.w, b.bbox.h)
        assert np.float32(a.score).tobytes() == np.float32(b.score).tobytes()
        assert np.array_equal(a.vertices_3d, b.vertices_3d)
        assert torch.equal(a.flame_params.to_3dmm_tensor(), b.flame_params.to_3dmm_tensor())
        assert tuple(a.head_pose) == tuple(b.head_pose)


def test_scale_one_tiles_reach_the_network_as_the_photographs_bytes(crowd):
    det, image, photo, _, plan, conf = crowd
    det.detect_sliced(image, conf)
    torch.cuda.synchronize()
    canvas = det.model.raw_canvas()
    last = plan.tiles[4:]  # the second chunk: tiles 4, 5, 6, all 640 x 640 at scale 1
    assert len(last) == 3 and (last[:, 2:] == [640, 640, 0, 0, 640, 640]).all() and det.model.arena_batch == 4
    for i, (x, y, w, h) in enumerate(last[:, :4].tolist()):
        assert torch.equal(canvas[i], photo[y:y + h, x:x + w]), (i, x, y)
