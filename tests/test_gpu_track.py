"""Head tracking on the MI355X: csrc/head_track.hip (libvghtrack.so) through ``head_detector_amd.tracking`` against the NumPy restatement tests/head_track_ref.py,
and ``HeadTracker`` against its recomputation by hand.  Every comparison is BITWISE, the state included: every float is a single IEEE float32 operation in a
stated order and every choice follows a total order, so there is no tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_track_ref as ref  # noqa: E402

from head_detector_amd import _lib, _lib_track, tracking  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = dict(n_out="n_out", out_slot="slot", out_id="ids", out_det_row="det_row", out_hits="hits", out_misses="misses", out_box="boxes", out_score="scores",
              out_params="params", det_id="det_id", n_born="n_born", n_freed="n_freed", n_dropped="n_dropped")  # the restatement's names -> TrackedFrames'
STATE = dict(next_id="next_id", frame="frame", id="ids", hits="hits", misses="misses", age="age", det_row="det_row", score="scores", box="boxes", vel="vel", params="params")


def _dev():
    return torch.device("cuda", 0)


def gpu_track(state, seq, frames=slice(None), **rule):
    boxes, scores, flame, counts, unpad = (x[frames] for x in seq)
    out = tracking.track_frames(*(torch.from_numpy(np.ascontiguousarray(x)).to(_dev()) for x in (boxes, scores, flame, counts)), unpad, state, **rule)
    torch.cuda.current_stream().synchronize()
    return {k: getattr(out, name).cpu().numpy() for k, name in FIELDS.items()}


def state_of(state):
    return {k: getattr(state, name).cpu().numpy() for k, name in STATE.items()}


def same(got, want, keys, what):
    bad = ref.same_bytes(got, want, keys)
    if bad is not None:
        g, w = np.asarray(got[bad]).reshape(-1), np.asarray(want[bad]).reshape(-1)
        where = np.flatnonzero(g.view(np.int32) != w.view(np.int32)) if g.shape == w.shape else []
        raise AssertionError((what, bad, g.shape, w.shape, where[:8].tolist(), g[where[:8]].tolist(), w[where[:8]].tolist()))


SIZES = [(1, 1, 1), (3, 5, 4), (64, 64, 64), (65, 63, 60), (130, 200, 150), (2048, 2048, 300)]


@pytest.mark.parametrize("max_tracks,keep_k,live", SIZES)
def test_equals_the_restatement_after_every_frame(gpu_lib, max_tracks, keep_k, live):
    """Seeded videos of 6 frames, one call per frame, outputs and state compared after each: one slot and one row, fewer slots than heads, a whole wave, one more
    than a wave with fewer rows than slots, several waves with more rows than slots, and the capacity (with the vectorised restatement)."""
    M, K = max_tracks, keep_k
    seq = ref.random_sequence(M, K, live, 6, seed=7 * M + K)
    rule = dict(min_hits=2, max_age=1, report_misses=1, box_gain=0.75, vel_gain=0.5, param_gain=0.25)
    if M == 65:
        rule["max_out"] = 20  # fewer rows than reported tracks
    if M == 1:
        rule["min_hits"] = 1  # one row per frame, often not the head's: nothing would reach a second hit
    form = "vec" if M == 2048 else "loop"
    want_state, state = ref.new_state(M), tracking.TrackState(M, _dev())
    same(state_of(state), want_state, ref.STATE_FIELDS, "the initial state")
    seen = np.zeros(4, np.int64)
    for f in range(6):
        want = ref.track(want_state, *[x[f:f + 1] for x in seq], form, **rule)
        got = gpu_track(state, seq, slice(f, f + 1), **rule)
        same(got, want, ref.OUTPUTS, ("outputs", f))
        same(state_of(state), want_state, ref.STATE_FIELDS, ("state", f))
        seen += [int(want[k][0]) for k in ("n_out", "n_born", "n_freed", "n_dropped")]
    assert seen[0] > 0 and seen[1] > 0 and want_state["frame"][0] == 6  # the comparison is not over an empty case
    if live > 4:
        assert seen[2] > 0 and (want["out_misses"] > 0).any() and (want_state["hits"] > 2).any()
    if M == 3:  # fewer slots than confident detections
        assert seen[3] > 0
    if M == 65:
        assert int((want_state["hits"] >= 2).sum()) > 20 == int(want["n_out"][0])


@pytest.mark.parametrize("name", sorted(ref.planted_cases()))
def test_equals_the_restatement_on_planted_cases(gpu_lib, name):
    """Every planted sequence in ONE call: crossing heads, a score dip carried by stage 2, a LOW detection that never gives birth, a tentative track deleted on its
    first miss, coasting up to max_age and the slot reused in the same frame, a full table, the chain of N + 1 rounds, exact IoU ties, counts of 0 and above keep_k,
    non-finite values, gains of exactly 1.  What each case must contain is asserted on the restatement by tests/test_track_host.py and here on the device's output."""
    c = ref.planted_cases()[name]
    want, want_state = ref.run_case(c, "loop")
    state = tracking.TrackState(c["max_tracks"], _dev())
    got = gpu_track(state, [c[k] for k in ("boxes", "scores", "flame", "counts", "unpad")], **c["rule"])
    same(got, want, ref.OUTPUTS, name)
    same(state_of(state), want_state, ref.STATE_FIELDS, name)
    c["claim"](got, state_of(state), lambda **kw: ref.run_case(c, **kw))


def test_one_call_of_five_frames_equals_five_calls_of_one(gpu_lib):
    """On a non-default stream, twice: equal bytes every time, and equal to the restatement."""
    M, K = 130, 200
    seq = ref.random_sequence(M, K, 150, 5, seed=11)
    rule = dict(min_hits=1, max_age=2, report_misses=2, box_gain=0.5)
    want_state = ref.new_state(M)
    want = ref.track(want_state, *seq, "vec", **rule)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs = []
        for _ in range(2):
            whole_state, parts_state = tracking.TrackState(M, _dev()), tracking.TrackState(M, _dev())
            whole = gpu_track(whole_state, seq, **rule)
            parts = [gpu_track(parts_state, seq, slice(f, f + 1), **rule) for f in range(5)]
            parts = {k: np.concatenate([p[k] for p in parts]) for k in ref.OUTPUTS}
            same(whole, parts, ref.OUTPUTS, "one call against five")
            same(state_of(whole_state), state_of(parts_state), ref.STATE_FIELDS, "one call against five: state")
            runs.append((whole, state_of(whole_state)))
        same(runs[0][0], runs[1][0], ref.OUTPUTS, "again")
        same(runs[0][1], runs[1][1], ref.STATE_FIELDS, "again: state")
    same(runs[0][0], want, ref.OUTPUTS, "restatement")
    same(runs[0][1], want_state, ref.STATE_FIELDS, "restatement: state")
    # reset() gives the initial state back
    whole_state.reset()
    torch.cuda.synchronize()
    same(state_of(whole_state), ref.new_state(M), ref.STATE_FIELDS, "reset")


def test_invalid_jobs_return_before_anything_runs(gpu_lib):
    """n_frames above the capacity, a NaN threshold, a bad unpad row and a misaligned workspace: ERR_INVALID, and neither the state nor an output is touched."""
    lib = _lib_track.load()
    M, K, B = 8, 8, 2
    seq = ref.random_sequence(M, K, 6, B, seed=1)
    dev_in = [torch.from_numpy(x).to(_dev()) for x in seq[:4]]
    state = tracking.TrackState(M, _dev())
    tracking.track_frames(*dev_in, seq[4], state, min_hits=1)  # a state that is not the initial one
    torch.cuda.synchronize()
    before = state.buffer.clone()
    i32, f32 = dict(dtype=torch.int32, device=_dev()), dict(dtype=torch.float32, device=_dev())
    outs = [torch.full((B,), 77, **i32)] + [torch.full((B, M), 77, **i32) for _ in range(5)] + [torch.full((B, M, 4), 77.0, **f32), torch.full((B, M), 77.0, **f32),
                                                                                               torch.full((B, M, 413), 77.0, **f32), torch.full((B, K), 77, **i32)] + \
           [torch.full((B,), 77, **i32) for _ in range(3)]
    ws = torch.zeros(4096, dtype=torch.uint8, device=_dev())
    table = np.ascontiguousarray(seq[4])

    def call(n_frames=B, high_thr=0.5, ws_ptr=None, unpad=table):
        job = _lib_track.TrackJob(n_frames, K, M, 640, M, 30, 1, 0, high_thr, 0.1, 0.3, 0.5, 1.0, 0.5, 0.5, 0, *[t.data_ptr() for t in dev_in], unpad.ctypes.data,
                                  *[o.data_ptr() for o in outs])
        return lib.vght_track_frames(C.byref(job), state.buffer.data_ptr(), ws.data_ptr() if ws_ptr is None else ws_ptr, torch.cuda.current_stream().cuda_stream), \
            lib.vght_last_error().decode()

    for kw, words in ((dict(n_frames=1025), "1025"), (dict(high_thr=float("nan")), "high_thr is NaN"), (dict(ws_ptr=ws.data_ptr() + 8), "aligned"),
                      (dict(unpad=np.float32([[0, 0, 1], [0, 0, 0]])), "frame 1: unpad")):
        rc, msg = call(**kw)
        assert rc == -1 and words in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(state.buffer, before) and all(bool((o == 77).all()) for o in outs) and not bool(ws.any())
    with pytest.raises(_lib.VghError, match="aligned"):
        _lib_track.check(call(ws_ptr=ws.data_ptr() + 4)[0])
    rc, msg = call()  # the same job, valid, runs
    torch.cuda.synchronize()
    assert rc == 0 and not torch.equal(state.buffer, before) and int(state.frame[0]) == 2 * B and not bool((outs[0] == 77).any())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def video(gpu_lib, flame_model):
    """One detector of max_batch 3, one seeded 480 x 600 frame and the two thresholds taken from the scores of the run (as smoke() takes its own): the 11th best
    score is HIGH, the 31st LOW."""
    import warnings

    from head_detector_amd.detector import HeadDetector

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        det = HeadDetector("vgg_heads_m", weights="synthetic", max_batch=3, flame_model=flame_model)
    frame = np.random.default_rng(5).integers(0, 256, (480, 600, 3), dtype=np.uint8)
    scores = det.model.model([torch.from_numpy(frame).to(_dev())])[1][0, :, 0]
    return det, frame, float(scores[10]), float(scores[30])


def test_tracker_end_to_end(video):
    from head_detector_amd.letterbox import geometry

    det, frame, high, low = video
    rule = dict(high_thr=high, low_thr=low, min_hits=1, param_gain=0.5, box_gain=0.75)
    one = tracking.HeadTracker(det, max_tracks=64, **rule)
    singles, frames_single = [], []
    for _ in range(3):
        singles.append(one.update(frame))
        frames_single.append(one.last_frames)
    many = tracking.HeadTracker(det, max_tracks=64, **rule)
    batch = many.update_batch([frame, frame, frame])
    # the restatement, fed with engine.detect's slabs
    raw = [torch.from_numpy(frame).to(_dev())] * 3
    slabs = det.model.detect(raw, confidence_threshold=low, flame=None)
    _, _, pad_x, pad_y, scale = geometry(480, 600, 640)
    unpad = np.tile(np.float32([pad_x, pad_y, scale]), (3, 1))
    want_state = ref.new_state(64)
    want = ref.track(want_state, slabs.boxes.cpu().numpy(), slabs.scores.cpu().numpy(), slabs.flame_params.cpu().numpy(), slabs.counts.cpu().numpy(), unpad, "vec",
                     image_size=640, **rule)
    count = int(slabs.counts[0])
    n = int((slabs.scores[0, :count] >= high).sum())
    assert 1 <= n < count, "no HIGH or no LOW detection: the comparison would be empty"
    got = {k: getattr(many.last_frames, name).cpu().numpy() for k, name in FIELDS.items()}
    same(got, want, ref.OUTPUTS, "update_batch against the restatement")
    same(state_of(many.state), want_state, ref.STATE_FIELDS, "state")
    same(state_of(one.state), want_state, ref.STATE_FIELDS, "state of three updates")
    for f in range(3):
        same({k: getattr(frames_single[f], name).cpu().numpy() for k, name in FIELDS.items()}, {k: want[k][f:f + 1] for k in ref.OUTPUTS}, ref.OUTPUTS, ("update", f))
    # ids 0 .. n - 1 in ascending detection row in frame 1, unchanged afterwards
    high_rows = np.flatnonzero(slabs.scores[0, :count].cpu().numpy() >= np.float32(high))
    for f in range(3):
        for res in (singles[f], batch[f]):
            assert isinstance(res, tracking.TrackedPredictionResult) and len(res.heads) == n
            assert res.track_ids.tolist() == list(range(n)) and res.track_ids.dtype == np.int64 and res.hits.tolist() == [f + 1] * n and not res.coasting.any()
        assert want["out_det_row"][f, :n].tolist() == high_rows.tolist()
    # heads: rint of the smoothed box clipped to the image, FlameParams of the smoothed vector, vertices of ONE decode of all reported tracks
    P = det.model.program
    rows = torch.from_numpy(np.repeat(unpad, n, axis=0)).to(_dev())
    smoothed = torch.from_numpy(np.concatenate([want["out_params"][f, :n] for f in range(3)])).to(_dev())
    _, _, verts = det._flame.decode(smoothed, unpad=rows, shape_live=P.shape_c, expr_live=P.expr_c, want_vertices=False)
    for f in range(3):
        bb = np.rint(want["out_box"][f, :n]).astype(int).clip(0, [600, 480, 600, 480])
        for i, head in enumerate(batch[f].heads):
            assert (head.bbox.x, head.bbox.y, head.bbox.x + head.bbox.w, head.bbox.y + head.bbox.h) == tuple(bb[i])
            assert np.float32(head.score).tobytes() == want["out_score"][f, i].tobytes()
            assert torch.equal(torch.from_numpy(head.vertices_3d), verts[f * n + i].cpu())  # the same kernel on the same inputs in the same call shape
            p = torch.from_numpy(want["out_params"][f, i:i + 1])
            assert torch.equal(head.flame_params.shape, p[:, :300]) and torch.equal(head.flame_params.rotation, p[:, 403:409])
            assert torch.equal(head.flame_params.translation, p[:, 409:412]) and torch.equal(head.flame_params.scale, p[:, 412:413] / scale)
            other = singles[f].heads[i]  # update() decodes n heads at a time, not 3 n: everything but the vertices is equal bit for bit
            assert (other.bbox.x, other.bbox.y, other.bbox.w, other.bbox.h) == (head.bbox.x, head.bbox.y, head.bbox.w, head.bbox.h) and other.vertices_3d.shape == head.vertices_3d.shape
            assert torch.equal(other.flame_params.to_3dmm_tensor(), head.flame_params.to_3dmm_tensor()) and tuple(other.head_pose) == tuple(head.head_pose)
    # a frame of another size needs reset()
    with pytest.raises(ValueError, match=r"reset\(\)"):
        one.update(frame[:400])
    one.reset()
    again = one.update(frame[:400])
    assert again.track_ids.tolist() == list(range(len(again.heads))) and int(one.state.frame[0]) == 1
