"""Host half of head tracking (head_detector_amd/tracking.py, include/vgh_track.h): the two forms of the restatement (tests/head_track_ref.py) against each other
on random tie-heavy sequences and on every planted case, every planted case against what it claims to contain, argument errors, and the ABI of libvghtrack.so.
No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_track_ref as ref  # noqa: E402

from head_detector_amd import _lib_track, tracking  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib_track.C


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def test_loop_form_equals_vectorised_form_on_random_tie_heavy_sequences():
    """A small image and an 8-pixel grid: the IoUs take few values, so the order's tie-breaks decide; table sizes on either side of the number of heads."""
    ties = births = frees = drops = second = 0
    for seed in range(10):
        M, K, live = [(3, 5, 4), (6, 8, 8), (16, 16, 12), (12, 24, 20), (40, 40, 30)][seed % 5]
        seq = ref.random_sequence(M, K, live, 6, seed, grid=8.0, width=128, height=96, head_px=(8.0, 24.0))
        rule = dict(min_hits=2, max_age=2, report_misses=1, box_gain=0.75, max_out=max(1, M - 2)) if seed % 2 else dict(min_hits=1, max_age=1, match_thr=0.2)
        a, b = ref.new_state(M), ref.new_state(M)
        for f in range(6):
            frame = [x[f] for x in seq]
            before = ref.copy_state(a)
            out_a, out_b = ref.step(a, *frame, "loop", **rule), ref.step(b, *frame, "vec", **rule)
            assert ref.same_bytes(out_a, out_b, ref.OUTPUTS) is None and ref.same_bytes(a, b, ref.STATE_FIELDS) is None, (seed, f)
            births, frees, drops = births + int(out_a["n_born"][0]), frees + int(out_a["n_freed"][0]), drops + int(out_a["n_dropped"][0])
            # the sequence is tie-heavy: some live slot sees two rows at the same positive IoU
            slots = np.flatnonzero(before["id"] >= 0)
            if len(slots):
                pred = (before["box"] + before["vel"]).astype(np.float32)
                det = ((np.fmin(np.fmax(frame[0], 0), 640) - np.tile(frame[4][:2], 2)) / frame[4][2]).astype(np.float32)[:max(0, min(int(frame[3]), K))]
                if len(det):
                    m = ref.iou_matrix(pred[slots], det)
                    ties += int(sum(len(row[row > 0]) != len(set(row[row > 0].tolist())) for row in m))
            low = (frame[1] < 0.5) & (frame[1] >= 0.1) & (np.arange(K) < frame[3])
            second += int((out_a["det_id"][low] >= 0).sum())
    assert ties > 20 and births > 50 and frees > 20 and drops > 5 and second > 5, (ties, births, frees, drops, second)


def test_planted_cases_hold_what_they_claim_in_both_forms():
    cases = ref.planted_cases()
    assert {"crossing", "score_dip", "low_never_gives_birth", "tentative_deleted_on_first_miss", "coasting_then_reuse", "table_full", "chain", "exact_ties",
            "counts_outside", "non_finite", "gains_of_one", "letterbox_and_cap"} <= set(cases)
    for name, c in cases.items():
        assert 2 <= len(c["counts"]) <= 8, name
        out, state = ref.run_case(c, "loop")
        out_v, state_v = ref.run_case(c, "vec")
        assert ref.same_bytes(out, out_v, ref.OUTPUTS) is None and ref.same_bytes(state, state_v, ref.STATE_FIELDS) is None, name
        c["claim"](out, state, lambda **kw: ref.run_case(c, **kw))
        assert state["frame"][0] == len(c["counts"]) and state["next_id"][0] == out["n_born"].sum(), name
        for f in range(len(c["counts"])):  # the rows behind n_out hold -1 / 0
            n = int(out["n_out"][f])
            assert (out["out_slot"][f, n:] == -1).all() and (out["out_id"][f, n:] == -1).all() and not out["out_box"][f, n:].any() and not out["out_params"][f, n:].any(), name


def test_one_call_of_b_frames_is_b_calls_of_one_frame_in_the_restatement():
    seq = ref.random_sequence(16, 16, 12, 5, seed=3)
    a, b = ref.new_state(16), ref.new_state(16)
    whole = ref.track(a, *seq, "vec", min_hits=1)
    parts = [ref.track(b, *[x[f:f + 1] for x in seq], "vec", min_hits=1) for f in range(5)]
    assert ref.same_bytes(whole, {k: np.concatenate([p[k] for p in parts]) for k in ref.OUTPUTS}, ref.OUTPUTS) is None and ref.same_bytes(a, b, ref.STATE_FIELDS) is None


# ---- Python argument errors -----------------------------------------------------------------------------------------------------------------------------------
def _state_stand_in(max_tracks=4):
    state = tracking.TrackState.__new__(tracking.TrackState)  # the checks come before anything touches the state's memory
    state.max_tracks, state.device = max_tracks, torch.device("cuda", 0)
    return state


def test_track_frames_argument_errors_need_no_gpu():
    state = _state_stand_in()
    b, s, p, c = torch.zeros(2, 4, 4), torch.zeros(2, 4), torch.zeros(2, 4, 413), torch.zeros(2, dtype=torch.int32)
    u = np.float32([[0, 0, 1], [0, 0, 1]])
    for kw, words in ((dict(high_thr=float("nan")), "high_thr"), (dict(match_thr_low=float("nan")), "match_thr_low"), (dict(box_gain=float("inf")), "box_gain"),
                      (dict(param_gain=float("nan")), "param_gain"), (dict(vel_gain="fast"), "vel_gain"), (dict(max_age=-1), "max_age"), (dict(min_hits=0), "min_hits"),
                      (dict(report_misses=0.5), "report_misses"), (dict(max_out=0), "max_out"), (dict(max_out=4096), "max_out"), (dict(image_size=0), "image_size"),
                      (dict(iou=0.5), "unknown rule parameter")):
        with pytest.raises(ValueError, match=words):
            tracking.track_frames(b, s, p, c, u, state, **kw)
    for args, words in (((b.double(), s, p, c, u), "boxes"), ((b, s, p, c.long(), u), "counts"), ((b.numpy(), s, p, c, u), "boxes"), ((b[:, :, :3], s, p, c, u), r"keep_k >= 1, 4"),
                        ((b, s[:, :3], p, c, u), "scores"), ((b, s, p[:, :, :400], c, u), "flame_params"), ((b, s, p, c[:1], u), "counts"), ((b, s, p, c, u[:1]), "unpad"),
                        ((b, s, p, c, np.float32([[0, 0, 1], [0, 0, 0]])), "unpad"), ((b, s, p, c, np.float32([[0, np.nan, 1], [0, 0, 1]])), "unpad"),
                        ((torch.zeros(1, 4096, 4), torch.zeros(1, 4096), torch.zeros(1, 4096, 413), c[:1], u[:1]), "exceed"), ((b, s, p, c, u), "GPU")):
        with pytest.raises(ValueError, match=words):
            tracking.track_frames(*args, state)
    with pytest.raises(ValueError, match="TrackState"):
        tracking.track_frames(b, s, p, c, u, None)
    for bad in (0, 4096, 2.5):
        with pytest.raises(ValueError, match="max_tracks"):
            tracking.TrackState(bad)
    with pytest.raises(ValueError, match="not a GPU"):
        tracking.TrackState(4, "cpu")
    assert tracking.check_rule("x", {}) == tracking.RULE_DEFAULTS == {k: ref.RULE[k] for k in tracking.RULE_DEFAULTS}  # the API defaults, on both sides


def test_tracker_rejects_a_frame_of_another_size_before_the_detector_runs():
    class Detector:  # what update_batch touches before the first device call
        _max_batch, _image_size, _device = 2, 640, torch.device("cuda", 0)

        @staticmethod
        def _convert_image(im):
            return im

    tracker = tracking.HeadTracker.__new__(tracking.HeadTracker)
    tracker.detector, tracker.rule, tracker._frame_shape = Detector, tracking.check_rule("t", {}), (48, 64)
    with pytest.raises(ValueError, match=r"reset\(\)"):
        tracker.update(np.zeros((50, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="max_batch"):
        tracker.update_batch([np.zeros((48, 64, 3), np.uint8)] * 3)
    with pytest.raises(ValueError, match="uint8"):
        tracker.update(np.zeros((48, 64, 3), np.float32))
    assert tracker.update_batch([]) == []
    with pytest.raises(ValueError, match="min_hits"):
        tracking.HeadTracker(None, min_hits=0)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return {ln.split()[-1] for ln in out if " T " in ln}


def _job(**over):
    """A job whose every pointer is set (to host memory that is never touched: the argument checks come first)."""
    spare = np.zeros(64, np.float32)
    fields = dict(n_frames=1, keep_k=4, max_tracks=4, image_size=640, max_out=4, max_age=30, min_hits=3, report_misses=0, high_thr=0.5, low_thr=0.1, match_thr=0.3,
                  match_thr_low=0.5, box_gain=1.0, vel_gain=0.5, param_gain=0.5, reserved=0)
    fields.update({name: spare.ctypes.data for name, kind in _lib_track.TrackJob._fields_ if kind is C.c_void_p})
    fields["unpad"] = np.float32([0, 0, 1] * 4).ctypes.data
    fields.update(over)
    job = _lib_track.TrackJob(**fields)
    job._keep = spare
    return job


def test_track_library_abi():
    hdr = open(os.path.join(ROOT, "include", "vgh_track.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vght_[a-z0-9_]+)\s*\(", code))
    want = {"vght_version", "vght_last_error", "vght_state_bytes", "vght_state_init", "vght_workspace_bytes", "vght_track_frames"}
    assert declared == want == set(_lib_track.SYMBOLS)
    exported = _exported(_lib_track.LIB_PATH)
    assert exported == want, exported ^ want  # hidden visibility: nothing of companion_host.h, no kernel stub
    lib = _lib_track.load()
    assert lib.vght_version().startswith(b"vghtrack")
    for name, value in (("VGHT_MAX_TRACKS", _lib_track.MAX_TRACKS), ("VGHT_MAX_DETS", _lib_track.MAX_DETS), ("VGHT_MAX_FRAMES", _lib_track.MAX_FRAMES),
                        ("VGHT_NUM_PARAMS", _lib_track.NUM_PARAMS), ("VGHT_STATE_HEADER_BYTES", _lib_track.STATE_HEADER_BYTES)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    assert (_lib_track.MAX_TRACKS, _lib_track.MAX_DETS, _lib_track.MAX_FRAMES, _lib_track.NUM_PARAMS) == (2048, 2048, 1024, 413)
    fields = re.search(r"typedef struct vght_track_job \{(.*?)\} vght_track_job;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _lib_track.TrackJob._fields_]  # the struct, field for field
    kinds = {"int32_t": C.c_int32, "float": C.c_float}
    assert [C.c_void_p if star else kinds[t] for t, star in re.findall(r"^\s*(?:const )?(\w+)(\*?) \w+;", fields, flags=re.M)] == [k for _, k in _lib_track.TrackJob._fields_]
    # sizes: 0 for invalid ones, multiples of 16, and the state's size is that of the documented layout
    for M in (1, 3, 64, 65, 130, 2048):
        assert lib.vght_state_bytes(M) == _lib_track.state_layout(M)["total"] and lib.vght_state_bytes(M) % 16 == 0
        assert all(v % 16 == 0 for v in _lib_track.state_layout(M).values())
        assert lib.vght_workspace_bytes(M, 7) % 16 == 0 and lib.vght_workspace_bytes(M, 7) >= 8 * M
    assert lib.vght_state_bytes(2048) >= 2048 * (6 * 4 + 32 + 413 * 4)
    assert lib.vght_state_bytes(0) == lib.vght_state_bytes(-1) == lib.vght_state_bytes(2049) == 0
    assert lib.vght_workspace_bytes(0, 4) == lib.vght_workspace_bytes(2049, 4) == lib.vght_workspace_bytes(4, 0) == lib.vght_workspace_bytes(4, 2049) == 0


def test_every_invalid_job_carries_its_message_and_needs_no_gpu():
    lib = _lib_track.load()
    mem = np.zeros(64, np.uint8)
    good = mem.ctypes.data + (-mem.ctypes.data) % 16

    def refused(job, words, state=good, ws=good):
        rc = lib.vght_track_frames(C.byref(job) if job is not None else None, state, ws, None)
        msg = lib.vght_last_error()
        assert rc == -1 and words in msg, (words, rc, msg)

    refused(None, b"null job")
    nan, inf = float("nan"), float("inf")
    for over, words in ((dict(n_frames=0), b"n_frames"), (dict(n_frames=1025), b"n_frames 1025 outside 1 .. 1024"), (dict(keep_k=0), b"keep_k"), (dict(keep_k=2049), b"keep_k 2049"),
                        (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=2049), b"max_tracks 2049"), (dict(image_size=0), b"image_size"), (dict(max_out=0), b"max_out"),
                        (dict(max_out=2049), b"max_out"), (dict(max_age=-1), b"max_age"), (dict(min_hits=0), b"min_hits"), (dict(report_misses=-1), b"report_misses"),
                        (dict(high_thr=nan), b"high_thr is NaN"), (dict(low_thr=nan), b"low_thr is NaN"), (dict(match_thr=nan), b"match_thr is NaN"),
                        (dict(match_thr_low=nan), b"match_thr_low is NaN"), (dict(box_gain=inf), b"box_gain"), (dict(vel_gain=nan), b"vel_gain"), (dict(param_gain=-inf), b"param_gain")):
        refused(_job(**over), words)
    for name, kind in _lib_track.TrackJob._fields_:
        if kind is C.c_void_p and name not in ("out_params_dev", "det_id_dev"):  # those two are optional
            refused(_job(**{name: None}), b"null " + name.encode())
    refused(_job(), b"null state", state=None)
    refused(_job(), b"null workspace", ws=None)
    refused(_job(), b"state is not 16-byte aligned", state=good + 4)
    refused(_job(), b"workspace is not 16-byte aligned", ws=good + 8)
    refused(_job(boxes_dev=good + 4), b"boxes_dev / out_box_dev")
    refused(_job(out_box_dev=good + 8), b"boxes_dev / out_box_dev")
    for row, f in (([0, 0, 0], 0), ([nan, 0, 1], 1), ([0, inf, 1], 0), ([0, 0, -1], 1)):
        table = np.float32([[0, 0, 1], [0, 0, 1]])
        table[f] = row
        refused(_job(n_frames=2, unpad=table.ctypes.data), b"frame %d: unpad" % f)
    assert lib.vght_state_init(None, 4, None) == -1 and b"null state" in lib.vght_last_error()
    assert lib.vght_state_init(good + 4, 4, None) == -1 and b"aligned" in lib.vght_last_error()
    assert lib.vght_state_init(good, 0, None) == -1 and b"max_tracks 0" in lib.vght_last_error()
    assert not mem.any()


def test_the_library_is_claimed_in_the_build():
    """The core's source scan reads every unclaimed file of csrc/; the flags are what the stated arithmetic needs."""
    from head_detector_amd import build

    mine = [c for c in build.COMPANIONS if c.lib == "libvghtrack.so"]
    assert len(mine) == 1 and mine[0] == build.Companion("libvghtrack.so", ["head_track.hip"], build.HOST_HEADERS, "vgh_track.h", ["-ffp-contract=off"], "build_track")
    assert len(build.COMPANIONS) == 6  # seven libraries with the core
    src = open(os.path.join(ROOT, "head_detector_amd", "csrc", "head_track.hip")).read()
    assert '#include "companion_host.h"' in src and "static_assert(VGHT_OK == OK && VGHT_ERR_INVALID == ERR_INVALID && VGHT_ERR_HIP == ERR_HIP && VGHT_ERR_NOMEM == ERR_NOMEM," in src
    assert "#pragma clang fp contract(off)" in src
    for by_hand in ("hipEventRecord(", "hipEventSynchronize(", "hipHostMalloc(", "hipMalloc(", "set_error(const char", "g_error", "asm", "dlopen", "atomicAdd(float", "fmaf("):
        assert by_hand not in src, by_hand
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert 'vght_version().startswith(b"vghtrack")' in entry
