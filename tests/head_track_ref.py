"""NumPy restatement of the head-tracking rule (include/vgh_track.h) and a generator of planted sequences for the tests.  Not a test module.

Two forms of the association, everything else shared: ``form="loop"`` is literal -- every pair's IoU one scalar float32 operation at a time, the pairs above
the threshold sorted by (iou descending, slot ascending, row ascending), a sequential greedy walk; ``form="vec"`` computes the IoU matrix with array operations
and matches in rounds of mutual best choice (what the device does).  Every operation is float32, rounded on its own."""
import numpy as np

F = np.float32
NP_ = 413
STATE_FIELDS = ("next_id", "frame", "id", "hits", "misses", "age", "det_row", "score", "box", "vel", "params")
OUTPUTS = ("n_out", "out_slot", "out_id", "out_det_row", "out_hits", "out_misses", "out_box", "out_score", "out_params", "det_id", "n_born", "n_freed", "n_dropped")
RULE = dict(image_size=640, high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, max_age=30, min_hits=3, report_misses=0, box_gain=1.0, vel_gain=0.5,
            param_gain=0.5, max_out=None)  # the API defaults; max_out None = max_tracks
LAST_ROUNDS = []  # rounds of every stage of the last ``form="vec"`` step, the final round that matches nothing included


def new_state(max_tracks: int) -> dict:
    M = max_tracks
    return dict(next_id=np.zeros(1, np.int32), frame=np.zeros(1, np.int32), id=np.full(M, -1, np.int32), hits=np.zeros(M, np.int32), misses=np.zeros(M, np.int32),
                age=np.zeros(M, np.int32), det_row=np.full(M, -1, np.int32), score=np.zeros(M, F), box=np.zeros((M, 4), F), vel=np.zeros((M, 4), F),
                params=np.zeros((M, NP_), F))


def copy_state(state: dict) -> dict:
    return {k: v.copy() for k, v in state.items()}


def same_bytes(a: dict, b: dict, keys):
    """None if every named array of the two dicts is bytewise equal, else the name of the first that differs."""
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


# ---- similarity ---------------------------------------------------------------------------------------------------------------------------------------------
def iou_scalar(a, b):
    area_a = F(np.fmax(F(0), F(a[2] - a[0])) * np.fmax(F(0), F(a[3] - a[1])))
    area_b = F(np.fmax(F(0), F(b[2] - b[0])) * np.fmax(F(0), F(b[3] - b[1])))
    w = np.fmax(F(0), F(np.fmin(a[2], b[2]) - np.fmax(a[0], b[0])))
    h = np.fmax(F(0), F(np.fmin(a[3], b[3]) - np.fmax(a[1], b[1])))
    inter = F(w * h)
    return F(inter / F(F(area_a + area_b) - inter))


def iou_matrix(a, b):
    """a [n, 4], b [m, 4] float32 -> [n, m] float32, the operations of ``iou_scalar`` elementwise."""
    area_a = np.fmax(F(0), a[:, 2] - a[:, 0]) * np.fmax(F(0), a[:, 3] - a[:, 1])
    area_b = np.fmax(F(0), b[:, 2] - b[:, 0]) * np.fmax(F(0), b[:, 3] - b[:, 1])
    w = np.fmax(F(0), np.fmin(a[:, None, 2], b[None, :, 2]) - np.fmax(a[:, None, 0], b[None, :, 0]))
    h = np.fmax(F(0), np.fmin(a[:, None, 3], b[None, :, 3]) - np.fmax(a[:, None, 1], b[None, :, 1]))
    inter = w * h
    with np.errstate(all="ignore"):
        out = inter / ((area_a[:, None] + area_b[None, :]) - inter)
    assert out.dtype == F
    return out


def match_loop(pred, slots, det, rows, thr):
    """The greedy matching, literally: {slot: row}."""
    pairs = []
    for s in slots:
        for r in rows:
            iou = iou_scalar(pred[s], det[r])
            if iou > thr:  # False for NaN
                pairs.append((-float(iou), int(s), int(r)))
    pairs.sort()
    match, taken = {}, set()
    for _, s, r in pairs:
        if s not in match and r not in taken:
            match[s] = r
            taken.add(r)
    return match


def match_vec(pred, slots, det, rows, thr):
    """The same matching as rounds of mutual best choice; appends the number of rounds to LAST_ROUNDS."""
    slots, rows = np.asarray(slots, np.int64), np.asarray(rows, np.int64)
    match, rounds = {}, 0
    if len(slots) and len(rows):
        iou = iou_matrix(pred[slots], det[rows])
        val = np.where(iou > thr, iou, F(-1))  # an iou is never negative
        free_s, free_r = np.ones(len(slots), bool), np.ones(len(rows), bool)
        while True:
            rounds += 1
            v = np.where(free_s[:, None] & free_r[None, :], val, F(-1))
            sp, rp = v.argmax(1), v.argmax(0)  # the first maximum: the lowest row, the lowest slot
            at = np.arange(len(slots))
            mutual = (v[at, sp] >= 0) & (rp[sp] == at)
            if not mutual.any():
                break
            for i in np.flatnonzero(mutual):
                match[int(slots[i])] = int(rows[sp[i]])
            free_r[sp[mutual]] = False
            free_s[mutual] = False
    else:
        rounds = 1
    LAST_ROUNDS.append(rounds)
    return match


# ---- one frame ----------------------------------------------------------------------------------------------------------------------------------------------
def _smooth(old, new, gain):
    return new.copy() if gain == F(1) else (old + gain * (new - old)).astype(F)


def step(state: dict, boxes, scores, flame, count, unpad, form="loop", **rule) -> dict:
    """Steps ``state`` (in place) through one frame: boxes [K, 4], scores [K], flame [K, 413], count an integer, unpad (pad_x, pad_y, scale).  -> the frame's
    outputs, named like the fields of vght_track_job without ``_dev``."""
    R = dict(RULE, **rule)
    boxes, scores, flame = np.asarray(boxes, F), np.asarray(scores, F), np.asarray(flame, F)
    K, M = scores.shape[0], state["id"].shape[0]
    max_out = M if R["max_out"] is None else int(R["max_out"])
    S, pad_x, pad_y, scale = F(R["image_size"]), F(unpad[0]), F(unpad[1]), F(unpad[2])
    gains = {k: F(R[k]) for k in ("box_gain", "vel_gain", "param_gain")}
    if form == "vec":
        LAST_ROUNDS.clear()
    with np.errstate(all="ignore"):
        # 1. detections
        n_det = min(max(int(count), 0), K)
        c = np.fmin(np.fmax(boxes, F(0)), S)
        det = ((c - np.array([pad_x, pad_y, pad_x, pad_y], F)) / scale).astype(F)
        exists = np.arange(K) < n_det
        high = exists & (scores >= F(R["high_thr"]))
        low = exists & ~high & (scores >= F(R["low_thr"]))
        # 2. predict
        live = state["id"] >= 0
        pred = (state["box"] + state["vel"]).astype(F)
        fresh = state["misses"] == 0
        # 3, 4. association
        matcher = match_loop if form == "loop" else match_vec
        match = matcher(pred, np.flatnonzero(live), det, np.flatnonzero(high), F(R["match_thr"]))
        taken = set(match.values())
        second = matcher(pred, [s for s in np.flatnonzero(live & fresh) if s not in match], det, np.flatnonzero(low), F(R["match_thr_low"]))
        match.update(second)
        taken |= set(second.values())
        det_id = np.full(K, -1, np.int32)
        n_freed = 0
        for s in np.flatnonzero(live):
            if s in match:  # 5. matched
                r = match[s]
                nb = _smooth(pred[s], det[r], gains["box_gain"])
                state["vel"][s] = _smooth(state["vel"][s], (nb - state["box"][s]).astype(F), gains["vel_gain"])
                state["box"][s] = nb
                x, q = flame[r], state["params"][s]
                state["params"][s] = np.where(np.isfinite(x), _smooth(q, x, gains["param_gain"]), q)
                state["hits"][s] += 1
                state["misses"][s] = 0
                state["score"][s] = scores[r]
                state["det_row"][s] = r
                det_id[r] = state["id"][s]
            else:  # 6. unmatched
                state["box"][s] = pred[s]
                state["misses"][s] += 1
                state["det_row"][s] = -1
                if state["hits"][s] < R["min_hits"] or state["misses"][s] > R["max_age"]:
                    for k in ("hits", "misses", "age", "score", "box", "vel"):
                        state[k][s] = 0
                    state["id"][s] = state["det_row"][s] = -1
                    n_freed += 1
        # 7. births
        free = [int(s) for s in np.flatnonzero(state["id"] < 0)]
        cand = [int(r) for r in np.flatnonzero(high) if r not in taken]
        n_born = min(len(free), len(cand))
        for s, r in zip(free, cand):
            state["id"][s] = det_id[r] = state["next_id"][0]
            state["next_id"][0] += 1
            state["box"][s], state["vel"][s] = det[r], 0
            state["params"][s] = np.where(np.isfinite(flame[r]), flame[r], F(0))
            state["hits"][s], state["misses"][s], state["age"][s] = 1, 0, 0
            state["score"][s], state["det_row"][s] = scores[r], r
        # 8. report
        alive = state["id"] >= 0
        rep = np.flatnonzero(alive & (state["hits"] >= R["min_hits"]) & (state["misses"] <= R["report_misses"]))[:max_out]
        n = len(rep)
        out = dict(n_out=np.int32([n]), out_slot=np.full(max_out, -1, np.int32), out_id=np.full(max_out, -1, np.int32), out_det_row=np.full(max_out, -1, np.int32),
                   out_hits=np.zeros(max_out, np.int32), out_misses=np.zeros(max_out, np.int32), out_box=np.zeros((max_out, 4), F), out_score=np.zeros(max_out, F),
                   out_params=np.zeros((max_out, NP_), F), det_id=det_id, n_born=np.int32([n_born]), n_freed=np.int32([n_freed]), n_dropped=np.int32([len(cand) - n_born]))
        out["out_slot"][:n] = rep
        for k, field in (("out_id", "id"), ("out_det_row", "det_row"), ("out_hits", "hits"), ("out_misses", "misses"), ("out_box", "box"), ("out_score", "score"),
                         ("out_params", "params")):
            out[k][:n] = state[field][rep]
        state["age"][alive] += 1
        state["frame"][0] += 1
    return out


def track(state: dict, boxes, scores, flame, counts, unpad, form="loop", **rule) -> dict:
    """B frames in order: every output stacked along a leading frame axis."""
    frames = [step(state, boxes[f], scores[f], flame[f], counts[f], unpad[f], form, **rule) for f in range(len(counts))]
    out = {k: np.stack([fr[k] for fr in frames]) for k in OUTPUTS}
    for k in ("n_out", "n_born", "n_freed", "n_dropped"):
        out[k] = out[k].reshape(-1)  # [B]
    return out


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------------------------
def param_vector(value: float) -> np.ndarray:
    return (F(value) + np.arange(NP_, dtype=F) * F(0.001)).astype(F)


def from_frames(frames, keep_k: int, unpad=(0.0, 0.0, 1.0)):
    """frames: per frame a list of (box in IMAGE coordinates, score[, parameter value or vector]) in row order -> (boxes, scores, flame, counts, unpad) with the
    boxes in the padded space of ``unpad``; absent rows hold a box that would match everything and a score of 1, so that reading past counts shows."""
    B = len(frames)
    boxes, scores = np.tile(F([0, 0, 640, 640]), (B, keep_k, 1)), np.ones((B, keep_k), F)
    flame, counts = np.full((B, keep_k, NP_), 7, F), np.zeros(B, np.int32)
    px, py, s = unpad
    for f, rows in enumerate(frames):
        for r, row in enumerate(rows):
            box = np.asarray(row[0], np.float64)
            boxes[f, r] = box * s + [px, py, px, py]
            scores[f, r] = row[1]
            v = row[2] if len(row) > 2 else float(r)
            flame[f, r] = param_vector(v) if np.isscalar(v) else v
        counts[f] = len(rows)
    return boxes, scores, flame, counts, np.tile(F(unpad), (B, 1))


def sq(x, y, w=20.0):
    return (x, y, x + w, y + w)


CHAIN_N = 6


def planted_cases() -> dict:
    """name -> dict(boxes, scores, flame, counts, unpad, max_tracks, rule, claim): ``claim(out, state, run)`` asserts on the restatement's outputs (stacked over the
    frames) and final state that the sequence contains what it is there for; ``run(**rule_overrides)`` re-runs the restatement on the same sequence."""
    cases = {}

    def add(name, frames, claim, max_tracks=4, keep_k=4, unpad=(0.0, 0.0, 1.0), edit=None, **rule):
        seq = list(from_frames(frames, keep_k, unpad))
        if edit:
            edit(*seq)
        cases[name] = dict(boxes=seq[0], scores=seq[1], flame=seq[2], counts=seq[3], unpad=seq[4], max_tracks=max_tracks, rule=rule, claim=claim)

    # two heads of 40 px, 16 px per frame towards each other, 6 px apart in y, the rows swapped in every other frame.  In frame 2 each head's detection lies
    # where the OTHER head's box of frame 1 was: with the velocity the prediction is the head's own detection (IoU 1), without it the other's wins (0.74 > 0.43)
    def crossing(out, state, run):
        rows_a = [0, 1, 0, 1, 0]
        assert all(out["det_id"][f][rows_a[f]] == 0 and out["det_id"][f][1 - rows_a[f]] == 1 for f in range(5)) and int(out["n_born"].sum()) == 2
        still = run(vel_gain=0.0)[0]
        assert still["det_id"][2][rows_a[2]] == 1 and still["det_id"][2][1 - rows_a[2]] == 0  # the identities swap at the crossing

    frames = []
    for f in range(5):
        a, b = (sq(100 + 16 * f, 100, 40.0), 0.9, 1.0), (sq(148 - 16 * f, 106, 40.0), 0.8, 2.0)
        frames.append([a, b] if f % 2 == 0 else [b, a])
    add("crossing", frames, crossing, min_hits=1, vel_gain=1.0, match_thr_low=0.5)

    def dip(out, state, run):
        assert out["det_id"][:, 0].tolist() == [0] * 5 and int(out["n_born"].sum()) == 1 and state["hits"][0] == 5
        assert int(run(low_thr=0.4)[0]["n_born"].sum()) == 2  # without stage 2 (the dip below low_thr) the track is lost and the head is born again

    add("score_dip", [[(sq(50, 50), s)] for s in (0.9, 0.9, 0.3, 0.3, 0.9)], dip, min_hits=1, max_age=0)

    def low_only(out, state, run):
        assert not out["n_born"].any() and (state["id"] == -1).all() and (out["det_id"] == -1).all() and state["next_id"][0] == 0

    add("low_never_gives_birth", [[(sq(50, 50), 0.3)] for _ in range(4)], low_only)

    def tentative(out, state, run):
        assert out["n_born"].tolist() == [1, 0, 0] and out["n_freed"].tolist() == [0, 1, 0] and (state["id"] == -1).all() and not out["n_out"].any()
        assert run(min_hits=1)[0]["n_freed"].tolist() == [0, 0, 0]

    add("tentative_deleted_on_first_miss", [[(sq(50, 50), 0.9)], [], []], tentative, min_hits=3)

    def coasting(out, state, run):
        assert out["n_out"].tolist() == [1, 1, 1, 1] and out["out_misses"][:, 0].tolist() == [0, 1, 2, 0] and out["out_det_row"][:, 0].tolist() == [0, -1, -1, 0]
        assert out["n_freed"].tolist() == [0, 0, 0, 1] and out["n_born"].tolist() == [1, 0, 0, 1] and out["out_id"][:, 0].tolist() == [0, 0, 0, 1]
        assert out["out_slot"][:, 0].tolist() == [0, 0, 0, 0] and state["age"][0] == 1

    add("coasting_then_reuse", [[(sq(50, 50), 0.9)], [], [], [(sq(300, 300), 0.9)]], coasting, max_tracks=1, min_hits=1, max_age=2, report_misses=2)

    def dropped(out, state, run):
        assert out["n_born"].tolist() == [2, 0, 0] and out["n_dropped"].tolist() == [2, 2, 2] and out["det_id"][0].tolist() == [0, 1, -1, -1]

    add("table_full", [[(sq(50 + 60 * k, 50), 0.9) for k in range(4)]] * 3, dropped, max_tracks=2, min_hits=1)

    # the zigzag s0 r0 s1 r1 ... with strictly shrinking gaps: every slot prefers the row on its right, every row the slot on its right, only the last pair is
    # mutual, and the matching resolves from the right one pair per round
    def chain(out, state, run):
        assert out["det_id"][1][:CHAIN_N].tolist() == list(range(CHAIN_N))
        run(form="vec")
        assert LAST_ROUNDS[0] == CHAIN_N + 1, LAST_ROUNDS

    gaps = [8.0 - 0.3 * k for k in range(2 * CHAIN_N - 1)]
    at = np.concatenate([[0.0], np.cumsum(gaps)]) + 40.0
    add("chain", [[(sq(at[2 * i], 50), 0.9) for i in range(CHAIN_N)], [(sq(at[2 * i + 1], 50), 0.9) for i in range(CHAIN_N)]], chain, max_tracks=8, keep_k=8, min_hits=1)

    def ties(out, state, run):
        assert out["det_id"][0].tolist()[:2] == [0, 1] and out["det_id"][1].tolist()[:2] == [0, 1] and out["det_id"][2].tolist()[:2] == [0, -1]
        assert state["misses"][:2].tolist() == [0, 1] and np.array_equal(state["box"][0], state["box"][1])

    add("exact_ties", [[(sq(50, 50), 0.9), (sq(50, 50), 0.9)], [(sq(50, 50), 0.9), (sq(50, 50), 0.9)], [(sq(50, 50), 0.9)]], ties, min_hits=1)

    # counts of 0 with rows that would match and give birth if they were read, a count above keep_k and a negative one
    def counts_claim(out, state, run):
        assert out["n_born"].tolist() == [0, 4, 0, 0] and (out["det_id"][0] == -1).all() and (out["det_id"][2] == -1).all() and out["n_out"].tolist() == [0, 4, 4, 4]

    def counts_edit(boxes, scores, flame, counts, unpad):
        counts[:] = [0, 9, 0, -3]

    add("counts_outside", [[(sq(50 + 60 * k, 50), 0.9) for k in range(4)]] * 4, counts_claim, edit=counts_edit, min_hits=1, report_misses=5)

    nan, inf = float("nan"), float("inf")

    def non_finite(out, state, run):
        assert np.isfinite(state["box"]).all() and np.isfinite(state["params"]).all() and np.isfinite(out["out_box"]).all()
        assert out["det_id"][0].tolist() == [0, -1, 1, -1] and state["params"][0, 5] == 0 and state["params"][0, 6] == 0  # NaN and -inf scores are ignored, +inf is HIGH
        assert out["det_id"][1].tolist()[:2] == [0, 1] and state["params"][1, 7] == param_vector(2.0)[7]  # an infinite element keeps the old value
        assert state["box"][0].tolist() == [0.0, 50.0, 70.0, 70.0]  # NaN -> 0

    def non_finite_edit(boxes, scores, flame, counts, unpad):
        flame[0, 0, 5], flame[0, 0, 6], flame[1, 1, 7], flame[1, 1, 8] = nan, -inf, inf, nan  # born with 0; keeps the old value
        flame[1, 0, 5], flame[1, 0, 6] = inf, nan  # matched: the 0 of the birth stays

    add("non_finite", [[((nan, 50, 70, 70), 0.9), (sq(200, 200), nan), ((300, -inf, 320, 320), inf, 2.0), (sq(400, 400), -inf)],
                       [((nan, 50, 70, 70), 0.9), ((300, -inf, 320, 320), 0.9, 3.0)]], non_finite, edit=non_finite_edit, min_hits=1)

    def gains_one(out, state, run):
        x, q = param_vector(0.3), param_vector(1e-3)
        assert ((q + F(1) * (x - q)).astype(F) != x).any()  # why the special case is there
        assert state["params"][0].tobytes() == x.tobytes() and state["box"][0].tolist() == [53.0, 50.5, 73.0, 70.5] and state["vel"][0].tolist() == [3.0, 0.5, 3.0, 0.5]

    add("gains_of_one", [[(sq(50, 50), 0.9, 1e-3)], [(sq(53, 50.5), 0.9, 0.3)]], gains_one, min_hits=1, box_gain=1.0, vel_gain=1.0, param_gain=1.0)

    # a threshold below 0: boxes that do not overlap at all (iou = 0) are a pair
    def negative(out, state, run):
        assert out["det_id"][1][0] == 0 and int(out["n_born"].sum()) == 1 and state["box"][0].tolist() == [300.0, 300.0, 320.0, 320.0]
        assert int(run(match_thr=0.0)[0]["n_born"].sum()) == 2

    add("negative_threshold", [[(sq(50, 50), 0.9)], [(sq(300, 300), 0.9)]], negative, min_hits=1, match_thr=-1.0)

    # a letterboxed frame (1280 x 960 at S = 640) and the cap of the report
    def capped(out, state, run):
        assert out["n_out"].tolist() == [2, 2] and out["out_slot"][1].tolist() == [0, 1] and (state["id"] >= 0).sum() == 4
        assert np.array_equal(out["out_box"][0, 0], F([100, 100, 140, 140]))

    add("letterbox_and_cap", [[(sq(100 + 100 * k, 100, 40.0), 0.9) for k in range(4)]] * 2, capped, unpad=(0.0, 80.0, 0.5), min_hits=1, max_out=2)
    return cases


def run_case(case: dict, form="loop", **overrides):
    state = new_state(case["max_tracks"])
    out = track(state, case["boxes"], case["scores"], case["flame"], case["counts"], case["unpad"], form, **dict(case["rule"], **overrides))
    return out, state


def random_sequence(max_tracks: int, keep_k: int, live: int, n_frames: int, seed: int, grid: float = 0.0, width: int = 1280, height: int = 960, head_px=(16.0, 48.0)):
    """A seeded video: ``live`` heads drifting at constant velocity over a ``width`` x ``height`` image letterboxed to 640, each seen in a frame with
    probability 0.85 (a few twice, with the same box: exact ties), scores from six values on both sides of the default thresholds, some false positives, the
    rows shuffled, a few non-finite parameter elements; a frame keeps its first keep_k rows.  ``grid`` > 0 snaps every coordinate to its multiples, which makes
    equal IoUs common."""
    rng = np.random.default_rng(seed)
    scale = 640.0 / max(width, height)
    pad = ((640 - width * scale) / 2, (640 - height * scale) / 2)
    size = rng.uniform(head_px[0], head_px[1], live)
    pos = rng.uniform(0, 1, (live, 2)) * [width - head_px[1], height - head_px[1]]
    vel = rng.normal(0, 4.0, (live, 2))
    frames = []
    for f in range(n_frames):
        rows = []
        for h in range(live):
            if rng.uniform() < 0.85:
                xy = pos[h] + vel[h] * f + rng.normal(0, 0.5, 2)
                box = np.array([xy[0], xy[1], xy[0] + size[h], xy[1] + size[h]])
                if grid:
                    box = np.round(box / grid) * grid
                v = param_vector(h + 0.01 * f)
                if rng.uniform() < 0.05:
                    v[rng.integers(0, NP_)] = (np.nan, np.inf)[f % 2]
                rows.append((box, rng.choice([0.05, 0.1, 0.3, 0.5, 0.6, 0.9]), v))
                if rng.uniform() < 0.05:
                    rows.append((box, rows[-1][1], v))
        for _ in range(max(1, live // 10)):
            xy = rng.uniform(0, 1, 2) * [width - 40, height - 40]
            rows.append((np.array([xy[0], xy[1], xy[0] + 30, xy[1] + 30]), rng.choice([0.3, 0.6]), float(f)))
        rng.shuffle(rows)
        frames.append(rows[:keep_k])
    return from_frames(frames, keep_k, (pad[0], pad[1], scale))
