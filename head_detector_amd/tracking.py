"""Head tracking across video frames: stable identities, heads that survive a few frames of occlusion, smoothed boxes and smoothed FLAME parameters, associated on
the device (libvghtrack.so, include/vgh_track.h).  ``track_frames`` is the thin wrapper of vght_track_frames, ``TrackState`` owns the device-resident track
table, ``HeadTracker`` puts a ``HeadDetector`` in front of them.

The rule is stated once, in include/vgh_track.h; DESIGN.md 3.6k repeats it and tests/head_track_ref.py restates it in NumPy: ByteTrack's two-stage association
(tracks against the confident detections, then the tracks still unmatched against the weak ones) as the greedy matching in the total order (IoU descending, slot
ascending, row ascending), a constant-velocity prediction of the box, and exponential smoothing of the box, the velocity and the 413 FLAME parameters.  Every
threshold and gain below is an API default, NOT a tuned value: no real weights or video exist in this tree to tune them on."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

from .detection_result import PredictionResult

RULE_DEFAULTS = dict(high_thr=0.5, low_thr=0.1, match_thr=0.3, match_thr_low=0.5, max_age=30, min_hits=3, report_misses=0, box_gain=1.0, vel_gain=0.5, param_gain=0.5)


def check_rule(who: str, rule: dict) -> dict:
    """The rule's parameters with the defaults filled in; ValueError for an unknown name or a value the library would reject."""
    unknown = set(rule) - set(RULE_DEFAULTS)
    if unknown:
        raise ValueError(f"{who}: unknown rule parameter(s) {sorted(unknown)}; the rule has {sorted(RULE_DEFAULTS)}")
    R = dict(RULE_DEFAULTS, **rule)
    for k in ("high_thr", "low_thr", "match_thr", "match_thr_low"):
        if not isinstance(R[k], (int, float)) or math.isnan(R[k]):
            raise ValueError(f"{who}: {k} {R[k]!r} is not a number")
    for k in ("box_gain", "vel_gain", "param_gain"):
        if not isinstance(R[k], (int, float)) or not math.isfinite(R[k]):
            raise ValueError(f"{who}: {k} {R[k]!r} is not a finite number")
    for k, least in (("max_age", 0), ("min_hits", 1), ("report_misses", 0)):
        if int(R[k]) != R[k] or R[k] < least:
            raise ValueError(f"{who}: {k} {R[k]!r} is not an integer >= {least}")
    return R


class TrackState:
    """The device-resident track table of ``max_tracks`` slots (the layout include/vgh_track.h documents), one caller-owned block; ``ids``, ``hits``, ``misses``,
    ``age``, ``det_row``, ``scores``, ``boxes``, ``vel`` and ``params`` are tensor views of it (a free slot has id -1), ``next_id`` and ``frame`` views of its two
    scalars.  ``reset()`` frees every slot and restarts the ids at 0."""

    def __init__(self, max_tracks: int = 256, device: Any = None):
        import torch

        from . import _lib_track

        if int(max_tracks) != max_tracks or not 1 <= max_tracks <= _lib_track.MAX_TRACKS:
            raise ValueError(f"TrackState: max_tracks {max_tracks!r} outside 1 .. {_lib_track.MAX_TRACKS}")
        self.max_tracks = M = int(max_tracks)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"TrackState: device {self.device} is not a GPU (there is no CPU path)")
        at = _lib_track.state_layout(M)
        lib = _lib_track.load()
        assert at["total"] == lib.vght_state_bytes(M)
        self.buffer = torch.empty(at["total"], dtype=torch.uint8, device=self.device)

        def view(name, n, dtype, *shape):
            return self.buffer[at[name]:at[name] + 4 * n].view(dtype).view(*shape)

        i32, f32 = torch.int32, torch.float32
        header = self.buffer[:_lib_track.STATE_HEADER_BYTES].view(i32)
        self.next_id, self.frame = header[0:1], header[1:2]
        self.ids, self.hits, self.misses, self.age, self.det_row = (view(k, M, i32, M) for k in ("id", "hits", "misses", "age", "det_row"))
        self.scores = view("score", M, f32, M)
        self.boxes, self.vel = view("box", 4 * M, f32, M, 4), view("vel", 4 * M, f32, M, 4)
        self.params = view("params", _lib_track.NUM_PARAMS * M, f32, M, _lib_track.NUM_PARAMS)
        self.reset()

    def reset(self) -> None:
        import torch

        from . import _lib_track

        with torch.cuda.device(self.device):
            _lib_track.check(_lib_track.load().vght_state_init(self.buffer.data_ptr(), self.max_tracks, torch.cuda.current_stream(self.device).cuda_stream))


@dataclass
class TrackedFrames:
    """What ``track_frames`` returns: capacity-sized tensors on the GPU, one row per frame; the first ``n_out[b]`` rows of frame b are its reported tracks in
    ascending slot order, the rows behind hold -1 (slot, ids, det_row) and zeros."""

    n_out: "torch.Tensor"  # int32 [B]
    slot: "torch.Tensor"  # int32 [B, max_out]
    ids: "torch.Tensor"  # int32 [B, max_out]
    det_row: "torch.Tensor"  # int32 [B, max_out]: the detection row of the frame, -1 for a coasting track
    hits: "torch.Tensor"  # int32 [B, max_out]
    misses: "torch.Tensor"  # int32 [B, max_out]
    boxes: "torch.Tensor"  # float32 [B, max_out, 4] xyxy in image coordinates, smoothed
    scores: "torch.Tensor"  # float32 [B, max_out]
    params: Optional["torch.Tensor"]  # float32 [B, max_out, 413], smoothed; None without want_params
    det_id: "torch.Tensor"  # int32 [B, keep_k]: the id every detection row was given, -1 if none
    n_born: "torch.Tensor"  # int32 [B]
    n_freed: "torch.Tensor"  # int32 [B]
    n_dropped: "torch.Tensor"  # int32 [B]: confident detections that found no free slot


def track_frames(boxes, scores, flame_params, counts, unpad, state: TrackState, *, image_size: int = 640, max_out: Optional[int] = None, want_params: bool = True,
                 **rule) -> TrackedFrames:
    """Steps ``state`` through B frames in order (vght_track_frames) with the per-frame slabs exactly as ``VGHeadsEngine.detect`` leaves them: ``boxes``
    [B, keep_k, 4] xyxy in the padded S-space of each frame, ``scores`` [B, keep_k], ``flame_params`` [B, keep_k, 413], ``counts`` [B] int32, all contiguous on the
    GPU of ``state``; ``unpad`` [B, 3] = (pad_x, pad_y, scale) per frame on the host (letterbox.geometry).  Queued on the current stream; nothing is read back.
    ``rule``: high_thr, low_thr, match_thr, match_thr_low, max_age, min_hits, report_misses, box_gain, vel_gain, param_gain (API defaults, not tuned values).
    ``max_out`` (default ``state.max_tracks``): rows of the per-frame outputs."""
    import torch

    from . import _lib_track

    R = check_rule("track_frames", rule)
    if not isinstance(state, TrackState):
        raise ValueError(f"track_frames: state must be a TrackState; got {type(state).__name__}")
    max_out = state.max_tracks if max_out is None else max_out
    if int(max_out) != max_out or not 1 <= max_out <= _lib_track.MAX_TRACKS:
        raise ValueError(f"track_frames: max_out {max_out!r} outside 1 .. {_lib_track.MAX_TRACKS}")
    if int(image_size) != image_size or image_size < 1:
        raise ValueError(f"track_frames: image_size {image_size!r} is not a positive integer")
    for name, t, dtype in (("boxes", boxes, torch.float32), ("scores", scores, torch.float32), ("flame_params", flame_params, torch.float32), ("counts", counts, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError(f"track_frames: {name} must be a {dtype} tensor; got {getattr(t, 'dtype', type(t))}")
    if boxes.dim() != 3 or boxes.shape[0] < 1 or boxes.shape[1] < 1 or boxes.shape[2] != 4:
        raise ValueError(f"track_frames: boxes must be [B >= 1, keep_k >= 1, 4]; got {tuple(boxes.shape)}")
    B, keep_k = int(boxes.shape[0]), int(boxes.shape[1])
    if B > _lib_track.MAX_FRAMES or keep_k > _lib_track.MAX_DETS:
        raise ValueError(f"track_frames: B = {B} frames of keep_k = {keep_k} rows exceed the {_lib_track.MAX_FRAMES} frames of {_lib_track.MAX_DETS} rows of one call")
    if tuple(scores.shape) != (B, keep_k) or tuple(flame_params.shape) != (B, keep_k, _lib_track.NUM_PARAMS) or tuple(counts.shape) != (B,):
        raise ValueError(f"track_frames: scores must be [{B}, {keep_k}], flame_params [{B}, {keep_k}, {_lib_track.NUM_PARAMS}] and counts [{B}]; got "
                         f"{tuple(scores.shape)}, {tuple(flame_params.shape)} and {tuple(counts.shape)}")
    table = np.ascontiguousarray(np.asarray(unpad, dtype=np.float32))
    if table.shape != (B, 3) or not np.isfinite(table).all() or not (table[:, 2] > 0).all():
        raise ValueError(f"track_frames: unpad must be [{B}, 3] finite (pad_x, pad_y, scale) rows with a positive scale; got shape {table.shape}")
    for name, t in (("boxes", boxes), ("scores", scores), ("flame_params", flame_params), ("counts", counts)):
        if not t.is_cuda or t.device != state.device or not t.is_contiguous():
            raise ValueError(f"track_frames: {name} must be a contiguous tensor on the GPU of the state, {state.device} (there is no CPU path)")
    lib = _lib_track.load()
    dev, O = state.device, int(max_out)
    with torch.cuda.device(dev):
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        out = TrackedFrames(torch.empty(B, **i32), torch.empty(B, O, **i32), torch.empty(B, O, **i32), torch.empty(B, O, **i32), torch.empty(B, O, **i32),
                            torch.empty(B, O, **i32), torch.empty(B, O, 4, **f32), torch.empty(B, O, **f32),
                            torch.empty(B, O, _lib_track.NUM_PARAMS, **f32) if want_params else None, torch.empty(B, keep_k, **i32), torch.empty(B, **i32),
                            torch.empty(B, **i32), torch.empty(B, **i32))
        ws = torch.empty(max(16, int(lib.vght_workspace_bytes(state.max_tracks, keep_k))), dtype=torch.uint8, device=dev)
        job = _lib_track.TrackJob(B, keep_k, state.max_tracks, int(image_size), O, int(R["max_age"]), int(R["min_hits"]), int(R["report_misses"]), float(R["high_thr"]),
                                  float(R["low_thr"]), float(R["match_thr"]), float(R["match_thr_low"]), float(R["box_gain"]), float(R["vel_gain"]), float(R["param_gain"]), 0,
                                  boxes.data_ptr(), scores.data_ptr(), flame_params.data_ptr(), counts.data_ptr(), table.ctypes.data, out.n_out.data_ptr(), out.slot.data_ptr(),
                                  out.ids.data_ptr(), out.det_row.data_ptr(), out.hits.data_ptr(), out.misses.data_ptr(), out.boxes.data_ptr(), out.scores.data_ptr(),
                                  out.params.data_ptr() if want_params else None, out.det_id.data_ptr(), out.n_born.data_ptr(), out.n_freed.data_ptr(), out.n_dropped.data_ptr())
        _lib_track.check(lib.vght_track_frames(_lib_track.C.byref(job), state.buffer.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out


class TrackedPredictionResult(PredictionResult):
    """A ``PredictionResult`` whose heads are the reported tracks of one frame, in ascending slot order, with three arrays beside them: ``track_ids`` int64 [n],
    ``hits`` int64 [n] (frames in which the track was matched) and ``coasting`` bool [n] (no detection in this frame: the box is the prediction, the parameters the
    last smoothed ones; only with ``report_misses`` > 0).  Everything a ``PredictionResult`` does works on it unchanged."""

    def __init__(self, *args, track_ids: np.ndarray, hits: np.ndarray, coasting: np.ndarray, **kwargs):
        super().__init__(*args, **kwargs)
        self.track_ids, self.hits, self.coasting = track_ids, hits, coasting


class HeadTracker:
    """``HeadDetector`` on a video: ``update(frame)`` / ``update_batch(frames)`` -> ``TrackedPredictionResult`` per frame.  Up to the detector's ``max_batch`` frames go
    through ONE ``engine.detect`` call at ``confidence_threshold=low_thr``, one vght_track_frames call, one host read of the reported counts and one FLAME decode of
    all reported tracks' SMOOTHED parameters, un-padded per frame.  A head's box is rint of the smoothed image box clipped to the image, its ``FlameParams`` come from
    the smoothed vector (scale divided by the frame's letterbox scale, translation left in the padded space, like ``detect_batch``) and its head pose from them.
    The rotation-6D and jaw elements are smoothed linearly like every other element; FLAME decode re-orthonormalises the 6D rotation, which is what makes that
    admissible.  All frames of a tracker have one size; ``reset()`` forgets every track (and the size).  The defaults are API defaults, not tuned values."""

    def __init__(self, detector, *, max_tracks: int = 256, high_thr: float = 0.5, low_thr: float = 0.1, match_thr: float = 0.3, match_thr_low: float = 0.5,
                 max_age: int = 30, min_hits: int = 3, report_misses: int = 0, box_gain: float = 1.0, vel_gain: float = 0.5, param_gain: float = 0.5):
        self.rule = check_rule("HeadTracker", dict(high_thr=high_thr, low_thr=low_thr, match_thr=match_thr, match_thr_low=match_thr_low, max_age=max_age, min_hits=min_hits,
                                                   report_misses=report_misses, box_gain=box_gain, vel_gain=vel_gain, param_gain=param_gain))
        self.detector = detector
        self.state = TrackState(max_tracks, detector._device)
        if max_tracks > detector._flame.max_heads:
            raise ValueError(f"HeadTracker: max_tracks={max_tracks} exceeds the FLAME layer's capacity of {detector._flame.max_heads} heads")
        self._frame_shape = None
        self.last_frames: Optional[TrackedFrames] = None  # what the last update_batch got from track_frames, on the device

    def reset(self) -> None:
        self.state.reset()
        self._frame_shape = None

    def update(self, frame, *, rgb: str = "host") -> TrackedPredictionResult:
        return self.update_batch([frame], rgb=rgb)[0]

    def update_batch(self, frames: Sequence, *, rgb: str = "host") -> List[TrackedPredictionResult]:
        """``frames``: RGB images as ``HeadDetector.detect_batch`` takes them, or ``video.YUV420Frame`` s / ``video.YUV420Frame16`` s (one kind, all of them; converted inside the device letterbox).  For
        those, each result's ``original_image`` is the frame's ``to_rgb()``: a NumPy array, or with ``rgb="device"`` a GPU tensor, or with ``rgb="none"`` None (no RGB
        copy is made), and its ``source_frame`` is the frame, which ``anonymize_frame`` works on."""
        import torch

        from .head_info import Bbox, FlameParams, HeadMetadata
        from .letterbox import geometry
        from .utils import calculate_rpy

        det = self.detector
        if len(frames) > det._max_batch:
            raise ValueError(f"update_batch: {len(frames)} frames exceed max_batch={det._max_batch} (pass max_batch= to HeadDetector)")
        from .video import FRAME_TYPES, frame_rgb

        yuv = any(isinstance(im, FRAME_TYPES) for im in frames)  # (a list mixing them with RGB images is refused by the engine)
        if rgb != "host" and not yuv:
            raise ValueError(f"rgb={rgb!r} applies to YUV420Frame inputs only")
        originals = list(frames) if yuv else [det._convert_image(im) for im in frames]
        if not originals:
            return []
        raw = []
        for im in originals:
            src = im if yuv else torch.from_numpy(np.ascontiguousarray(im))
            if not yuv and (src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] < 3):
                raise ValueError(f"update_batch expects uint8 frames [H,W,3]; got {src.dtype} {tuple(src.shape)}")
            shape = (int(src.shape[0]), int(src.shape[1]))
            if self._frame_shape is None:
                self._frame_shape = shape
            if shape != self._frame_shape:
                raise ValueError(f"update_batch: a frame of {shape[0]} x {shape[1]} after frames of {self._frame_shape[0]} x {self._frame_shape[1]}: a tracker's boxes "
                                 "live in one image's coordinates; call reset() before a video of another size")
            raw.append(src if yuv else src.to(det._device, non_blocking=True))
        H, W = self._frame_shape
        S, B = det._image_size, len(raw)
        _, _, pad_x, pad_y, scale = geometry(H, W, S)
        unpad = np.tile(np.float32([pad_x, pad_y, scale]), (B, 1))
        slabs = det.model.detect(raw, confidence_threshold=float(self.rule["low_thr"]), flame=None)
        tracked = track_frames(slabs.boxes, slabs.scores, slabs.flame_params, slabs.counts, unpad, self.state, image_size=S, **self.rule)
        self.last_frames = tracked
        n_out = tracked.n_out.cpu().numpy()  # the one host read the heads depend on
        at = np.concatenate([[0], np.cumsum(n_out)]).astype(int)
        n, P = int(at[-1]), det.model.program
        smoothed = torch.cat([tracked.params[b, :n_out[b]] for b in range(B)]) if n else tracked.params[0, :0]
        if n:  # one decode of every reported track of every frame, un-padded straight into image coordinates
            rows = torch.from_numpy(unpad).to(det._device)[torch.from_numpy(np.repeat(np.arange(B), n_out)).to(det._device)].contiguous()
            _, _, verts = det._flame.decode(smoothed.contiguous(), unpad=rows, shape_live=P.shape_c, expr_live=P.expr_c, want_vertices=False)
            verts = verts.cpu().numpy()
        else:
            verts = np.zeros((0, det._flame.v_template.shape[0], 3), dtype=np.float32)
        smoothed = smoothed.detach().cpu()
        boxes, scores = tracked.boxes.cpu().numpy(), tracked.scores.cpu().numpy()
        ids, hits, misses = tracked.ids.cpu().numpy(), tracked.hits.cpu().numpy(), tracked.misses.cpu().numpy()
        results = []
        for b, orig in enumerate(originals):
            frame = orig if yuv else None
            if yuv:
                orig = frame_rgb(orig, rgb)
            k = int(n_out[b])
            bb = np.rint(boxes[b, :k]).astype(int)
            bb[:, [0, 2]] = bb[:, [0, 2]].clip(0, W)
            bb[:, [1, 3]] = bb[:, [1, 3]].clip(0, H)
            heads = []
            for i in range(k):
                fp = FlameParams.from_3dmm(smoothed[at[b] + i].unsqueeze(0))
                fp.scale = fp.scale / scale
                heads.append(HeadMetadata(bbox=Bbox(x=bb[i, 0], y=bb[i, 1], w=bb[i, 2] - bb[i, 0], h=bb[i, 3] - bb[i, 1]), score=scores[b, i], flame_params=fp,
                                          vertices_3d=verts[at[b] + i], head_pose=calculate_rpy(fp)))
            results.append(TrackedPredictionResult(original_image=orig, heads=heads, faces=det._flame.faces, pncc_processor=det._pncc, head_indices=det._head_indices,
                                                   triangles=det._triangles, face_indices=det._face_indices, track_ids=ids[b, :k].astype(np.int64),
                                                   hits=hits[b, :k].astype(np.int64), coasting=misses[b, :k] > 0, source_frame=frame))
        return results
