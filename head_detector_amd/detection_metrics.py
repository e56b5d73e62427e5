"""Detection benchmark metrics: the AP of a set of detected heads against annotated boxes, as the reference's two head-detection benchmarks report it
(yolo_head_training/evaluation/evaluate_wider.py and evaluate_fddb.py: both hand ``[x, y, w, h, score]`` rows and ``[x, y, w, h]`` annotations to
pycocotools' ``COCOeval(..., 'bbox')`` and print ``stats[0]`` as "mAP").

  box_iou(dt_xywh, gt_xywh, crowd=None)                         -> [nd, ng] float64                     bbIou                                   (device)
  match_detections(detections, ground_truth, ...)               -> DetectionMatches                     COCOeval.evaluate                        (device)
  average_precision(detections, ground_truth, ...)              -> DetectionAP                          evaluate + accumulate (device), summarize (host)
  DetectionEvaluator(...).add(...) / .evaluate() / .reset()     -> DetectionAP                          image by image, as the evaluators collect
  rows_from_xyxy(boxes_xyxy, scores)                            -> [[x, y, w, h, score], ...]            parse_predictions                        (host)
  sanitize_predictions(rows, image_shape)                       -> [[x, y, w, h, score], ...]            FDDB's crop to the image                 (host)
  read_wider_annotations(path) / read_fddb_annotations(path)    -> {file name: [[x, y, w, h], ...]}      read_annotations of the two evaluators   (host)

IoU, the greedy matching, the global sort and the precision/recall curves run in csrc/detection_ap.hip (libvgheval.so, include/vgh_eval.h states the
semantics); there is no CPU path for them.  Every float is a single float64 operation in a stated order or an exact count, so the results are bitwise
reproducible and equal to the NumPy restatement tests/detection_ap_ref.py.  The semantics are pycocotools' BY ITS PUBLISHED DEFINITION: pycocotools is
not available to this project, so the values are UNPINNED against pycocotools itself (tools/first_contact.py compares wherever it is installed).

THE QUIRK OF THE DEFAULTS, kept.  COCOeval's ``maxDets`` is (1, 10, 100) and ``stats[0]`` is read at the last of them: only the 100 best detections of
an image count, however many were passed in.  The reference evaluates WIDER with up to 1 000 detections per image on images that hold up to ~2 000
faces, and inherits this: on a crowd its "mAP" cannot see more than 100 heads.  ``max_dets=(1, 10, 1000)`` is the intended reading.

Every function takes NumPy arrays or GPU tensors; the device functions return NumPy (``to_host=True``) or GPU tensors.  Arguments are validated
before a GPU is looked for."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib_eval
from .mesh_metrics import _host


def default_iou_thrs() -> np.ndarray:
    return np.linspace(.5, .95, 10)


def default_rec_thrs() -> np.ndarray:
    return np.linspace(0, 1, 101)


def default_area_ranges() -> np.ndarray:
    return np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------------------
def _device_of(*candidates):
    """The device of the first GPU tensor among the arguments; host data alone needs a GPU to be present."""
    for c in candidates:
        for e in (c if isinstance(c, (list, tuple)) else (c,)):
            if isinstance(e, torch.Tensor) and e.is_cuda:
                return e.device
    if not torch.cuda.is_available():
        raise _lib_eval.VghError("detection metrics need a GPU: the HIP kernels of libvgheval.so are the only implementation of the matching and the curves")
    return torch.device("cuda", torch.cuda.current_device())


def _rows(a, width, what) -> np.ndarray:
    """``a`` as finite float64 [n, width]; an empty list is [0, width]."""
    a = _host(a)
    if a.size == 0 and a.ndim <= 2:
        return np.zeros((0, width), dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what} must be [n, {width}], got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds NaN or infinite values")
    return np.ascontiguousarray(a)


def _thresholds(a, default, limit, what) -> np.ndarray:
    a = default() if a is None else _host(a)
    if a.ndim != 1 or not 1 <= a.shape[0] <= limit or not np.isfinite(a).all():
        raise ValueError(f"{what} must be 1 .. {limit} finite numbers, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _area_ranges(a) -> np.ndarray:
    a = default_area_ranges() if a is None else _host(a)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= _lib_eval.MAX_AREA_RNG or np.isnan(a).any():
        raise ValueError(f"area_ranges must be [A, 2] (lo, hi) with 1 <= A <= {_lib_eval.MAX_AREA_RNG}, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _max_dets(max_dets) -> tuple:
    try:
        out = tuple(int(k) for k in max_dets)
        exact = all(int(k) == k for k in max_dets)
    except TypeError:
        raise ValueError(f"max_dets must be a sequence of integers, got {max_dets!r}") from None
    if not exact or not 1 <= len(out) <= _lib_eval.MAX_MAX_DETS:
        raise ValueError(f"max_dets must be 1 .. {_lib_eval.MAX_MAX_DETS} integers, got {max_dets!r}")
    if any(k < 1 or k > _lib_eval.MAX_DET for k in out):
        raise ValueError(f"max_dets must lie in 1 .. {_lib_eval.MAX_DET} (the engine's top-k ceiling), got {out}")
    if any(b < a for a, b in zip(out, out[1:])):
        raise ValueError(f"max_dets must ascend, got {out}")
    return out


class _BoxSet:
    """Detections and ground truth of I images in CSR form on the host (``check``), then on the device (``upload``)."""

    def __init__(self, detections, ground_truth, gt_area=None, gt_crowd=None):
        detections, ground_truth = list(detections), list(ground_truth)
        if len(detections) != len(ground_truth):
            raise ValueError(f"{len(detections)} images of detections but {len(ground_truth)} of ground truth")
        n = len(detections)
        if n > _lib_eval.MAX_IMAGES:
            raise ValueError(f"{n} images exceed {_lib_eval.MAX_IMAGES}")
        for name, per_image in (("gt_area", gt_area), ("gt_crowd", gt_crowd)):
            if per_image is not None and len(per_image) != n:
                raise ValueError(f"{name} must hold one array per image ({n}), got {len(per_image)}")
        dts = [_rows(d, 5, f"detections[{i}]") for i, d in enumerate(detections)]
        gts = [_rows(g, 4, f"ground_truth[{i}]") for i, g in enumerate(ground_truth)]
        self.n = n
        self.dt_offset = np.zeros(n + 1, dtype=np.int64)
        self.gt_offset = np.zeros(n + 1, dtype=np.int64)
        if n:
            np.cumsum([len(d) for d in dts], out=self.dt_offset[1:])
            np.cumsum([len(g) for g in gts], out=self.gt_offset[1:])
        self.max_gt = int(np.diff(self.gt_offset).max(initial=0))
        if self.max_gt > _lib_eval.MAX_GT_PER_IMAGE:
            raise ValueError(f"an image holds {self.max_gt} ground truths, more than {_lib_eval.MAX_GT_PER_IMAGE}")
        if self.dt_offset[-1] > 2 ** 31 - 1 or self.gt_offset[-1] > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 boxes")
        dt = np.concatenate(dts) if dts else np.zeros((0, 5))
        self.dt_box = np.ascontiguousarray(dt[:, :4])
        self.dt_score = np.ascontiguousarray(dt[:, 4])
        self.gt_box = np.concatenate(gts) if gts else np.zeros((0, 4))
        self.gt_area = self.gt_crowd = None
        if gt_area is not None:
            parts = [_host(a).reshape(-1) for a in gt_area]
            if [len(p) for p in parts] != [len(g) for g in gts] or not all(np.isfinite(p).all() for p in parts):
                raise ValueError("gt_area must hold one finite number per ground truth")
            self.gt_area = np.concatenate(parts) if parts else np.zeros(0)
        if gt_crowd is not None:
            parts = [_host(c, None).reshape(-1) for c in gt_crowd]
            if [len(p) for p in parts] != [len(g) for g in gts]:
                raise ValueError("gt_crowd must hold one flag per ground truth")
            self.gt_crowd = (np.concatenate(parts) != 0).astype(np.uint8) if parts else np.zeros(0, dtype=np.uint8)

    def upload(self, dev):
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.dev = {"dt_box": up(self.dt_box), "dt_score": up(self.dt_score), "gt_box": up(self.gt_box), "gt_area": up(self.gt_area),
                    "gt_crowd": up(self.gt_crowd), "dt_offset": up(self.dt_offset.astype(np.int32)), "gt_offset": up(self.gt_offset.astype(np.int32))}
        s = _lib_eval.BoxSet()
        s.n_images, s.n_dt, s.n_gt, s.max_gt = self.n, int(self.dt_offset[-1]), int(self.gt_offset[-1]), self.max_gt
        for field, t in self.dev.items():
            setattr(s, field + "_dev", None if t is None else t.data_ptr())
        return s


def _run(fn_name, job, dev):
    with torch.cuda.device(dev):
        _lib_eval.check(getattr(_lib_eval.load(), fn_name)(C.byref(job), torch.cuda.current_stream().cuda_stream))


def _check_status(status, what):
    if int(status.item()) != 0:
        raise _lib_eval.VghError(f"{what}: the kernels found an image whose offsets contradict the array sizes")


# ---- IoU -----------------------------------------------------------------------------------------------------------------------------------------------
def box_iou(dt_xywh, gt_xywh, crowd=None, to_host: bool = True):
    """pycocotools' ``bbIou`` for every pair -> float64 [nd, ng].  Boxes are ``[x, y, w, h]``; with ``da = D.w * D.h`` and ``ga = G.w * G.h``,
    ``w = min(D.x + D.w, G.x + G.w) - max(D.x, G.x)`` (``h`` likewise; ``w <= 0`` or ``h <= 0`` gives 0), ``i = w * h``, the IoU is ``i / ((da + ga) - i)``,
    and ``i / da`` against a ground truth whose ``crowd`` flag ([ng], default none) is set.  Up to 4 096 ground truths."""
    dt, gt = _rows(dt_xywh, 4, "dt_xywh"), _rows(gt_xywh, 4, "gt_xywh")
    flags = None if crowd is None else [crowd]
    boxes = _BoxSet([np.concatenate([dt, np.zeros((len(dt), 1))], axis=1)], [gt], gt_crowd=flags)
    dev = _device_of(dt_xywh, gt_xywh)
    out = torch.empty((len(dt), len(gt)), dtype=torch.float64, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    offset = torch.tensor([0, out.numel()], dtype=torch.int64, device=dev)
    job = _lib_eval.BoxIouJob()
    job.set = boxes.upload(dev)
    job.n_iou, job.iou_offset_dev, job.iou_dev, job.status_dev = out.numel(), offset.data_ptr(), out.data_ptr() if out.numel() else None, status.data_ptr()
    _run("vghev_box_iou", job, dev)
    _check_status(status, "box_iou")
    return out.cpu().numpy() if to_host else out


# ---- matching ------------------------------------------------------------------------------------------------------------------------------------------
class DetectionMatches:
    """What ``match_detections`` returns.  The K kept detections (per image the ``max_det`` best by (-score, input position)) lie image after image in
    rank order: ``image``, ``rank``, ``index`` (the input position within the image) int32 [K], ``score`` float64 [K], ``kept_offset`` int64 [I + 1];
    ``match`` int32 [A, T, K] is the matched ground truth's input index within its image or -1, ``ignore`` bool [A, T, K] the detection's ignore flag,
    ``n_pos`` int32 [A] the number of non-ignored ground truths."""

    def __init__(self, image, rank, index, score, match, ignore, n_pos, kept_offset):
        self.image, self.rank, self.index, self.score, self.match, self.ignore, self.n_pos, self.kept_offset = image, rank, index, score, match, ignore, n_pos, kept_offset

    def __len__(self):
        return int(self.score.shape[0])

    def __repr__(self):
        return f"DetectionMatches(kept={len(self)}, area_ranges={self.match.shape[0]}, iou_thrs={self.match.shape[1]})"


def match_job(boxes: _BoxSet, iou_thrs, area_ranges, max_det, dev):
    """A ready vghev_box_match_job -> (job, dict of its output tensors, kept_offset on the host, the uploaded parameters, to be kept alive)."""
    T, A = len(iou_thrs), len(area_ranges)
    kept_offset = np.zeros(boxes.n + 1, dtype=np.int64)
    if boxes.n:
        np.cumsum(np.minimum(np.diff(boxes.dt_offset), max_det), out=kept_offset[1:])
    K = int(kept_offset[-1])
    if K > _lib_eval.MAX_KEPT:
        raise ValueError(f"{K} kept detections exceed {_lib_eval.MAX_KEPT}")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    out = {"image": i32(K), "rank": i32(K), "index": i32(K), "score": torch.empty((K,), dtype=torch.float64, device=dev), "match": i32(A, T, K),
           "ignore": torch.empty((A, T, K), dtype=torch.uint8, device=dev), "n_pos": torch.zeros((A,), dtype=torch.int32, device=dev),
           "status": torch.zeros((1,), dtype=torch.int32, device=dev)}  # a set without images queues nothing: these two stay as they are
    params = {"iou_thr": torch.from_numpy(iou_thrs).to(dev), "area_rng": torch.from_numpy(area_ranges).to(dev),
              "kept_offset": torch.from_numpy(kept_offset.astype(np.int32)).to(dev)}
    job = _lib_eval.BoxMatchJob()
    job.set = boxes.upload(dev)
    job.n_iou_thr, job.n_area, job.max_det, job.n_kept = T, A, max_det, K
    job.iou_thr_dev, job.area_rng_dev, job.kept_offset_dev = (params[k].data_ptr() for k in ("iou_thr", "area_rng", "kept_offset"))
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    job.match_dev, job.ignore_dev, job.det_image_dev, job.det_rank_dev, job.det_index_dev, job.det_score_dev = (
        ptr(out[k]) for k in ("match", "ignore", "image", "rank", "index", "score"))
    job.n_pos_dev, job.status_dev = out["n_pos"].data_ptr(), out["status"].data_ptr()
    return job, out, kept_offset, params


def _match(boxes: _BoxSet, iou_thrs, area_ranges, max_det, dev):
    """-> (dict of GPU tensors, kept_offset on the host)."""
    job, out, kept_offset, params = match_job(boxes, iou_thrs, area_ranges, max_det, dev)
    _run("vghev_box_match", job, dev)
    _check_status(out["status"], "match_detections")  # also waits for the kernels, so the uploads (boxes.dev, params) may go
    return out, kept_offset


def pr_job(m, n_kept, n_iou_thr, rec_thrs, n_area, max_dets, dev):
    """A ready vghev_pr_job from ``match_job``'s outputs -> (job, precision, scores, recall GPU tensors, what has to be kept alive)."""
    T, R, A, M, K = n_iou_thr, len(rec_thrs), n_area, len(max_dets), n_kept
    need = int(_lib_eval.load().vghev_ap_scratch_bytes(K))
    if need < 0:
        _lib_eval.check(need)
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    rec = torch.from_numpy(rec_thrs).to(dev)
    precision = torch.empty((T, R, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, A, M), dtype=torch.float64, device=dev)
    job = _lib_eval.PrJob()
    job.n_kept, job.n_iou_thr, job.n_rec_thr, job.n_area, job.n_max_dets = K, T, R, A, M
    for k, v in enumerate(max_dets):
        job.max_dets[k] = v
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    job.rec_thr_dev, job.match_dev, job.ignore_dev, job.det_rank_dev, job.det_score_dev = rec.data_ptr(), ptr(m["match"]), ptr(m["ignore"]), ptr(m["rank"]), ptr(m["score"])
    job.n_pos_dev, job.scratch_dev, job.scratch_bytes = m["n_pos"].data_ptr(), scratch.data_ptr(), scratch.numel()
    job.precision_dev, job.scores_dev, job.recall_dev = precision.data_ptr(), scores.data_ptr(), recall.data_ptr()
    return job, precision, scores, recall, (scratch, rec)


def match_detections(detections, ground_truth, iou_thrs=None, area_ranges=None, max_det: int = 100, gt_area=None, gt_crowd=None, to_host: bool = True) -> DetectionMatches:
    """``COCOeval.evaluate`` for one category: per image the detections ordered by score and cut to ``max_det``, and for every area range and IoU
    threshold the greedy matching include/vgh_eval.h states -> ``DetectionMatches``.

    ``detections`` and ``ground_truth`` are lists over the images of ``[n, 5]`` rows ``x, y, w, h, score`` and ``[n, 4]`` rows ``x, y, w, h`` (an image
    without any: an empty list).  ``gt_area`` (default ``w * h``, what the reference writes) and ``gt_crowd`` (default none) are lists over the images
    too.  ``iou_thrs`` (default .5 : .05 : .95, at most 16), ``area_ranges`` ([A, 2], default all / small / medium / large, at most 8), ``max_det`` at
    most 1 024, at most 4 096 ground truths per image and 2^20 images."""
    iou_thrs = _thresholds(iou_thrs, default_iou_thrs, _lib_eval.MAX_IOU_THR, "iou_thrs")
    area_ranges = _area_ranges(area_ranges)
    (max_det,) = _max_dets((max_det,))
    boxes = _BoxSet(detections, ground_truth, gt_area, gt_crowd)
    dev = _device_of(detections, ground_truth)
    out, kept_offset = _match(boxes, iou_thrs, area_ranges, max_det, dev)
    out["ignore"] = out["ignore"].to(torch.bool)
    if to_host:
        out = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        kept_offset = torch.from_numpy(kept_offset).to(dev)
    return DetectionMatches(out["image"], out["rank"], out["index"], out["score"], out["match"], out["ignore"], out["n_pos"], kept_offset)


# ---- AP ------------------------------------------------------------------------------------------------------------------------------------------------
def summarize_stats(precision: np.ndarray, recall: np.ndarray, iou_thrs: np.ndarray, max_dets) -> np.ndarray:
    """COCOeval.summarize's twelve numbers from the host arrays, each ``np.mean(x[x > -1])`` or -1 if nothing is left, as it forms them:
    AP, AP@.5, AP@.75, AP small / medium / large (all at the last of ``max_dets``), AR at ``max_dets[0]``, ``[1]`` and the last, AR small / medium / large.
    The area ranges are taken by position (all, small, medium, large); an entry whose IoU threshold, range or ``max_dets`` position is absent is -1."""
    T, _, A, M = precision.shape

    def one(ap, iou=None, a=0, k=M - 1):
        if a >= A or k >= M:
            return -1.0
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == iou_thrs)[0]]
        s = s[:, :, a, k] if ap else s[:, a, k]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    return np.array([one(1), one(1, iou=.5), one(1, iou=.75), one(1, a=1), one(1, a=2), one(1, a=3), one(0, k=0), one(0, k=1), one(0), one(0, a=1),
                     one(0, a=2), one(0, a=3)])


class DetectionAP:
    """``precision`` [T, R, A, M], ``recall`` [T, A, M], ``scores`` [T, R, A, M] (float64, -1 where an area range holds no ground truth), ``n_pos`` int32
    [A]: NumPy, or GPU tensors with ``to_host=False``.  ``stats`` (NumPy, always formed on the host) holds COCOeval's twelve numbers in ``summarize``'s
    order and ``ap = stats[0]`` is the number the reference prints as "mAP"."""

    def __init__(self, precision, recall, scores, n_pos, stats, iou_thrs, rec_thrs, area_ranges, max_dets):
        self.precision, self.recall, self.scores, self.n_pos, self.stats = precision, recall, scores, n_pos, stats
        self.iou_thrs, self.rec_thrs, self.area_ranges, self.max_dets = iou_thrs, rec_thrs, area_ranges, max_dets

    @property
    def ap(self) -> float:
        return float(self.stats[0])

    def summary(self) -> list:
        """The twelve lines in COCOeval's wording."""
        span = f"{self.iou_thrs[0]:0.2f}:{self.iou_thrs[-1]:0.2f}"
        last = self.max_dets[-1]
        rows = [(1, span, "all", last), (1, "0.50", "all", last), (1, "0.75", "all", last), (1, span, "small", last), (1, span, "medium", last),
                (1, span, "large", last), (0, span, "all", self.max_dets[0]), (0, span, "all", self.max_dets[1] if len(self.max_dets) > 1 else last),
                (0, span, "all", last), (0, span, "small", last), (0, span, "medium", last), (0, span, "large", last)]
        return [" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, k, v) for (ap, iou, area, k), v in zip(rows, self.stats)]

    def __repr__(self):
        return f"DetectionAP(ap={self.ap:.4f}, n_pos={[int(v) for v in self.n_pos]}, max_dets={self.max_dets})"


def check_ap_arguments(iou_thrs=None, rec_thrs=None, area_ranges=None, max_dets=(1, 10, 100)):
    """Validates what needs no GPU -> (iou_thrs [T], rec_thrs [R], area_ranges [A, 2], max_dets tuple)."""
    return (_thresholds(iou_thrs, default_iou_thrs, _lib_eval.MAX_IOU_THR, "iou_thrs"), _thresholds(rec_thrs, default_rec_thrs, _lib_eval.MAX_REC_THR, "rec_thrs"),
            _area_ranges(area_ranges), _max_dets(max_dets))


def average_precision(detections, ground_truth, iou_thrs=None, rec_thrs=None, area_ranges=None, max_dets=(1, 10, 100), gt_area=None, gt_crowd=None,
                      to_host: bool = True) -> DetectionAP:
    """``COCOeval(gt, dt, 'bbox')``'s evaluate, accumulate and summarize for one category -> ``DetectionAP``; ``.ap`` is the reference's "mAP".

    Arguments as ``match_detections``; ``rec_thrs`` defaults to 0 : .01 : 1 (at most 1 024), ``max_dets`` to COCOeval's (1, 10, 100) (ascending, at
    most 4 values of at most 1 024).  NOTE the module docstring's quirk: with the default only the 100 best detections of an image count, which the
    reference inherits on WIDER's crowds; ``max_dets=(1, 10, 1000)`` is the intended reading.  The matching and the curves run on the device;
    ``stats`` is formed on the host from the device's arrays exactly as ``summarize`` forms it."""
    iou_thrs, rec_thrs, area_ranges, max_dets = check_ap_arguments(iou_thrs, rec_thrs, area_ranges, max_dets)
    boxes = _BoxSet(detections, ground_truth, gt_area, gt_crowd)
    dev = _device_of(detections, ground_truth)
    m, kept_offset = _match(boxes, iou_thrs, area_ranges, max_dets[-1], dev)
    job, precision, scores, recall, hold = pr_job(m, int(kept_offset[-1]), len(iou_thrs), rec_thrs, len(area_ranges), max_dets, dev)
    _run("vghev_pr_accumulate", job, dev)
    p_host, r_host = precision.cpu().numpy(), recall.cpu().numpy()  # waits for the kernels: scratch and the match arrays may go
    stats = summarize_stats(p_host, r_host, iou_thrs, max_dets)
    if to_host:
        return DetectionAP(p_host, r_host, scores.cpu().numpy(), m["n_pos"].cpu().numpy(), stats, iou_thrs, rec_thrs, area_ranges, max_dets)
    return DetectionAP(precision, recall, scores, m["n_pos"], stats, iou_thrs, rec_thrs, area_ranges, max_dets)


class DetectionEvaluator:
    """Collects a test set image by image, as the reference's evaluators fill their ``result`` dictionary, and evaluates it in one go.

    ``add(predictions, gt_xywh, key=None, gt_area=None, gt_crowd=None)``: ``predictions`` is a ``PredictionResult`` (its ``detection_rows()`` are taken) or ``[n, 5]`` rows
    ``x, y, w, h, score``; ``gt_xywh`` the image's ``[n, 4]`` annotations, ``gt_area`` [n] (default ``w * h``) and ``gt_crowd`` [n] (default none) their
    areas and crowd flags as in ``average_precision``.  An image added again under the same ``key`` replaces the earlier entry (a
    dictionary, like the reference's); without a key every call adds an image.  ``evaluate()`` -> ``DetectionAP``; ``reset()`` forgets everything.
    The options are ``average_precision``'s and are validated at construction."""

    def __init__(self, iou_thrs=None, rec_thrs=None, area_ranges=None, max_dets=(1, 10, 100), to_host: bool = True):
        self.iou_thrs, self.rec_thrs, self.area_ranges, self.max_dets = check_ap_arguments(iou_thrs, rec_thrs, area_ranges, max_dets)
        self.to_host = to_host
        self.reset()

    def reset(self) -> None:
        self._images = {}
        self._auto = 0

    def __len__(self):
        return len(self._images)

    def add(self, predictions, gt_xywh, key=None, gt_area=None, gt_crowd=None) -> None:
        rows = predictions.detection_rows() if hasattr(predictions, "detection_rows") else predictions
        rows, gt = _rows(rows, 5, "predictions"), _rows(gt_xywh, 4, "gt_xywh")
        if len(gt) > _lib_eval.MAX_GT_PER_IMAGE:
            raise ValueError(f"an image holds {len(gt)} ground truths, more than {_lib_eval.MAX_GT_PER_IMAGE}")
        area = gt[:, 2] * gt[:, 3] if gt_area is None else _host(gt_area).reshape(-1)  # the default of the device: w * h, one float64 product
        crowd = np.zeros(len(gt), dtype=np.uint8) if gt_crowd is None else (_host(gt_crowd, None).reshape(-1) != 0).astype(np.uint8)
        if len(area) != len(gt) or len(crowd) != len(gt) or not np.isfinite(area).all():
            raise ValueError(f"gt_area and gt_crowd must hold one finite number and one flag per ground truth ({len(gt)}), got {len(area)} and {len(crowd)}")
        if key is None:
            key = ("#", self._auto)
            self._auto += 1
        self._images[key] = (rows, gt, area, crowd)

    def evaluate(self) -> DetectionAP:
        columns = list(zip(*self._images.values())) or [[], [], [], []]
        return average_precision(columns[0], columns[1], self.iou_thrs, self.rec_thrs, self.area_ranges, self.max_dets, gt_area=columns[2], gt_crowd=columns[3],
                                 to_host=self.to_host)


# ---- the evaluators' host helpers ----------------------------------------------------------------------------------------------------------------------
def rows_from_xyxy(boxes_xyxy, scores) -> list:
    """``parse_predictions`` of both evaluators: every ``x1, y1, x2, y2`` box is truncated with ``int()`` (towards zero), then
    ``[x1, y1, x2 - x1, y2 - y1, float(score)]``."""
    boxes = _host(boxes_xyxy).reshape(-1, 4) if np.size(_host(boxes_xyxy)) else np.zeros((0, 4))
    scores = _host(scores).reshape(-1)
    if len(boxes) != len(scores):
        raise ValueError(f"{len(boxes)} boxes but {len(scores)} scores")
    if not (np.isfinite(boxes).all() and np.isfinite(scores).all()):
        raise ValueError("boxes and scores must be finite")
    out = []
    for box, score in zip(boxes, scores):
        x1, y1, x2, y2 = (int(v) for v in box)
        out.append([x1, y1, x2 - x1, y2 - y1, float(score)])
    return out


def sanitize_predictions(rows, image_shape) -> list:
    """What FDDB's evaluator does to its rows before scoring them: every ``[x, y, w, h, score]`` box is cut to the image ``image_shape = (H, W, ...)``.
    Both corners, ``(x, y)`` and ``(x + w, y + h)``, are moved into ``[0, W] x [0, H]`` and the size is what lies between them, so a box outside the
    image keeps a corner on its border and a size of 0.  Integer rows (what ``rows_from_xyxy`` makes) stay integers."""
    shape = tuple(image_shape)
    if len(shape) < 2:
        raise ValueError(f"image_shape must be (H, W, ...), got {shape}")
    limit = (shape[1], shape[0])  # x runs to the width, y to the height

    def inside(value, axis):
        return 0 if value < 0 else (limit[axis] if value > limit[axis] else value)

    out = []
    for row in rows:
        if len(row) != 5:
            raise ValueError(f"a row must be [x, y, w, h, score], got {list(row)}")
        near = [inside(row[axis], axis) for axis in (0, 1)]
        far = [inside(row[axis] + row[axis + 2], axis) for axis in (0, 1)]
        out.append([near[0], near[1], far[0] - near[0], far[1] - near[1], row[4]])
    return out


def read_wider_annotations(path) -> dict:
    """WIDER FACE's ``wider_face_val_bbx_gt.txt`` -> {file name: [[x, y, w, h], ...]}, in the file's order.  A record is the image's name, the number of
    its boxes, and one line per box that starts with ``x y w h`` (the attribute flags behind them are dropped).  A record with 0 boxes still carries one
    placeholder box line, which is skipped -- the three-line step of the reference's reader."""
    with open(path, "r") as f:
        records = iter(f.read().splitlines())
    annotations = {}
    for name in records:
        name = name.strip()
        if not name:
            continue
        count = int(next(records))
        box_lines = [next(records, "") for _ in range(max(count, 1))]
        annotations[name] = [[int(field) for field in text.split()[:4]] for text in box_lines[:count]]
    return annotations


def read_fddb_annotations(path) -> dict:
    """The FDDB ``label.txt`` of the reference's evaluator -> {file name: [[x, y, w, h], ...]}, in the file's order.  A ``# name`` line opens an image;
    the lines below it hold the corners ``left top right bottom`` of one box each, returned as corner and size."""
    annotations = {}
    boxes = None
    with open(path, "r") as f:
        for text in f:
            fields = text.split()
            if not fields:
                continue
            if fields[0].startswith("#"):
                boxes = annotations.setdefault(text.strip().lstrip("#").strip(), [])
                continue
            if boxes is None or len(fields) != 4:
                raise ValueError(f"{path}: {text.strip()!r} is neither a '# name' line nor four corners below one")
            left, top, right, bottom = (int(field) for field in fields)
            boxes.append([left, top, right - left, bottom - top])
    return annotations
