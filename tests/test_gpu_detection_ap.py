"""COCO-style box evaluation on the MI355X: csrc/detection_ap.hip (libvgheval.so) through ``head_detector_amd.detection_metrics`` against the NumPy
float64 restatement tests/detection_ap_ref.py.  Every comparison is BITWISE: every float is a single IEEE float64 operation in a stated order or an
exact scan, so there is no tolerance anywhere.  The seeded sets (detection_ap_ref.seeded_set) are integer boxes on a coarse grid with few scores, so
that equal IoUs, equal scores, touching and zero-area boxes and areas exactly on the borders of the area ranges are frequent, with ground-truth counts
on either side of a wave and detection counts on either side of the default cut."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detection_ap_ref as ref  # noqa: E402

from head_detector_amd import detection_metrics as dm  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.head_info import RPY, Bbox, HeadMetadata  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float64:
        got, want = got.view(np.int64), want.view(np.int64)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, f"{bad.size} of {got.size} differ, first at {np.unravel_index(bad[0], got.shape)}")


def same_ap(got, want, what):
    for key in ("precision", "recall", "scores", "n_pos", "stats"):
        same_bits(getattr(got, key), want[key], (what, key))


def same_matches(got, want, what):
    for key in ("image", "rank", "index", "score", "match", "ignore", "n_pos"):
        same_bits(getattr(got, key), want[key], (what, key))


_sets = {}


def seeded(name):
    """The set and its restated evaluation, computed once."""
    if name not in _sets:
        dt, gt, crowd, max_dets = ref.seeded_set(name)
        _sets[name] = (dt, gt, crowd, max_dets, ref.evaluate(dt, gt, max_dets=max_dets, gt_crowd=crowd))
    return _sets[name]


def iou_boxes(nd, ng, seed):
    rng = np.random.default_rng(seed)
    dt, gt, crowd = ref.seeded_image(rng, ng, nd)
    dt = dt[:, :4]
    if nd >= 5 and ng >= 5:
        gt[0] = [40, 40, 32, 32]
        dt[0] = [72, 40, 8, 8]  # touches gt 0: w == 0
        dt[1] = [48, 48, 8, 8]  # nested in gt 0
        dt[2] = [48, 48, 0, 8]  # zero area inside gt 0
        dt[3] = [40, 40, 32, 32]  # gt 0 itself
        gt[1] = [48, 48, 0, 0]
        crowd[:3] = (0, 1, 1)
        gt[2] = [32, 32, 64, 64]  # a crowd box around dt 1: IoU = i / da = 1
    return dt, gt, crowd


@pytest.mark.parametrize("nd,ng", [(1, 1), (63, 65), (100, 257), (0, 5), (5, 0)])
def test_box_iou(nd, ng):
    dt, gt, crowd = iou_boxes(nd, ng, 100 * nd + ng)
    want = ref.box_iou(dt, gt, crowd)
    if nd and ng:  # the vectorised restatement is the scalar one
        for d, g in ((0, 0), (nd - 1, ng - 1), (nd // 2, ng // 3)):
            assert want[d, g] == ref.iou_one(dt[d], gt[g], crowd[g])
    if nd >= 5 and ng >= 5:
        assert want[0, 0] == 0.0 and want[1, 0] == 64.0 / 1024.0 and want[2, 0] == 0.0 and want[3, 0] == 1.0 and want[1, 2] == 1.0
    same_bits(dm.box_iou(dt, gt, crowd), want, "with crowd flags")
    same_bits(dm.box_iou(dt, gt), ref.box_iou(dt, gt), "without")


@pytest.mark.parametrize("name", ["one", "three", "many", "large", "mixed"])
def test_matching_and_curves(name):
    """"one", "three" and "many" stay inside the kernel's 512-entry LDS variant; "large" (513 and 1 100 ground truths) and "mixed" (small images around
    one with 513) run every image through the 4 096-entry one.  "many" and "mixed" each hold an image with more detections than their variant ranks in
    one tile of scores (2 500 > 2 048 and 17 000 > 16 384)."""
    dt, gt, crowd, max_dets, want = seeded(name)
    m = want["match"]
    if name == "large":  # ground truths far above position 512 are matched, crowd ones among the ignored
        assert m["match"].max() > 1024 and sum(int(c.sum()) for c in crowd) > 100
    if name == "mixed":
        assert max(len(g) for g in gt) == 513 and min(len(g) for g in gt) == 0
    for which, image, count, tile in (("many", 5, 2500, 2048), ("mixed", 7, 17000, 16384)):
        if name == which:  # detections of the later tiles are among the 100 kept, and all of them outrank one another across the tiles
            assert len(dt[image]) == count and max(len(g) for g in gt) <= tile // 4 and (m["index"][m["image"] == image] >= tile).any()
    # the sets do hit the rules they were built for
    assert (m["match"] >= 0).any() and m["ignore"].any() and (want["precision"] > 0).any()
    if name != "one":
        assert len(np.unique(m["score"])) < len(m["score"]) // 4
    same_matches(dm.match_detections(dt, gt, max_det=max_dets[-1], gt_crowd=crowd), m, name)
    same_ap(dm.average_precision(dt, gt, max_dets=max_dets, gt_crowd=crowd), want, name)


def test_an_understated_max_gt_is_reported():
    """The offsets live on the device, so the kernel checks every image against the job's max_gt: an image with more ground truths than the caller stated
    is left out, nothing of it is written, and the status word says so.  (detection_metrics always states the true maximum.)"""
    dt, gt, crowd, max_dets, want = seeded("mixed")
    dev = torch.device("cuda", 0)
    boxes = dm._BoxSet(dt, gt, gt_crowd=crowd)
    job, out, kept_offset, hold = dm.match_job(boxes, ref.IOU_THRS, ref.AREA_RANGES, max_dets[-1], dev)
    for key in ("match", "index"):
        out[key].fill_(-7)
    job.set.max_gt = 512  # the 513-ground-truth image no longer fits the variant this selects
    dm._run("vghev_box_match", job, dev)
    assert int(out["status"].item()) != 0
    lo, hi = int(kept_offset[3]), int(kept_offset[4])
    match, index = out["match"].cpu().numpy(), out["index"].cpu().numpy()
    assert (match[:, :, lo:hi] == -7).all() and (index[lo:hi] == -7).all()
    keep = np.r_[0:lo, hi:len(index)]
    same_bits(match[:, :, keep], want["match"]["match"][:, :, keep], "the other images")
    same_bits(index[keep], want["match"]["index"][keep], "the other images' order")


def test_explicit_areas():
    """gt_area is the annotation's own number, not w * h."""
    dt, gt, crowd, max_dets, _ = seeded("three")
    area = [np.random.default_rng(5 + i).choice([512.0, 1024.0, 1025.0, 9216.0, 9217.0], len(g)) for i, g in enumerate(gt)]
    want = ref.evaluate(dt, gt, max_dets=max_dets, gt_area=area, gt_crowd=crowd)
    same_ap(dm.average_precision(dt, gt, max_dets=max_dets, gt_area=area, gt_crowd=crowd), want, "gt_area")


@pytest.mark.parametrize("name", ref.PLANTED)
def test_planted(name):
    dt, gt, options = ref.planted(name)
    want = ref.evaluate(dt, gt, **options)
    same_ap(dm.average_precision(dt, gt, **options), want, name)
    same_matches(dm.match_detections(dt, gt, max_det=options.get("max_dets", (100,))[-1]), want["match"], name)


def test_single_threshold_range_and_max_det():
    dt, gt, crowd, _, _ = seeded("many")
    options = dict(iou_thrs=[0.3], rec_thrs=[0.2, 0.0, 0.03, 1.0, 0.06, 0.07, 2.0], area_ranges=[[1024.0, 9216.0]], max_dets=(7,))
    want = ref.evaluate(dt, gt, gt_crowd=crowd, **options)
    got = dm.average_precision(dt, gt, gt_crowd=crowd, **options)
    assert got.precision.shape == (1, 7, 1, 1) and got.recall.shape == (1, 1, 1) and got.stats.shape == (12,)
    # seven detections per image reach a recall just under 0.1: the unsorted thresholds 0, .03, .06 and .07 open at four different positions, the others never
    reached = np.array(options["rec_thrs"]) <= want["recall"][0, 0, 0]
    assert reached.tolist() == [False, True, True, False, True, True, False] and ((want["precision"][0, :, 0, 0] > 0) == reached).all()
    assert len(set(want["scores"][0, :, 0, 0])) == 5
    same_ap(got, want, "T = A = M = 1")


def test_gpu_tensors_and_two_calls():
    dt, gt, crowd, max_dets, want = seeded("three")
    dev = torch.device("cuda", 0)
    dt_t = [torch.from_numpy(d).to(dev) for d in dt]
    gt_t = [torch.from_numpy(g).to(dev) for g in gt]
    first = dm.average_precision(dt_t, gt_t, max_dets=max_dets, gt_crowd=crowd, to_host=False)
    second = dm.average_precision(dt_t, gt_t, max_dets=max_dets, gt_crowd=crowd, to_host=False)
    for key in ("precision", "recall", "scores", "n_pos"):
        a, b = getattr(first, key), getattr(second, key)
        assert isinstance(a, torch.Tensor) and a.is_cuda and torch.equal(a, b), key
        same_bits(a.cpu().numpy(), want[key], key)
    same_bits(first.stats, want["stats"], "stats")
    m = dm.match_detections(dt_t, gt_t, max_det=max_dets[-1], gt_crowd=crowd, to_host=False)
    assert m.match.is_cuda and m.ignore.dtype == torch.bool
    same_bits(m.match.cpu().numpy(), want["match"]["match"], "match")
    iou = dm.box_iou(dt_t[0][:, :4], gt_t[0], to_host=False)
    assert iou.is_cuda
    same_bits(iou.cpu().numpy(), ref.box_iou(dt[0][:, :4], gt[0]), "iou")


def test_evaluator_with_prediction_results():
    dt, gt, _, _, _ = seeded("many")
    ev = dm.DetectionEvaluator(max_dets=(1, 10, 100))
    rows = []
    for i in range(0, 40):
        heads = [HeadMetadata(bbox=Bbox(x=int(r[0]), y=int(r[1]), w=int(r[2]), h=int(r[3])), score=np.float32(r[4]), flame_params=None, vertices_3d=None,
                              head_pose=RPY(0.0, 0.0, 0.0)) for r in dt[i]]
        result = PredictionResult(np.zeros((4, 4, 3), dtype=np.uint8), heads)
        rows.append(result.detection_rows())
        ev.add(result, gt[i], key=f"image {i}")
    ev.add(rows[3], gt[3], key="image 3")  # the same image again: replaced, not doubled
    assert len(ev) == 40
    want = dm.average_precision(rows, gt[:40])
    got = ev.evaluate()
    same_ap(got, {k: getattr(want, k) for k in ("precision", "recall", "scores", "n_pos", "stats")}, "evaluator")
    same_ap(got, ref.evaluate(rows, gt[:40]), "evaluator against the restatement")
    assert got.ap == got.stats[0] and len(got.summary()) == 12
    ev.reset()
    assert len(ev) == 0
    # areas and crowd flags go through the evaluator as through average_precision
    dt, gt, crowd, max_dets, want = seeded("three")
    ev = dm.DetectionEvaluator(max_dets=max_dets)
    for d, g, c in zip(dt, gt, crowd):
        ev.add(d, g, gt_crowd=c)
    same_ap(ev.evaluate(), want, "evaluator with crowd flags")
    area = [np.full(len(g), 2000.0) for g in gt]
    ev.reset()
    for d, g, c, a in zip(dt, gt, crowd, area):
        ev.add(d, g, gt_area=a, gt_crowd=c)
    same_ap(ev.evaluate(), ref.evaluate(dt, gt, max_dets=max_dets, gt_area=area, gt_crowd=crowd), "evaluator with areas")
