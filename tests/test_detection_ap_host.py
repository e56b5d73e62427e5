"""COCO-style box evaluation, the part that needs no GPU: the NumPy restatement tests/detection_ap_ref.py (what the device is held to, bitwise, in
tests/test_gpu_detection_ap.py) on cases worked by hand below, the host helpers of ``head_detector_amd.detection_metrics`` restated from the reference's
two detection benchmarks on the hand-written files of tests/golden/detection/, and the argument checks of every public function."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import detection_ap_ref as ref  # noqa: E402

from head_detector_amd import _lib_eval, detection_metrics as dm  # noqa: E402
from head_detector_amd.detection_result import PredictionResult  # noqa: E402
from head_detector_amd.head_info import RPY, Bbox, HeadMetadata  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection")
EPS = 2.220446049250313e-16
ONE = 1.0 / (1.0 + EPS)  # the precision of a lone true positive: 1 - 2^-52, not 1


def run(name, **more):
    dt, gt, options = ref.planted(name)
    return ref.evaluate(dt, gt, **{**options, **more})


def test_constants():
    assert EPS == np.spacing(1) and ONE == 1.0 - 2.0 ** -52
    assert np.array_equal(ref.IOU_THRS, np.linspace(.5, .95, 10)) and np.array_equal(ref.IOU_THRS, dm.default_iou_thrs())
    assert np.array_equal(ref.REC_THRS, np.linspace(0, 1, 101)) and np.array_equal(ref.REC_THRS, dm.default_rec_thrs())
    assert np.array_equal(ref.AREA_RANGES, [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]) and np.array_equal(ref.AREA_RANGES, dm.default_area_ranges())
    assert ref.REC_THRS[50] == 0.5


def test_tp_fp_tp():
    """Two ground truths, detections TP, FP, TP in score order.  At every IoU threshold (the IoUs are 1): tp = 1, 1, 2 and fp = 0, 1, 1, so
    rc = .5, .5, 1 and pr = 1/(1+eps), 1/(2+eps), 2/(3+eps); from the right the running maximum is 1/(1+eps), 2/(3+eps), 2/(3+eps).  The 51 recall
    thresholds 0 .. .50 find position 0, the 50 thresholds .51 .. 1 position 2: AP = (51 * 1/(1+eps) + 50 * 2/(3+eps)) / 101."""
    r = run("tp_fp_tp")
    p = r["precision"][0, :, 0, 2]
    assert np.array_equal(p[:51], np.full(51, ONE)) and np.array_equal(p[51:], np.full(50, 2.0 / (3.0 + EPS)))
    assert np.array_equal(r["scores"][0, :51, 0, 2], np.full(51, 0.9)) and np.array_equal(r["scores"][0, 51:, 0, 2], np.full(50, 0.7))
    want = (51 * 1.0 + 50 * (2.0 / (3.0 + EPS))) / 101
    assert abs(r["stats"][1] - want) < 1e-14 and abs(r["stats"][0] - want) < 1e-14
    assert r["n_pos"].tolist() == [2, 2, 0, 0] and r["stats"][4] == -1 and r["stats"][5] == -1
    # max_dets = 1: only the best detection counts: recall .5; max_dets = 10: all three
    assert r["recall"][0, 0].tolist() == [0.5, 1.0, 1.0] and r["stats"][6] == 0.5 and r["stats"][7] == 1.0 and r["stats"][8] == 1.0
    m = r["match"]
    assert m["index"].tolist() == [0, 1, 2] and m["match"][0, 0].tolist() == [0, -1, 1] and not m["ignore"][0].any()
    assert m["ignore"][2, 0].tolist() == [True, True, True]  # "medium": matched to an ignored ground truth, or unmatched and itself too small


def test_perfect_detections():
    """Six images with one ground truth each, two per size class, each found exactly: every area range holds at least two true positives and no false
    one, so pr ends on 2/(2+eps) = 1 exactly (2 + eps rounds to 2) and the running maximum carries it to the front; one detection per image, so
    AR at max_dets = 1 is 1 as well."""
    r = run("perfect")
    assert r["n_pos"].tolist() == [6, 2, 2, 2] and np.array_equal(r["stats"], np.ones(12))
    assert (r["precision"] == 1.0).all() and (r["recall"] == 1.0).all()


def test_no_detections():
    r = run("no_detections")
    assert r["n_pos"].tolist() == [3, 1, 1, 1] and np.array_equal(r["stats"], np.zeros(12))
    assert (r["precision"] == 0.0).all() and (r["recall"] == 0.0).all() and (r["scores"] == 0.0).all()


def test_no_ground_truth_in_a_range():
    """Both ground truths are small; the one detection finds the first: recall .5 and precision 1/(1+eps) up to it."""
    r = run("small_only")
    assert r["n_pos"].tolist() == [2, 2, 0, 0]
    assert (r["precision"][:, :, 2:] == -1).all() and (r["recall"][:, 2:] == -1).all() and (r["scores"][:, :, 2:] == -1).all()
    assert r["stats"][[4, 5, 10, 11]].tolist() == [-1, -1, -1, -1] and r["stats"][8] == 0.5
    assert np.array_equal(r["precision"][0, :, 1, 2], np.where(ref.REC_THRS <= 0.5, ONE, 0.0))
    # no ground truth at all: everything is -1
    r = ref.evaluate([[[0, 0, 5, 5, 0.5]]], [[]])
    assert np.array_equal(r["stats"], -np.ones(12)) and r["n_pos"].tolist() == [0, 0, 0, 0]


def test_ignored_match_is_neither_tp_nor_fp():
    """In "small" the large ground truth is ignored.  The best detection matches it and becomes ignored itself; the second finds the small one.  So
    tp = 0, 1 and fp = 0, 0: precision 1/(1+eps) at every recall.  Were the first a false positive it would be 1/(2+eps)."""
    r = run("ignored_match")
    m = r["match"]
    assert m["match"][1, 0].tolist() == [1, 0] and m["ignore"][1, 0].tolist() == [True, False]
    assert np.array_equal(r["precision"][:, :, 1, 2], np.full((10, 101), ONE)) and (r["recall"][:, 1, 2] == 1.0).all()
    assert m["ignore"][3, 0].tolist() == [False, True]  # "large": the second one matches an ignored ground truth
    assert m["match"][2, 0].tolist() == [1, 0] and r["n_pos"].tolist() == [2, 1, 0, 1]


def test_equal_iou_takes_the_later_ground_truth():
    """Both IoUs are 100 / ((100 + 200) - 100) = .5 exactly: the walk's ">=" moves on to the second.  At the thresholds above .5 nothing matches."""
    dt, gt, _ = ref.planted("equal_iou")
    assert ref.iou_one(dt[0][0][:4], gt[0][0], False) == 0.5 == ref.iou_one(dt[0][0][:4], gt[0][1], False)
    r = run("equal_iou")
    assert r["match"]["match"][0, :, 0].tolist() == [1] + [-1] * 9
    assert r["match"]["match"][0, :, 0].tolist() == run("equal_iou", fast=False)["match"]["match"][0, :, 0].tolist()
    # a crowd ground truth can be matched again, any other only once
    two = [[[0, 0, 10, 10, 0.9], [0, 0, 10, 10, 0.8]]]
    assert ref.evaluate(two, [[[0, 0, 10, 10]]])["match"]["match"][0, 0].tolist() == [0, -1]
    crowd = ref.evaluate(two, [[[0, 0, 10, 10]]], gt_crowd=[[1]])
    assert crowd["match"]["match"][0, 0].tolist() == [0, 0] and crowd["match"]["ignore"][0, 0].tolist() == [True, True] and crowd["n_pos"][0] == 0


def test_rank_100_counts_only_with_larger_max_dets():
    """101 detections, the only true positive has the lowest score: rank 100.  COCOeval's default keeps ranks 0 .. 99: recall 0, AP 0.  With
    max_dets = (1, 10, 1000) it counts: recall 1 and precision 1/(101+eps) at every recall threshold."""
    r = run("rank_100")
    assert len(r["match"]["score"]) == 100 and r["stats"][0] == 0.0 and r["stats"][8] == 0.0 and (r["recall"][:, 0, 2] == 0.0).all()
    r = run("rank_100_counted")
    assert len(r["match"]["score"]) == 101 and r["match"]["index"][100] == 100 and r["match"]["match"][0, 0, 100] == 0
    assert r["stats"][8] == 1.0 and r["stats"][7] == 0.0 and abs(r["stats"][0] - 1.0 / (101.0 + EPS)) < 1e-16
    assert np.array_equal(r["precision"][:, :, 0, 2], np.full((10, 101), 1.0 / (101.0 + EPS)))


def test_orders_and_the_fast_walk():
    """Equal scores keep their input order; the loop-free walk of the restatement is the worded one on sets full of ties; summarize is the module's."""
    order = ref.match_image([[0, 0, 1, 1, .5], [0, 0, 1, 1, .7], [0, 0, 1, 1, .5], [0, 0, 1, 1, .7]], [], None, None, ref.IOU_THRS, ref.AREA_RANGES, 3)[0]
    assert order.tolist() == [1, 3, 0]
    dt, gt, crowd, max_dets = ref.seeded_set("one")
    rng = np.random.default_rng(3)
    more = [ref.seeded_image(rng, ng, nd) for ng, nd in ((7, 30), (65, 40), (3, 0), (0, 4))]
    dt, gt, crowd = dt + [m[0] for m in more], gt + [m[1] for m in more], crowd + [m[2] for m in more]
    fast, slow = ref.evaluate(dt, gt, gt_crowd=crowd), ref.evaluate(dt, gt, gt_crowd=crowd, fast=False)
    for key in ("match", "ignore", "index"):
        assert np.array_equal(fast["match"][key], slow["match"][key]), key
    assert np.array_equal(fast["precision"], slow["precision"]) and (fast["match"]["match"] >= 0).any() and fast["match"]["ignore"].any()
    # the module's summary against the restatement's entry-by-entry table (written apart; the planted cases above check both against hand numbers)
    assert np.array_equal(dm.summarize_stats(fast["precision"], fast["recall"], ref.IOU_THRS, max_dets), fast["stats"])
    for name in ref.PLANTED:
        r = run(name)
        assert np.array_equal(dm.summarize_stats(r["precision"], r["recall"], ref.IOU_THRS, ref.planted(name)[2].get("max_dets", (1, 10, 100))), r["stats"]), name
    one = ref.evaluate(dt, gt, gt_crowd=crowd, iou_thrs=[0.75], area_ranges=[[0, 1e10]], max_dets=(5,))
    assert np.array_equal(dm.summarize_stats(one["precision"], one["recall"], np.array([0.75]), (5,)), one["stats"])
    assert one["stats"][1] == -1 and one["stats"][2] == one["stats"][0] and one["stats"][7] == -1 and one["stats"][6] == one["stats"][8] and one["stats"][3] == -1
    # areas exactly on a border belong to both neighbours
    r = ref.evaluate([[]], [[[0, 0, 32, 32], [0, 0, 96, 96], [0, 0, 64, 16]]])
    assert r["n_pos"].tolist() == [3, 2, 3, 1]


def test_summary_wording():
    r = run("tp_fp_tp")
    ap = dm.DetectionAP(r["precision"], r["recall"], r["scores"], r["n_pos"], r["stats"], ref.IOU_THRS, ref.REC_THRS, ref.AREA_RANGES, (1, 10, 100))
    lines = ap.summary()
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.835"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
    assert len(lines) == 12 and ap.ap == r["stats"][0] and "DetectionAP" in repr(ap)


def test_rows_from_xyxy_and_sanitize():
    rows = dm.rows_from_xyxy(np.array([[10.9, 20.2, 30.7, 45.5], [-3.7, -0.2, 5.9, 6.1]], dtype=np.float32), np.array([0.75, 0.25], dtype=np.float32))
    assert rows == [[10, 20, 20, 25, 0.75], [-3, 0, 8, 6, 0.25]]  # int() truncates towards zero; w = int(x2) - int(x1)
    assert all(isinstance(v, int) for v in rows[0][:4]) and isinstance(rows[0][4], float)
    assert dm.rows_from_xyxy([], []) == []
    with pytest.raises(ValueError):
        dm.rows_from_xyxy(np.zeros((2, 4)), np.zeros(3))
    with pytest.raises(ValueError):
        dm.rows_from_xyxy(np.array([[0, 0, np.nan, 1]]), np.zeros(1))
    # an image of height 100 and width 200: the corner is clamped, the size shrinks by what it moved, the far corner is clamped
    clean = dm.sanitize_predictions([[-10, -5, 30, 30, 0.5], [190, 90, 30, 30, 0.4], [20, 30, 40, 50, 0.3], [250, 120, 10, 10, 0.2]], (100, 200, 3))
    assert clean == [[0, 0, 20, 25, 0.5], [190, 90, 10, 10, 0.4], [20, 30, 40, 50, 0.3], [200, 100, 0, 0, 0.2]]
    assert all(isinstance(v, int) for row in clean for v in row[:4])
    assert dm.sanitize_predictions([[-1.5, 2.0, 4.0, 200.0, 0.5]], (100, 200)) == [[0, 2.0, 2.5, 98.0, 0.5]]
    with pytest.raises(ValueError):
        dm.sanitize_predictions([[0, 0, 1, 1]], (10, 10))
    with pytest.raises(ValueError):
        dm.sanitize_predictions([[0, 0, 1, 1, 0.5]], (10,))


def test_annotation_readers():
    wider = dm.read_wider_annotations(os.path.join(GOLDEN, "wider_face_val_bbx_gt.txt"))
    assert list(wider) == ["0--Parade/0_Parade_marchingband_1_465.jpg", "0--Parade/0_Parade_Parade_0_452.jpg", "1--Handshaking/1_Handshaking_Handshaking_1_94.jpg"]
    assert wider["0--Parade/0_Parade_marchingband_1_465.jpg"] == [[345, 211, 4, 4], [331, 126, 3, 3]]
    assert wider["0--Parade/0_Parade_Parade_0_452.jpg"] == []  # 0 boxes: its record still has a box line, three lines in all
    assert wider["1--Handshaking/1_Handshaking_Handshaking_1_94.jpg"] == [[78, 221, 7, 8], [78, 238, 14, 17], [113, 212, 11, 15]]
    fddb = dm.read_fddb_annotations(os.path.join(GOLDEN, "fddb_label.txt"))
    assert fddb == {"2002/08/11/big/img_591.jpg": [[184, 38, 171, 247]], "2002/08/26/big/img_265.jpg": [[40, 60, 70, 100], [200, 50, 81, 120]],
                    "2002/07/19/big/img_423.jpg": []}
    with open(os.path.join(GOLDEN, "fddb_label.txt")) as f:
        broken = f.read().replace("40 60 110 160", "40 60 110")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "label.txt"), "w") as f:
            f.write(broken)
        with pytest.raises(ValueError):
            dm.read_fddb_annotations(os.path.join(tmp, "label.txt"))
    # the readers' output is what the evaluation takes
    r = ref.evaluate([[b + [0.9] for b in boxes] for boxes in wider.values()], list(wider.values()))
    assert r["n_pos"][0] == 5 and r["stats"][0] == 1.0


def test_detection_rows():
    heads = [HeadMetadata(bbox=Bbox(x=3, y=4, w=10, h=12), score=np.float32(0.5), flame_params=None, vertices_3d=None, head_pose=RPY(0.0, 0.0, 0.0)),
             HeadMetadata(bbox=Bbox(x=7, y=8, w=2, h=1), score=0.25, flame_params=None, vertices_3d=None, head_pose=RPY(0.0, 0.0, 0.0))]
    rows = PredictionResult(np.zeros((4, 4, 3), dtype=np.uint8), heads).detection_rows()
    assert rows == [[3, 4, 10, 12, 0.5], [7, 8, 2, 1, 0.25]] and isinstance(rows[0][4], float)
    assert PredictionResult(np.zeros((4, 4, 3), dtype=np.uint8), []).detection_rows() == []


def test_argument_errors_need_no_gpu():
    """Everything is validated before a GPU is looked for."""
    dt, gt = [np.array([[0, 0, 5, 5, 0.5]])], [np.array([[0, 0, 5, 5.0]])]
    bad_options = (dict(max_dets=(10, 1, 100)), dict(max_dets=(1, 10, 1025)), dict(max_dets=(0, 1)), dict(max_dets=()), dict(max_dets=(1, 2, 3, 4, 5)),
                   dict(max_dets=(1.5,)), dict(iou_thrs=[]), dict(iou_thrs=np.linspace(0, 1, 17)), dict(iou_thrs=[[0.5]]), dict(iou_thrs=[np.nan]),
                   dict(rec_thrs=np.linspace(0, 1, 1025)), dict(rec_thrs=[]), dict(area_ranges=[[0, 1, 2]]), dict(area_ranges=np.zeros((9, 2))),
                   dict(area_ranges=[0, 1]), dict(gt_area=[[1.0], [2.0]]), dict(gt_area=[[1.0, 2.0]]), dict(gt_crowd=[[0, 1]]), dict(gt_area=[[np.nan]]))
    for bad in bad_options:
        with pytest.raises(ValueError):
            dm.average_precision(dt, gt, **bad)
    nan_score = [np.array([[0, 0, 5, 5, np.nan]])]
    for call in (dm.average_precision, dm.match_detections):
        for bad in ((nan_score, gt), (dt, [np.array([[0, 0, np.inf, 5]])]), (dt, gt + gt), ([np.zeros((1, 4))], gt), (dt, [np.zeros((1, 5))]), (dt, [np.zeros((4097, 4))]),
                    ([np.zeros(5)], gt)):
            with pytest.raises(ValueError):
                call(*bad)
    for bad in (dict(max_det=0), dict(max_det=1025), dict(iou_thrs=[]), dict(area_ranges=[[1]])):
        with pytest.raises(ValueError):
            dm.match_detections(dt, gt, **bad)
    for bad in ((np.zeros((2, 5)), np.zeros((2, 4))), (np.zeros((2, 4)), np.zeros((4097, 4))), (np.zeros((2, 4)), np.zeros((3, 4)), [0, 1]),
                (np.full((1, 4), np.nan), np.zeros((1, 4)))):
        with pytest.raises(ValueError):
            dm.box_iou(*bad)
    with pytest.raises(ValueError):
        dm.DetectionEvaluator(max_dets=(100, 10))
    ev = dm.DetectionEvaluator()
    for bad in ((nan_score[0], gt[0]), (np.zeros((2, 4)), gt[0]), (dt[0], np.zeros((4097, 4)))):
        with pytest.raises(ValueError):
            ev.add(*bad)
    for bad in (dict(gt_crowd=[0, 1]), dict(gt_area=[1.0, 2.0]), dict(gt_area=[np.nan])):
        with pytest.raises(ValueError):
            ev.add(dt[0], gt[0], **bad)
    assert len(ev) == 0
    ev.add(dt[0], gt[0], gt_area=[25.0], gt_crowd=[1])
    ev.add([], [])
    assert len(ev) == 2


def test_library_checks_need_no_gpu():
    """The C entry points check sizes and pointers before anything is queued."""
    lib = _lib_eval.load()
    assert lib.vghev_ap_scratch_bytes(0) > 0 and lib.vghev_ap_scratch_bytes(1000) >= 1024 * 12 + 1000 * 12
    assert lib.vghev_ap_scratch_bytes(-1) == -1 and lib.vghev_ap_scratch_bytes(_lib_eval.MAX_KEPT + 1) == -1 and b"n_kept" in lib.vghev_last_error()
    job = _lib_eval.BoxMatchJob()
    job.set.n_images, job.set.max_gt, job.n_iou_thr, job.n_area, job.max_det = 1, 4097, 10, 4, 100
    assert lib.vghev_box_match(C.byref(job), None) == -1 and b"max_gt" in lib.vghev_last_error()
    job.set.max_gt, job.n_iou_thr = 10, 17
    assert lib.vghev_box_match(C.byref(job), None) == -1 and b"n_iou_thr" in lib.vghev_last_error()
    job.n_iou_thr, job.max_det = 10, 1025
    assert lib.vghev_box_match(C.byref(job), None) == -1 and b"max_det" in lib.vghev_last_error()
    job.max_det, job.set.n_images = 100, _lib_eval.MAX_IMAGES + 1
    assert lib.vghev_box_match(C.byref(job), None) == -1 and b"n_images" in lib.vghev_last_error()
    job.set.n_images = 1
    assert lib.vghev_box_match(C.byref(job), None) == -1 and b"NULL" in lib.vghev_last_error()
    iou = _lib_eval.BoxIouJob()
    iou.set.n_images, iou.n_iou = 1, -1
    assert lib.vghev_box_iou(C.byref(iou), None) == -1 and b"n_iou" in lib.vghev_last_error()
    iou.n_iou = 0
    assert lib.vghev_box_iou(C.byref(iou), None) == -1 and b"NULL" in lib.vghev_last_error()
    iou.set.n_images = 0
    assert lib.vghev_box_iou(C.byref(iou), None) == 0
    pr = _lib_eval.PrJob()
    pr.n_iou_thr, pr.n_rec_thr, pr.n_area, pr.n_max_dets = 10, 101, 4, 3
    pr.max_dets[0], pr.max_dets[1], pr.max_dets[2] = 10, 1, 100
    assert lib.vghev_pr_accumulate(C.byref(pr), None) == -1 and b"ascend" in lib.vghev_last_error()
    pr.max_dets[0], pr.max_dets[1] = 1, 10
    assert lib.vghev_pr_accumulate(C.byref(pr), None) == -1 and b"scratch" in lib.vghev_last_error()
    pr.scratch_bytes = 1 << 20
    assert lib.vghev_pr_accumulate(C.byref(pr), None) == -1 and b"NULL" in lib.vghev_last_error()
    pr.n_rec_thr = 1025
    assert lib.vghev_pr_accumulate(C.byref(pr), None) == -1 and b"n_rec_thr" in lib.vghev_last_error()
    assert lib.vghev_box_match(None, None) == -1 and lib.vghev_pr_accumulate(None, None) == -1 and lib.vghev_box_iou(None, None) == -1
