"""ctypes binding of libvgheval.so (include/vgh_eval.h): mesh and detection benchmark metrics.  A library of its own: none of libvgh.so, libvghview.so, libvghvis.so and
libvghtex.so knows of it, and their bindings do not load it; like them there is NO fallback: a missing library raises ``VghError``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._companion import load_library, raise_for
from ._lib import VghError  # noqa: F401 (callers name it through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvgheval.so")
MAX_HEADS = 1048576  # = VGHEV_MAX_HEADS
MAX_POINTS = 1048576  # = VGHEV_MAX_POINTS
MAX_TOP_K = 16  # = VGHEV_MAX_TOP_K
NEIGHBOURS = {"reference": 0, "nearest": 1}  # = VGHEV_NEIGHBOURS_REFERENCE, VGHEV_NEIGHBOURS_NEAREST
# detection AP (csrc/detection_ap.hip)
MAX_IMAGES = 1048576  # = VGHEV_MAX_IMAGES
MAX_GT_PER_IMAGE = 4096  # = VGHEV_MAX_GT_PER_IMAGE
MAX_DET = 1024  # = VGHEV_MAX_DET
MAX_KEPT = 1073741824  # = VGHEV_MAX_KEPT
MAX_IOU_THR = 16  # = VGHEV_MAX_IOU_THR
MAX_REC_THR = 1024  # = VGHEV_MAX_REC_THR
MAX_AREA_RNG = 8  # = VGHEV_MAX_AREA_RNG
MAX_MAX_DETS = 4  # = VGHEV_MAX_MAX_DETS


class ZOrderJob(C.Structure):
    """vghev_z_order_job: predicted and ground-truth points of n heads on the device and the agreement counts they give."""
    _fields_ = [("n_heads", C.c_int32), ("n_points", C.c_int32), ("top_k", C.c_int32), ("mode", C.c_int32), ("pred_dev", C.c_void_p), ("gt_dev", C.c_void_p),
                ("agree_dev", C.c_void_p)]


class NearestJob(C.Structure):
    """vghev_nearest_job: queries and points of n heads on the device, the optional per-head scales and transform, and the three outputs."""
    _fields_ = [("n_heads", C.c_int32), ("n_queries", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32), ("query_dev", C.c_void_p),
                ("query_scale_dev", C.c_void_p), ("points_dev", C.c_void_p), ("transform_dev", C.c_void_p), ("point_scale_dev", C.c_void_p),
                ("sqdist_dev", C.c_void_p), ("index_dev", C.c_void_p), ("mean_dev", C.c_void_p)]


class BoxSet(C.Structure):
    """vghev_box_set: detections and ground truth of I images in CSR form on the device."""
    _fields_ = [("n_images", C.c_int32), ("n_dt", C.c_int32), ("n_gt", C.c_int32), ("max_gt", C.c_int32), ("dt_box_dev", C.c_void_p),
                ("dt_score_dev", C.c_void_p), ("dt_offset_dev", C.c_void_p), ("gt_box_dev", C.c_void_p), ("gt_area_dev", C.c_void_p),
                ("gt_crowd_dev", C.c_void_p), ("gt_offset_dev", C.c_void_p)]


class BoxIouJob(C.Structure):
    """vghev_box_iou_job: the dense IoU block of every image."""
    _fields_ = [("set", BoxSet), ("n_iou", C.c_int64), ("iou_offset_dev", C.c_void_p), ("iou_dev", C.c_void_p), ("status_dev", C.c_void_p)]


class BoxMatchJob(C.Structure):
    """vghev_box_match_job: thresholds, area ranges and the per-(area range, threshold, kept detection) outputs of the matching."""
    _fields_ = [("set", BoxSet), ("n_iou_thr", C.c_int32), ("n_area", C.c_int32), ("max_det", C.c_int32), ("reserved", C.c_int32), ("n_kept", C.c_int64),
                ("iou_thr_dev", C.c_void_p), ("area_rng_dev", C.c_void_p), ("kept_offset_dev", C.c_void_p), ("match_dev", C.c_void_p),
                ("ignore_dev", C.c_void_p), ("det_image_dev", C.c_void_p), ("det_rank_dev", C.c_void_p), ("det_index_dev", C.c_void_p),
                ("det_score_dev", C.c_void_p), ("n_pos_dev", C.c_void_p), ("status_dev", C.c_void_p)]


class PrJob(C.Structure):
    """vghev_pr_job: the matching's outputs, the caller's scratch and the three curve arrays."""
    _fields_ = [("n_kept", C.c_int64), ("n_iou_thr", C.c_int32), ("n_rec_thr", C.c_int32), ("n_area", C.c_int32), ("n_max_dets", C.c_int32),
                ("max_dets", C.c_int32 * 4), ("rec_thr_dev", C.c_void_p), ("match_dev", C.c_void_p), ("ignore_dev", C.c_void_p),
                ("det_rank_dev", C.c_void_p), ("det_score_dev", C.c_void_p), ("n_pos_dev", C.c_void_p), ("scratch_dev", C.c_void_p),
                ("scratch_bytes", C.c_int64), ("precision_dev", C.c_void_p), ("scores_dev", C.c_void_p), ("recall_dev", C.c_void_p)]


# every symbol include/vgh_eval.h declares: (restype, argtypes)
SYMBOLS = {
    "vghev_version": (C.c_char_p, []),
    "vghev_last_error": (C.c_char_p, []),
    "vghev_z_order": (C.c_int, [C.POINTER(ZOrderJob), C.c_void_p]),
    "vghev_nearest": (C.c_int, [C.POINTER(NearestJob), C.c_void_p]),
    "vghev_box_iou": (C.c_int, [C.POINTER(BoxIouJob), C.c_void_p]),
    "vghev_box_match": (C.c_int, [C.POINTER(BoxMatchJob), C.c_void_p]),
    "vghev_pr_accumulate": (C.c_int, [C.POINTER(PrJob), C.c_void_p]),
    "vghev_ap_scratch_bytes": (C.c_int64, [C.c_int64]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libvgheval.so and bind every declared symbol. Raises VghError if the library is absent."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise_for(rc, "libvgheval", load().vghev_last_error)
