/* vgh_eval.h -- libvgheval.so: mesh and detection benchmark metrics for the MI355X head detector (gfx950 only).
 *
 * The fifth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so (include/vgh_view.h), libvghvis.so (include/vgh_vis.h)
 * and libvghtex.so (include/vgh_tex.h).  This one judges predicted heads against ground-truth meshes: the two neighbour searches behind the DAD-3DHeads
 * metrics Z_n and chamfer distance (yolo_head_training/evaluation/dad_utils.py of the reference: calc_zn, calc_ch_dist), for any number of heads in one
 * call, and detections against annotated boxes: the COCO-style box AP of the reference's head-detection benchmarks (further down).  It links no object
 * of the other four and none of them loads it.  Every export carries the prefix vghev_; everything else has hidden visibility.
 *
 * Conventions as in vgh_tex.h: functions return VGHEV_OK (0) or a negative code, vghev_last_error() gives the message of the calling thread's last
 * failure, `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 *
 * ARITHMETIC.  Coordinates arrive as float32 and every distance is a SQUARED distance in float64,
 *     dx = a.x - b.x (in float64), ...;   d = (dx * dx + dy * dy) + dz * dz
 * in exactly this order without contraction into fused multiply-adds.  Points are ordered by (distance, index): a tie goes to the lower index.  There
 * are no float atomics and no order that depends on scheduling: every output is bitwise deterministic.
 */
#ifndef VGH_EVAL_H
#define VGH_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHEV_API __attribute__((visibility("default")))
#else
#define VGHEV_API
#endif

#define VGHEV_OK 0
#define VGHEV_ERR_INVALID (-1)
#define VGHEV_ERR_HIP (-2)

#define VGHEV_MAX_HEADS 1048576
#define VGHEV_MAX_POINTS 1048576 /* per head, of every point set */
#define VGHEV_MAX_TOP_K 16

#define VGHEV_NEIGHBOURS_REFERENCE 0 /* calc_zn as written: its column slice of the row-wise argsort */
#define VGHEV_NEIGHBOURS_NEAREST 1   /* every vertex against its own top_k nearest */

/* Z_n (calc_zn) for n heads of N points.  With D[a][b] the distance between ground-truth points a and b of one head and rank(a, b) the number of
 * points q with (D[q][b], q) < (D[a][b], a), agree[head] counts the pairs (i, j), i < N, j < top_k, with
 *     (gt_z[i] >= gt_z[p]) == (pred_z[i] >= pred_z[p])          (float32 comparisons of the third coordinate)
 * for the partner p = p(i, j):
 *   REFERENCE  the point of rank i in column j + 1: rank(p, j + 1) = i.  This is what the source computes: it sorts with argsort(distances, dim=0) and
 *              then slices COLUMNS 1 .. top_k, so vertex i meets the i-th nearest point of vertex j + 1.
 *   NEAREST    the point of rank j + 1 in column i: the j + 1-th nearest point of vertex i itself (rank 0, normally i, is dropped as the source drops it).
 * Z_n of a head is agree / (N * top_k), formed by the caller.  Non-finite coordinates give an unspecified count, never an access outside the arrays. */
typedef struct vghev_z_order_job {
    int32_t n_heads;        /* 0 .. VGHEV_MAX_HEADS; 0 queues nothing */
    int32_t n_points;       /* N: top_k + 1 .. VGHEV_MAX_POINTS */
    int32_t top_k;          /* 1 .. VGHEV_MAX_TOP_K */
    int32_t mode;           /* VGHEV_NEIGHBOURS_REFERENCE or VGHEV_NEIGHBOURS_NEAREST */
    const float* pred_dev;  /* f32 [n_heads, N, 3] on the device; never written */
    const float* gt_dev;    /* f32 [n_heads, N, 3] on the device; never written */
    int32_t* agree_dev;     /* i32 [n_heads] on the device */
} vghev_z_order_job;

/* One-sided nearest neighbour for n heads: for every query the nearest point of the same head.
 *   query  q = (double)query * query_scale[head] per coordinate (query_scale_dev NULL: q = (double)query)
 *   point  transform_dev NULL: p = (double)point.  Otherwise with T = transform[head] ([3, 4], row k = (R0k, R1k, R2k, tk): the rotation acts on row
 *          vectors, p = s * v R + t, as the source's align_pred_to_gt applies Procrustes' result) and s = point_scale[head] (NULL: 1):
 *              p_k = ((v0 * T[k][0] + v1 * T[k][1]) + v2 * T[k][2]) * s + T[k][3]          in float64, in this order, uncontracted
 *   sqdist[head, m] = min over points of the distance above, index[head, m] = the lowest index that attains it,
 *   mean[head] = (sum of sqdist[head, :]) / M with the sum in this fixed order: lane l < 256 adds elements l, l + 256, l + 512, ... in turn, then the 256
 *          partial sums fold as a tree, partial[l] += partial[l + h] for h = 128, 64, ..., 1.
 * mean is the one-sided chamfer distance of the source (kaolin's chamfer_distance(p1, p2, w1 = 1, w2 = 0) by its documented definition). */
typedef struct vghev_nearest_job {
    int32_t n_heads;                /* 0 .. VGHEV_MAX_HEADS; 0 queues nothing */
    int32_t n_queries;              /* M: 1 .. VGHEV_MAX_POINTS */
    int32_t n_points;               /* P: 1 .. VGHEV_MAX_POINTS */
    int32_t reserved;               /* 0 */
    const float* query_dev;         /* f32 [n_heads, M, 3] on the device; never written */
    const double* query_scale_dev;  /* f64 [n_heads] on the device, or NULL */
    const float* points_dev;        /* f32 [n_heads, P, 3] on the device; never written */
    const double* transform_dev;    /* f64 [n_heads, 3, 4] on the device, or NULL */
    const double* point_scale_dev;  /* f64 [n_heads] on the device, or NULL; needs transform_dev */
    double* sqdist_dev;             /* f64 [n_heads, M] on the device */
    int32_t* index_dev;             /* i32 [n_heads, M] on the device */
    double* mean_dev;               /* f64 [n_heads] on the device, or NULL */
} vghev_nearest_job;

/* ---- detection AP: COCO-style box evaluation (csrc/detection_ap.hip) ----------------------------------------------------------------------------
 * What the reference's head-detection benchmarks (yolo_head_training/evaluation/evaluate_wider.py, evaluate_fddb.py) ask of pycocotools'
 * COCOeval(..., 'bbox'), by its published definition, for one category.  Boxes are float64 [x, y, w, h]; every float below is ONE IEEE float64 operation
 * in the stated order or an exact integer count, so every output is bitwise deterministic and equal to tests/detection_ap_ref.py.
 *
 *   IoU(D, G, crowd)   da = D.w * D.h;  ga = G.w * G.h
 *                      w = fmin(D.x + D.w, G.x + G.w) - fmax(D.x, G.x);  h likewise;  w <= 0 or h <= 0: the IoU is 0
 *                      i = w * h;  u = crowd ? da : (da + ga) - i;  o = i / u
 *   rank               per image the detections are ordered by (-score, input position) and cut to max_det; the position in that order is the rank.
 *                      The "kept" arrays below hold kept_i = min(nd_i, max_det) entries per image, image after image, in rank order.
 *   ground truth       per area range a = (lo, hi): ignored = crowd || area < lo || area > hi; order = the non-ignored in input order, then the ignored.
 *   matching           per (a, threshold t), detections in rank order: best = fmin(t, 1 - 1e-10), m = none; walk the ground truths in the order above:
 *                      skip g if it is matched at this t and not crowd; stop if m is non-ignored and g is ignored; skip g if IoU < best; else best = IoU,
 *                      m = g (equality passes: of equal IoUs the later ground truth wins).  With a match the detection records m, inherits its ignore
 *                      flag, and m is marked matched; an unmatched detection whose own area w * h lies outside [lo, hi] is ignored.
 *   curves             per (t, a, max_dets[k]): the kept detections of rank < max_dets[k] in the global order (-score, image, rank); tp / fp are the
 *                      inclusive counts of matched / unmatched non-ignored ones; rc = tp / n_pos[a]; pr = tp / ((fp + tp) + 2.220446049250313e-16),
 *                      then its running maximum from the right; for rec_thr[r] the first position p with rc[p] >= rec_thr[r] gives
 *                      precision[t, r, a, k] = pr[p] and scores[t, r, a, k] = score[p] (0 if there is none); recall[t, a, k] = the last rc (0 without
 *                      detections).  With n_pos[a] == 0 all three are -1.
 *
 * The offset arrays live on the device, so the entry points cannot read them: they check the sizes below, and the kernels check every image's range
 * against them.  An image whose range is inconsistent is left out and *status_dev becomes non-zero; nothing is ever read or written outside the arrays.
 * Non-finite boxes or scores give unspecified values, never an access outside the arrays. */
#define VGHEV_MAX_IMAGES 1048576
#define VGHEV_MAX_GT_PER_IMAGE 4096
#define VGHEV_MAX_DET 1024      /* max_dets[-1]: the engine's own top-k ceiling */
#define VGHEV_MAX_KEPT 1073741824 /* kept detections of all images */
#define VGHEV_MAX_IOU_THR 16
#define VGHEV_MAX_REC_THR 1024
#define VGHEV_MAX_AREA_RNG 8
#define VGHEV_MAX_MAX_DETS 4

/* Detections and ground truth of I images in CSR form, all on the device, none ever written. */
typedef struct vghev_box_set {
    int32_t n_images;              /* I: 0 .. VGHEV_MAX_IMAGES; 0 queues nothing and writes nothing: no output, n_pos and status included, is touched */
    int32_t n_dt;                  /* Nd >= 0 */
    int32_t n_gt;                  /* Ng >= 0 */
    int32_t max_gt;                /* an upper bound of the ground truths of one image, 0 .. VGHEV_MAX_GT_PER_IMAGE; an image with more is inconsistent */
    const double* dt_box_dev;      /* f64 [Nd, 4] xywh */
    const double* dt_score_dev;    /* f64 [Nd]; not read by vghev_box_iou */
    const int32_t* dt_offset_dev;  /* i32 [I + 1] */
    const double* gt_box_dev;      /* f64 [Ng, 4] xywh */
    const double* gt_area_dev;     /* f64 [Ng], or NULL: w * h */
    const uint8_t* gt_crowd_dev;   /* u8 [Ng], or NULL: all 0 */
    const int32_t* gt_offset_dev;  /* i32 [I + 1] */
} vghev_box_set;

/* The dense IoU block of every image: iou[iou_offset[i] + d * ng_i + g] for detection d and ground truth g of image i, both in input order. */
typedef struct vghev_box_iou_job {
    vghev_box_set set;
    int64_t n_iou;                  /* sum of nd_i * ng_i */
    const int64_t* iou_offset_dev;  /* i64 [I + 1]: iou_offset[i + 1] - iou_offset[i] = nd_i * ng_i */
    double* iou_dev;                /* f64 [n_iou] */
    int32_t* status_dev;            /* i32 [1] */
} vghev_box_iou_job;

/* The matching.  Outputs for kept detection q (image i, rank r: q = kept_offset[i] + r) and matching (a, t) at [(a * T + t) * n_kept + q]. */
typedef struct vghev_box_match_job {
    vghev_box_set set;
    int32_t n_iou_thr;               /* T: 1 .. VGHEV_MAX_IOU_THR */
    int32_t n_area;                  /* A: 1 .. VGHEV_MAX_AREA_RNG */
    int32_t max_det;                 /* max_dets[-1]: 1 .. VGHEV_MAX_DET */
    int32_t reserved;                /* 0 */
    int64_t n_kept;                  /* sum of min(nd_i, max_det): 0 .. VGHEV_MAX_KEPT */
    const double* iou_thr_dev;       /* f64 [T] */
    const double* area_rng_dev;      /* f64 [A, 2]: lo, hi */
    const int32_t* kept_offset_dev;  /* i32 [I + 1]: kept_offset[i + 1] - kept_offset[i] = min(nd_i, max_det) */
    int32_t* match_dev;              /* i32 [A, T, n_kept]: the matched ground truth's input index within its image, or -1 */
    uint8_t* ignore_dev;             /* u8 [A, T, n_kept] */
    int32_t* det_image_dev;          /* i32 [n_kept] */
    int32_t* det_rank_dev;           /* i32 [n_kept] */
    int32_t* det_index_dev;          /* i32 [n_kept]: the detection's input position within its image */
    double* det_score_dev;           /* f64 [n_kept] */
    int32_t* n_pos_dev;              /* i32 [A]: the non-ignored ground truths of all images */
    int32_t* status_dev;             /* i32 [1] */
} vghev_box_match_job;

/* The curves from vghev_box_match's outputs (det_rank and det_score as it wrote them: image after image, in rank order). */
typedef struct vghev_pr_job {
    int64_t n_kept;                /* 0 .. VGHEV_MAX_KEPT */
    int32_t n_iou_thr;             /* T */
    int32_t n_rec_thr;             /* R: 1 .. VGHEV_MAX_REC_THR */
    int32_t n_area;                /* A */
    int32_t n_max_dets;            /* M: 1 .. VGHEV_MAX_MAX_DETS */
    int32_t max_dets[4];           /* on the HOST: ascending, 1 .. VGHEV_MAX_DET */
    const double* rec_thr_dev;     /* f64 [R] */
    const int32_t* match_dev;      /* i32 [A, T, n_kept] */
    const uint8_t* ignore_dev;     /* u8 [A, T, n_kept] */
    const int32_t* det_rank_dev;   /* i32 [n_kept] */
    const double* det_score_dev;   /* f64 [n_kept] */
    const int32_t* n_pos_dev;      /* i32 [A] */
    void* scratch_dev;             /* vghev_ap_scratch_bytes(n_kept) bytes on the device, 16-byte aligned; the library allocates nothing */
    int64_t scratch_bytes;
    double* precision_dev;         /* f64 [T, R, A, M] */
    double* scores_dev;            /* f64 [T, R, A, M] */
    double* recall_dev;            /* f64 [T, A, M] */
} vghev_pr_job;

VGHEV_API const char* vghev_version(void);
VGHEV_API const char* vghev_last_error(void);

/* Everything is checked (null pointers, sizes, flags) before anything is queued; the checks need no GPU. */
VGHEV_API int vghev_z_order(const vghev_z_order_job* job, void* stream);
VGHEV_API int vghev_nearest(const vghev_nearest_job* job, void* stream);
VGHEV_API int vghev_box_iou(const vghev_box_iou_job* job, void* stream);
VGHEV_API int vghev_box_match(const vghev_box_match_job* job, void* stream);
VGHEV_API int vghev_pr_accumulate(const vghev_pr_job* job, void* stream);
/* The scratch vghev_pr_accumulate needs for n_kept detections (the global sort's keys, its permutation and the sorted ranks and scores); the other two
 * exports need none.  Negative (VGHEV_ERR_INVALID) for an n_kept outside 0 .. VGHEV_MAX_KEPT. */
VGHEV_API int64_t vghev_ap_scratch_bytes(int64_t n_kept);

#ifdef __cplusplus
}
#endif
#endif
