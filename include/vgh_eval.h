/* vgh_eval.h -- libvgheval.so: mesh benchmark metrics for the MI355X head detector (gfx950 only).
 *
 * The fifth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so (include/vgh_view.h), libvghvis.so (include/vgh_vis.h)
 * and libvghtex.so (include/vgh_tex.h).  This one judges predicted heads against ground-truth meshes: the two neighbour searches behind the DAD-3DHeads
 * metrics Z_n and chamfer distance (yolo_head_training/evaluation/dad_utils.py of the reference: calc_zn, calc_ch_dist), for any number of heads in one
 * call.  It links no object of the other four and none of them loads it.  Every export carries the prefix vghev_; everything else has hidden visibility.
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

VGHEV_API const char* vghev_version(void);
VGHEV_API const char* vghev_last_error(void);

/* Everything is checked (null pointers, sizes, flags) before anything is queued; the checks need no GPU. */
VGHEV_API int vghev_z_order(const vghev_z_order_job* job, void* stream);
VGHEV_API int vghev_nearest(const vghev_nearest_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
