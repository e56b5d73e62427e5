/* vgh_merge.h -- libvghmerge.so: the cross-tile merge of sliced detection for the MI355X head detector (gfx950 only).
 *
 * The sixth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so and libvgheval.so.  It turns
 * the per-tile detections of one photograph, exactly as vgh_detect leaves them (fixed-capacity slabs in the padded S x S space of every tile), into one
 * list of heads in image coordinates.  It links no object of the other libraries and none of them loads it.  Every export carries the prefix vghm_;
 * everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHM_OK (0) or a negative code, vghm_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_MERGE_H
#define VGH_MERGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHM_API __attribute__((visibility("default")))
#else
#define VGHM_API
#endif

#define VGHM_OK 0
#define VGHM_ERR_INVALID (-1)
#define VGHM_ERR_HIP (-2)
#define VGHM_ERR_NOMEM (-3)

#define VGHM_MAX_CANDIDATES 16384 /* n_tiles * keep_k */
#define VGHM_MAX_HEADS 1048576    /* max_heads: rows of the outputs (more than VGHM_MAX_CANDIDATES are never filled with heads) */

#define VGHM_METRIC_IOU 0 /* inter / (area_a + area_b - inter) */
#define VGHM_METRIC_IOS 1 /* inter / fminf(area_a, area_b): intersection over the smaller box */

#define VGHM_STATUS_ABSENT 0     /* rank >= counts[tile] */
#define VGHM_STATUS_KEPT 1       /* emitted */
#define VGHM_STATUS_TRUNCATED 2  /* touches an interior edge of its tile */
#define VGHM_STATUS_SUPPRESSED 3 /* matched by an earlier kept candidate of another tile */
#define VGHM_STATUS_OVER_CAP 4   /* kept, but behind the first max_heads kept candidates */

/* The rule.  Candidate (t, r), index i = t * keep_k + r, exists iff r < counts[t].  All arithmetic is float32, every operation rounded on its own (no
 * fused multiply-add), in the order written.  S = image_size; a tile row is (off_x, off_y, w, h, pad_x, pad_y, new_w, new_h), integers converted to
 * float exactly.
 *   1. clip         c = fminf(fmaxf(box, 0), S) per coordinate.  A NaN coordinate therefore becomes 0 and an infinite one 0 or S: after this step every
 *                   coordinate is finite.
 *   2. truncation   with bs = border * scale[t]: the candidate is dropped (TRUNCATED) if
 *                       bit 0 of interior[t] (left)   and c.x1 < pad_x + bs, or
 *                       bit 1 (top)                   and c.y1 < pad_y + bs, or
 *                       bit 2 (right)                 and c.x2 > (float)(pad_x + new_w) - bs, or
 *                       bit 3 (bottom)                and c.y2 > (float)(pad_y + new_h) - bs.
 *                   Strict comparisons; an edge whose bit is clear never drops anything.
 *   3. image coordinates   f = ((c - pad) / scale[t]) + off, per coordinate (pad_x, off_x for x1 and x2; pad_y, off_y for y1 and y2).
 *   4. order        descending score, ties by ascending i.  "Descending score" is the order of the score's BIT PATTERN under the usual total-order map
 *                   u = bits ^ (bits & 0x80000000 ? 0xffffffff : 0x80000000), larger u first: for finite scores and infinities that is the numeric
 *                   order with +0 before -0; a NaN sorts where its bits put it (positive NaNs before +inf, negative NaNs after -inf).  Nothing else
 *                   looks at a score, so a non-finite score cannot do more than move its candidate in the order.
 *   5. greedy walk  in that order a candidate is SUPPRESSED iff an earlier KEPT candidate of ANOTHER tile matches it, a = the earlier, b = the later box:
 *                       area = (x2 - x1) * (y2 - y1);  w = fmaxf(0, fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1)), h alike;  inter = w * h
 *                       IOU:  inter / (area_a + area_b - inter) > match_thr        IOS:  inter / fminf(area_a, area_b) > match_thr
 *                   A NaN quotient (0 / 0 of zero-area boxes) does not suppress.  Candidates of one tile never suppress each other: that tile's own NMS has
 *                   ruled on them.
 *   6. emit         the first max_heads kept candidates, in order; later kept ones get OVER_CAP.
 * Outputs: rows [0, n_heads) hold the emitted heads; rows [n_heads, max_heads) hold head_row = head_tile = -1 and zeros.  n_kept_uncapped is the number of
 * kept candidates before the cap.  Every output is bitwise reproducible.
 *
 * counts are read on the device (values outside 0 .. keep_k are clamped to that range); the host never sees them.  The number of launches does not depend
 * on the number of candidates. */
typedef struct vghm_merge_job {
    int32_t n_tiles;    /* T >= 1 */
    int32_t keep_k;     /* >= 1; T * keep_k <= VGHM_MAX_CANDIDATES */
    int32_t image_size; /* S >= 1 */
    int32_t max_heads;  /* 1 .. VGHM_MAX_HEADS */
    int32_t metric;     /* VGHM_METRIC_IOU or VGHM_METRIC_IOS */
    float border;       /* source pixels of the tile; finite, >= 0 */
    float match_thr;    /* not NaN */
    int32_t reserved;   /* 0 */
    const float* boxes_dev;    /* f32 [T, keep_k, 4] xyxy in the padded S-space of each tile, on the device; never written */
    const float* scores_dev;   /* f32 [T, keep_k] on the device */
    const int32_t* counts_dev; /* i32 [T] on the device */
    const int32_t* tiles;      /* host, [T, 8]: off_x, off_y, w, h, pad_x, pad_y, new_w, new_h */
    const float* scale;        /* host, [T]: finite, > 0 */
    const uint8_t* interior;   /* host, [T]: bits 0 .. 3 = left, top, right, bottom edge lies inside the image */
    int32_t* head_row_dev;     /* i32 [max_heads] on the device: t * keep_k + r */
    int32_t* head_tile_dev;    /* i32 [max_heads] */
    float* boxes_full_dev;     /* f32 [max_heads, 4], 16-byte aligned */
    float* scores_out_dev;     /* f32 [max_heads] */
    int32_t* n_heads_dev;      /* i32 [1] */
    int32_t* n_kept_uncapped_dev; /* i32 [1] */
    uint8_t* status_dev;       /* u8 [T * keep_k] on the device, or NULL */
} vghm_merge_job;

VGHM_API const char* vghm_version(void);
VGHM_API const char* vghm_last_error(void);

/* Bytes of device workspace vghm_merge_tiles needs for these sizes (a 64-bit match mask [N, N / 64] dominates: 32 MiB at the capacity); 0 if the sizes
 * are invalid. */
VGHM_API int64_t vghm_merge_workspace_bytes(int32_t n_tiles, int32_t keep_k);

/* `workspace_dev`: caller-owned device memory of at least vghm_merge_workspace_bytes bytes, 16-byte aligned, used by this call alone until its work on
 * `stream` has run; its contents before and after are meaningless.  The library allocates nothing but its small per-device staging block for the three
 * host tables.  Null pointers, sizes out of range (T * keep_k > VGHM_MAX_CANDIDATES included), a bad metric, border, threshold or scale and a misaligned
 * workspace return VGHM_ERR_INVALID before anything is queued; these checks need no GPU. */
VGHM_API int vghm_merge_tiles(const vghm_merge_job* job, void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
