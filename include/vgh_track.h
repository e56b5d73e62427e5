/* vgh_track.h -- libvghtrack.so: head tracking across the frames of a video for the MI355X head detector (gfx950 only).
 *
 * The seventh library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so and
 * libvghmerge.so.  It takes the per-frame detections exactly as vgh_detect leaves them (fixed-capacity slabs in the padded S x S space of every frame) and
 * steps a device-resident table of tracks through the frames in order: stable identities, heads that survive a few frames of occlusion, smoothed boxes and
 * smoothed FLAME parameters.  Every count stays on the device.  It links no object of the other libraries and none of them loads it.  Every export carries
 * the prefix vght_; everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHT_OK (0) or a negative code, vght_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_TRACK_H
#define VGH_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHT_API __attribute__((visibility("default")))
#else
#define VGHT_API
#endif

#define VGHT_OK 0
#define VGHT_ERR_INVALID (-1)
#define VGHT_ERR_HIP (-2)
#define VGHT_ERR_NOMEM (-3)

#define VGHT_MAX_TRACKS 2048 /* max_tracks: slots of the track table; also the most rows max_out may ask for */
#define VGHT_MAX_DETS 2048   /* keep_k: detection rows of one frame */
#define VGHT_MAX_FRAMES 1024 /* n_frames of one call */
#define VGHT_NUM_PARAMS 413  /* floats of one FLAME parameter vector */

/* The state: caller-owned device memory of vght_state_bytes(max_tracks) bytes, 16-byte aligned.  With M = max_tracks and A(n) = n rounded up to a multiple
 * of 16, every part starts on a 16-byte boundary, in this order:
 *     header   16 bytes        i32 next_id, i32 frame, two i32 that are 0
 *     id       A(4 M)          i32 [M]      -1 = the slot is free
 *     hits     A(4 M)          i32 [M]      frames in which the slot was matched, the birth included
 *     misses   A(4 M)          i32 [M]      frames since the last match
 *     age      A(4 M)          i32 [M]      frames since the birth, the birth frame counted
 *     det_row  A(4 M)          i32 [M]      the detection row of the last frame, -1 if the slot coasted
 *     score    A(4 M)          f32 [M]      the score of the last matched detection
 *     box      16 M            f32 [M, 4]   xyxy in IMAGE coordinates
 *     vel      16 M            f32 [M, 4]   per frame, per coordinate
 *     params   A(4 * 413 M)    f32 [M, 413] the smoothed FLAME vector
 * so the offsets are 16, 16 + A(4 M), ..., 16 + 6 A(4 M), + 16 M, + 16 M, and the size is the last offset + A(1652 M).  A free slot holds id = det_row = -1 and
 * zeros everywhere else, except that its params keep what they last held (they are rewritten at the next birth). */
#define VGHT_STATE_HEADER_BYTES 16

/* The rule.  All arithmetic is float32, every operation rounded on its own (no fused multiply-add), in the order written.  S = image_size, (pad_x, pad_y,
 * scale) = the frame's row of `unpad`.  For one frame, with the state as the previous frame left it:
 *   1. detections   row r exists iff r < clamp(counts, 0, keep_k).  c = fminf(fmaxf(box, 0), S) per coordinate: a NaN coordinate becomes 0 and an infinite one
 *                   0 or S, so every coordinate is finite afterwards.  Image coordinates d = (c - pad) / scale (pad_x for x1 and x2, pad_y for y1 and y2).
 *                   The row is HIGH if score >= high_thr, else LOW if score >= low_thr, else ignored; a NaN score fails both comparisons.
 *   2. predict      for every live slot (id >= 0) p = box + vel per coordinate.
 *   3. similarity   of a predicted box a and a detection b:  area = fmaxf(0, x2 - x1) * fmaxf(0, y2 - y1);
 *                   inter = fmaxf(0, fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1)) * fmaxf(0, fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1));
 *                   iou = inter / ((area_a + area_b) - inter).  A NaN quotient (0 / 0 of zero-area boxes) never matches.
 *   4. association  two stages.  Stage 1: all live slots against the HIGH rows, pairs with iou > match_thr.  Stage 2: the slots stage 1 left unmatched
 *                   that had misses == 0 on entry against the LOW rows, pairs with iou > match_thr_low.  Within a stage the matching is the greedy matching
 *                   in the total order (iou descending, slot ascending, row ascending): a pair is taken iff neither side was taken by an earlier pair.
 *                   (The device computes it as rounds of mutual best choice, which under a strict total order is the same matching.)
 *   5. matched      slot, d = the detection's box, x = its parameter vector, q = the old value:
 *                       nb = p + box_gain * (d - p);   vel = vel + vel_gain * ((nb - box) - vel);   box = nb;
 *                       params = isfinite(x) ? q + param_gain * (x - q) : q    per element;
 *                   a gain that equals 1 copies the measurement instead (nb = d; vel = nb - box; params = x), because q + (x - q) is not x in float32.
 *                   hits += 1, misses = 0, score = the detection's score, det_row = r.
 *   6. unmatched    slot: box = p (the track coasts), misses += 1, det_row = -1.  It is freed if it was tentative (hits < min_hits) or if misses > max_age.
 *   7. births       after the frees of step 6, so a slot freed in this frame can be taken in it: the unmatched HIGH rows in ascending row order take the free
 *                   slots in ascending slot order, id = next_id++ in that order; box = d, vel = 0, params = x with non-finite elements set to 0, hits = 1,
 *                   misses = 0, age = 0, score and det_row as for a match.  Rows that find no free slot are counted in n_dropped.
 *   8. report       the slots with hits >= min_hits and misses <= report_misses, in ascending slot order; the first max_out of them are written, n_out is
 *                   their number.  Output rows behind n_out hold -1 (slot, id, det_row) and 0 (everything else).  age += 1 for every live slot; frame += 1.
 * A call of B frames leaves the same state and outputs, bit for bit, as B calls of one frame.  counts are read on the device; the host never sees them, and
 * the number of launches per frame does not depend on them. */
typedef struct vght_track_job {
    int32_t n_frames;      /* B: 1 .. VGHT_MAX_FRAMES */
    int32_t keep_k;        /* 1 .. VGHT_MAX_DETS */
    int32_t max_tracks;    /* M: 1 .. VGHT_MAX_TRACKS, the M the state was made for */
    int32_t image_size;    /* S >= 1 */
    int32_t max_out;       /* rows of the per-frame outputs: 1 .. VGHT_MAX_TRACKS */
    int32_t max_age;       /* >= 0 */
    int32_t min_hits;      /* >= 1 */
    int32_t report_misses; /* >= 0 */
    float high_thr;        /* not NaN */
    float low_thr;         /* not NaN */
    float match_thr;       /* not NaN */
    float match_thr_low;   /* not NaN */
    float box_gain;        /* finite */
    float vel_gain;        /* finite */
    float param_gain;      /* finite */
    int32_t reserved;      /* 0 */
    const float* boxes_dev;    /* f32 [B, keep_k, 4] xyxy in the padded S-space of each frame, on the device, 16-byte aligned; never written */
    const float* scores_dev;   /* f32 [B, keep_k] on the device */
    const float* flame_dev;    /* f32 [B, keep_k, 413] on the device */
    const int32_t* counts_dev; /* i32 [B] on the device */
    const float* unpad;        /* host, [B, 3]: pad_x, pad_y, scale per frame; finite, scale > 0 */
    int32_t* n_out_dev;        /* i32 [B] */
    int32_t* out_slot_dev;     /* i32 [B, max_out] */
    int32_t* out_id_dev;       /* i32 [B, max_out] */
    int32_t* out_det_row_dev;  /* i32 [B, max_out]: -1 for a coasting track */
    int32_t* out_hits_dev;     /* i32 [B, max_out] */
    int32_t* out_misses_dev;   /* i32 [B, max_out] */
    float* out_box_dev;        /* f32 [B, max_out, 4] in image coordinates, 16-byte aligned */
    float* out_score_dev;      /* f32 [B, max_out] */
    float* out_params_dev;     /* f32 [B, max_out, 413], or NULL = not written */
    int32_t* det_id_dev;       /* i32 [B, keep_k]: the id each detection row was given (matched or born), else -1; or NULL */
    int32_t* n_born_dev;       /* i32 [B] */
    int32_t* n_freed_dev;      /* i32 [B] */
    int32_t* n_dropped_dev;    /* i32 [B] */
} vght_track_job;

VGHT_API const char* vght_version(void);
VGHT_API const char* vght_last_error(void);

/* Bytes of the state for max_tracks slots (the layout above); 0 if max_tracks is outside 1 .. VGHT_MAX_TRACKS. */
VGHT_API int64_t vght_state_bytes(int32_t max_tracks);

/* Every slot free (id = det_row = -1, zeros elsewhere, params included), next_id = 0, frame = 0.  `state_dev` is 16-byte aligned. */
VGHT_API int vght_state_init(void* state_dev, int32_t max_tracks, void* stream);

/* Bytes of device workspace vght_track_frames needs for these sizes (two i32 per slot: what the parameter kernel has to do); 0 if a size is out of
 * range. */
VGHT_API int64_t vght_workspace_bytes(int32_t max_tracks, int32_t keep_k);

/* Steps the state through the job's frames in order.  `workspace_dev`: caller-owned device memory of at least vght_workspace_bytes bytes, 16-byte aligned,
 * used by this call alone until its work on `stream` has run.  The library allocates nothing but its small per-device staging block for the `unpad` table.
 * Null pointers, sizes out of range, non-finite gains, NaN thresholds, a bad `unpad` row and misaligned buffers return VGHT_ERR_INVALID before anything is
 * queued; these checks need no GPU.  Two launches per frame and one upload per call, whatever the counts are. */
VGHT_API int vght_track_frames(const vght_track_job* job, void* state_dev, void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
