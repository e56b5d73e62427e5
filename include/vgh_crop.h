/* vgh_crop.h -- libvghcrop.so: head tensors, fixed-size normalised crops of every head in ONE launch, for the MI355X head detector (gfx950 only).
 *
 * The tenth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so,
 * libvghtrack.so, libvghanon.so and libvghvideo.so.  It hands the heads to the next network: one dense [n, 3, S, S] (or [n, S, S, 3]) tensor in that network's
 * own dtype, normalised, cut out of u8 RGB images or of 8-bit YUV 4:2:0 frames where they lie (no RGB copy of a frame is written).  It links no object of the
 * other libraries, includes none of their headers and none of them loads it.  Every export carries the prefix vghc_; everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHC_OK (0) or a negative code, vghc_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_CROP_H
#define VGH_CROP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHC_API __attribute__((visibility("default")))
#else
#define VGHC_API
#endif

#define VGHC_OK 0
#define VGHC_ERR_INVALID (-1)
#define VGHC_ERR_HIP (-2)
#define VGHC_ERR_NOMEM (-3)

#define VGHC_MAX_SIZE 1024      /* S, the side of every crop of a call */
#define VGHC_MAX_SUPERSAMPLE 8  /* K, sub-samples along a side of an output pixel */
#define VGHC_MAX_HEADS 65536    /* n_heads of one call */
#define VGHC_MAX_SIDE 32767     /* height and width of a source */
#define VGHC_MAX_TILES 16777216 /* n_heads * ceil(S / 16)^2 of one call (2^24: the tile list of one launch) */

#define VGHC_SOURCE_RGB 0    /* u8 [h, w, 3], pixels 3 bytes apart */
#define VGHC_SOURCE_YUV420 1 /* 8-bit YUV 4:2:0 planes (NV12, NV21, I420, YV12) */

#define VGHC_DTYPE_U8 0
#define VGHC_DTYPE_F32 1
#define VGHC_DTYPE_F16 2
#define VGHC_DTYPE_BF16 3

#define VGHC_LAYOUT_NCHW 0 /* planar [n, 3, S, S] */
#define VGHC_LAYOUT_NHWC 1 /* interleaved [n, S, S, 3] */

#define VGHC_ORDER_RGB 0 /* output channel c is source channel c */
#define VGHC_ORDER_BGR 1 /* output channel c is source channel 2 - c */

/* THE RULE (the single statement of it; tests/head_tensors_ref.py restates it in NumPy and the device equals that bit for bit).
 *
 * SOURCE PIXELS.  src(x, y, c), 0 <= x < w, 0 <= y < h, c = 0 (R), 1 (G), 2 (B):
 *   VGHC_SOURCE_RGB     the byte at rgb_dev + y * rgb_pitch_bytes + 3 * x + c.
 *   VGHC_SOURCE_YUV420  the fields of vgh_yuv420_image (include/vgh.h) and its integer rule, restated here so that this header stands alone:
 *                           Y = y_dev[y * y_pitch_bytes + x], U = u_dev[(y >> 1) * uv_pitch_bytes + (x >> 1) * chroma_step], V = v_dev[(same offset)]
 *                           c = Y - y_offset, d = U - 128, e = V - 128, in int32, >> the arithmetic shift, clamp8(v) = min(max(v, 0), 255):
 *                           R = clamp8((cy * c + crv * e + 32768) >> 16), G = clamp8((cy * c + cgu * d + cgv * e + 32768) >> 16),
 *                           B = clamp8((cy * c + cbu * d + 32768) >> 16)
 *                       Every tap is converted AND clamped to bytes before any weight is applied: the result of a frame is that of the RGB image of these
 *                       bytes.  Nearest chroma sample, no chroma interpolation.
 *   Outside 0 <= x < w, 0 <= y < h a tap reads the call's fill byte of its channel.
 *
 * SUB-SAMPLES.  Head k has a source, a supersampling factor K in 1 .. 8 and six int64 coefficients in Q32 (units of 2^-32 source pixels; integer coordinates are
 * pixel centres): X0, XP, XQ, Y0, YP, YQ.  For output pixel (i, j) of its S x S crop (row i, column j) and sub-sample (b, a), 0 <= a, b < K, with p = j K + a and
 * q = i K + b, in int64:
 *     PX = X0 + p XP + q XQ            PY = Y0 + p YP + q YQ
 *     source pixel (sx, sy) = (PX >> 32, PY >> 32)      flooring shifts
 *     fractions    fx = (PX >> 27) & 31,  fy = (PY >> 27) & 31        5 bits; the host adds 2^26 to X0 and Y0 so that they are rounded to nearest
 *     value(c)     = (32 - fx)(32 - fy) t00 + fx (32 - fy) t01 + (32 - fx) fy t10 + fx fy t11        t00 = src(sx, sy, c), t01 = src(sx + 1, sy, c),
 *                                                                                                    t10 = src(sx, sy + 1, c), t11 = src(sx + 1, sy + 1, c)
 * The four weights sum to 1024.  sum(c) is the int32 total of value(c) over the K^2 sub-samples: at most 255 * 1024 * 64 = 16 711 680 < 2^24, so every sum is
 * exactly a float32 -- which is why K stops at 8 and the fractions have 5 bits.  The K^2 sub-samples are a regular grid, not an area integral: a head larger than
 * 8 S pixels a side is sampled sparsely (it aliases), by design.
 *
 * OUTPUT.  Output channel c reads source channel c (VGHC_ORDER_RGB) or 2 - c (VGHC_ORDER_BGR); fill, a and b are given in the OUTPUT's channel order.
 *   VGHC_DTYPE_U8     (2 sum + d) / (2 d), d = 1024 K^2, integer division: the mean, rounded half up.  a and b are ignored.
 *   VGHC_DTYPE_F32    y = fl32(fl32((float)sum * a[c]) + b[c]): two float32 operations, never contracted into one (the library is built with
 *                     -ffp-contract=off).  a[c] and b[c] are inputs: the caller forms them in float64 as scale / (d std_c) and -mean_c / std_c and rounds once.
 *   VGHC_DTYPE_F16, VGHC_DTYPE_BF16    the round-to-nearest-even conversion of that y.
 * a depends on K through d, so it travels PER HEAD (vghc_head.a); b does not and travels per call (vghc_job.b).
 *
 * DESTINATION.  Dense: head k's crop is element block k of [n_heads, 3, S, S] (VGHC_LAYOUT_NCHW) or [n_heads, S, S, 3] (VGHC_LAYOUT_NHWC) at dst_dev.
 */
typedef struct vghc_source {
    int32_t kind;            /* VGHC_SOURCE_* */
    int32_t h, w;            /* 1 .. VGHC_MAX_SIDE (luma size of a frame) */
    int32_t chroma_step;     /* YUV420: bytes between chroma samples of a row, 1 = planar, 2 = interleaved; RGB: 0 */
    const uint8_t* rgb_dev;  /* RGB: the image on the device; YUV420: NULL */
    int64_t rgb_pitch_bytes; /* RGB: >= 3 * w */
    const uint8_t *y_dev, *u_dev, *v_dev; /* YUV420: luma [h, w], chroma [(h+1)/2, (w+1)/2] each; RGB: NULL */
    int64_t y_pitch_bytes;   /* YUV420: >= w */
    int64_t uv_pitch_bytes;  /* YUV420: >= chroma_step * ((w+1)/2), one pitch for both chroma planes */
    int32_t y_offset;        /* YUV420: 0 .. 255 */
    int32_t cy, crv, cgu, cgv, cbu; /* YUV420: fixed-point coefficients * 2^16, each |c| <= 2^20 */
} vghc_source;

typedef struct vghc_head {
    int64_t x0, xp, xq, y0, yp, yq; /* Q32; |x0| + S K (|xp| + |xq|) < 2^62 and likewise for y: no position overflows */
    int32_t source;                 /* index into the job's sources */
    int32_t supersample;            /* K, 1 .. VGHC_MAX_SUPERSAMPLE */
    float a[3];                     /* finite; output channel order; ignored for VGHC_DTYPE_U8 */
    int32_t reserved;               /* 0 */
} vghc_head;

typedef struct vghc_job {
    const vghc_source* sources; /* host, [n_sources] */
    const vghc_head* heads;     /* host, [n_heads] */
    int32_t n_sources;          /* >= 0 (0 only with n_heads = 0) */
    int32_t n_heads;            /* 0 .. VGHC_MAX_HEADS */
    int32_t size;               /* S, 1 .. VGHC_MAX_SIZE */
    int32_t dtype;              /* VGHC_DTYPE_* */
    int32_t layout;             /* VGHC_LAYOUT_* */
    int32_t channel_order;      /* VGHC_ORDER_* */
    int32_t fill;               /* channel 0 | channel 1 << 8 | channel 2 << 16, output channel order; the top byte is 0 */
    float b[3];                 /* finite; output channel order; ignored for VGHC_DTYPE_U8 */
    void* dst_dev;              /* the result on the device, aligned to its element size; must not overlap a source */
    int64_t dst_bytes;          /* bytes the caller owns at dst_dev: at least n_heads * 3 * S * S elements */
} vghc_job;

VGHC_API const char* vghc_version(void);
VGHC_API const char* vghc_last_error(void);

/* Heads of many sources in ONE call: one staging upload (sources, heads, the (head, 16 x 16 tile) list) and one launch, whatever n_heads and n_sources are;
 * n_heads = 0 queues nothing.  The library allocates nothing but its per-device staging block.  Everything is checked before anything is queued, and the checks
 * need no GPU: null pointers, S, K, n_heads, source sides, pitches and YUV coefficients out of range, a source index outside the array, non-finite a or b, a
 * position that could overflow, a misaligned destination or one smaller than the result; each refusal returns VGHC_ERR_INVALID with its message. */
VGHC_API int vghc_head_tensors(const vghc_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
