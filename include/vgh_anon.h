/* vgh_anon.h -- libvghanon.so: head anonymisation (pixelate, blur or fill every head of an image) for the MI355X head detector (gfx950 only).
 *
 * The eighth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so,
 * libvghmerge.so and libvghtrack.so.  It returns a copy of an image in which the pixels every head owns are replaced by an effect that is computed from the
 * SOURCE image alone.  Every output byte is defined by the integer arithmetic stated below; there is no floating point anywhere in the library.  It links no
 * object of the other libraries and none of them loads it (the mesh silhouette of libvghvis.so reaches it as a device pointer the caller hands over).  Every
 * export carries the prefix vghan_; everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHAN_OK (0) or a negative code, vghan_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_ANON_H
#define VGH_ANON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHAN_API __attribute__((visibility("default")))
#else
#define VGHAN_API
#endif

#define VGHAN_OK 0
#define VGHAN_ERR_INVALID (-1)
#define VGHAN_ERR_HIP (-2)
#define VGHAN_ERR_NOMEM (-3)

#define VGHAN_MAX_SIDE 32767    /* image height and width, and the sides of a head's geometry box */
#define VGHAN_MAX_COORD 16777216 /* |x0|, |y0| of a geometry box stay below 2^24 */
#define VGHAN_MAX_HEADS 65536   /* n_heads of one call */
#define VGHAN_MAX_CELLS 64      /* cells along a side of a pixelated box */
#define VGHAN_MAX_RADIUS 1024   /* blur taps on either side of the centre */
#define VGHAN_TAP_SUM 65536     /* taps[0] + 2 * (taps[1] + ... + taps[r]) of every blur table */

#define VGHAN_METHOD_FILL 0
#define VGHAN_METHOD_PIXELATE 1
#define VGHAN_METHOD_BLUR 2

#define VGHAN_REGION_BOX 0     /* the owner map is painted from the geometry boxes */
#define VGHAN_REGION_ELLIPSE 1 /* ... from the ellipses inscribed in them */
#define VGHAN_REGION_MAP 2     /* the owner map is the caller's owner_dev (a mesh silhouette, a segmentation mask) */

/* The rule.  H = height, W = width, n = n_heads; src[y, x, c] is the byte at src_dev + y * src_pitch_bytes + 3 * x + c, dst is dense ([H, W, 3]).
 *
 * GEOMETRY BOX of head i: heads[i].(x0, y0, x1, y1), half-open [x0, x1) x [y0, y1) and NOT clipped to the image; Wb = x1 - x0, Hb = y1 - y0 lie in
 * 0 .. VGHAN_MAX_SIDE.  A box with a zero side contains no pixel.
 *
 * OWNER MAP O[y, x], int32, -1 = untouched:
 *   VGHAN_REGION_BOX      the largest i whose box contains (x, y)
 *   VGHAN_REGION_ELLIPSE  the largest i whose box contains (x, y) and for which, with dx = x - x0, dy = y - y0, in int64
 *                             (2 dx + 1 - Wb)^2 * Hb^2 + (2 dy + 1 - Hb)^2 * Wb^2 <= Wb^2 * Hb^2
 *                         (each side below 2^61 for sides <= 32767)
 *   VGHAN_REGION_MAP      owner_dev[y, x]; a value outside [0, n) counts as -1
 * ONE RULE FOR EVERY REGION: a pixel whose owner's geometry box does not contain it is left unchanged (this can only happen with VGHAN_REGION_MAP).
 *
 * EFFECT on an owned pixel (x, y) of head i = O[y, x], per channel c; every other pixel is copied.  Every effect reads src only, never the output of another
 * head, so the result does not depend on scheduling; where heads overlap the owner rule alone decides (a later head wins the pixel).
 *   VGHAN_METHOD_FILL      dst = color[c]
 *   VGHAN_METHOD_PIXELATE  s = heads[i].cell >= 1.  The pixel lies in cell ((x - x0) / s, (y - y0) / s) of a grid anchored at the unclipped (x0, y0); a cell is
 *                          the pixels of the geometry box with that pair (the last row and column of cells are ragged where s does not divide the box).
 *                          The cell's value is (2 S + m) / (2 m) (integer division), S and m being the sum and the number of ALL pixels of the cell that
 *                          lie in the image, owned by the head or not.  (S can exceed 32 bits; a cell with m = 0 is never referenced.)  At most
 *                          VGHAN_MAX_CELLS cells along either side: ceil(Wb / s), ceil(Hb / s) <= 64.
 *   VGHAN_METHOD_BLUR      r = heads[i].radius in 0 .. VGHAN_MAX_RADIUS, t[k] = taps[heads[i].tap_offset + k] for k = 0 .. r: t[k] >= 0 and
 *                          t[0] + 2 (t[1] + ... + t[r]) = 65536.  With replicate border at the image edge:
 *                              h(x, y) = (sum over k = -r .. r of t[|k|] * src[y, clamp(x + k, 0, W - 1), c] + 128) >> 8        (<= 65280: uint16)
 *                              dst     = (sum over k = -r .. r of t[|k|] * h(x, clamp(y + k, 0, H - 1))     + 2^23) >> 24      (the sum is below 2^32)
 *                          A constant image stays constant and r = 0 is the identity.  The taps are an input, so no result rests on an exp().
 */
typedef struct vghan_head {
    int32_t x0, y0, x1, y1; /* the geometry box */
    int32_t cell;           /* VGHAN_METHOD_PIXELATE: the cell side s; otherwise ignored */
    int32_t radius;         /* VGHAN_METHOD_BLUR: r; otherwise ignored */
    int32_t tap_offset;     /* VGHAN_METHOD_BLUR: the head's table is taps[tap_offset .. tap_offset + r]; otherwise ignored */
    int32_t reserved;       /* 0 */
} vghan_head;

typedef struct vghan_job {
    const uint8_t* src_dev;  /* u8 [H, W, 3] on the device, pixels 3 bytes apart, rows src_pitch_bytes apart; never written */
    uint8_t* dst_dev;        /* u8 [H, W, 3] on the device, dense, 4-byte aligned; must not overlap the source */
    int64_t src_pitch_bytes; /* >= 3 * width */
    int32_t height;          /* 1 .. VGHAN_MAX_SIDE */
    int32_t width;           /* 1 .. VGHAN_MAX_SIDE */
    int32_t n_heads;         /* 0 .. VGHAN_MAX_HEADS */
    int32_t method;          /* VGHAN_METHOD_* */
    int32_t region;          /* VGHAN_REGION_* */
    int32_t color;           /* VGHAN_METHOD_FILL: channel 0 | channel 1 << 8 | channel 2 << 16; the top byte is 0 */
    const vghan_head* heads; /* host, [n_heads] */
    const int32_t* taps;     /* host, [n_taps]; VGHAN_METHOD_BLUR only */
    int32_t n_taps;          /* >= 0 */
    int32_t reserved;        /* 0 */
    const int32_t* owner_dev; /* i32 [H, W] on the device, dense: VGHAN_REGION_MAP; NULL for the other regions */
} vghan_job;

VGHAN_API const char* vghan_version(void);
VGHAN_API const char* vghan_last_error(void);

/* Bytes of device workspace vghan_anonymize needs for this job, a multiple of 16: the owner map where the library paints it (4 H W), one u32 per pixelation
 * cell or per pixel of every blurred head's clipped box, and the u16 h rows of every blurred head's clipped box extended by r rows up and down (clamped to the
 * image).  0 for a job vghan_anonymize would refuse (the message says why); a valid job needs at least 16.  No GPU is needed. */
VGHAN_API int64_t vghan_workspace_bytes(const vghan_job* job);

/* dst = src with every head anonymised.  `workspace_dev`: caller-owned device memory of at least vghan_workspace_bytes(job) bytes, 16-byte aligned, used by
 * this call alone until its work on `stream` has run.  The library allocates nothing but its small per-device staging block for the head rows and taps.
 * Everything is checked before anything is queued, and the checks need no GPU: null pointers, sizes, sides and caps out of range, a tap offset outside the
 * table, a negative tap or a tap sum other than 65536, more than VGHAN_MAX_HEADS heads, source and destination that overlap, a misaligned workspace; each
 * refusal returns VGHAN_ERR_INVALID with its message.  The number of launches depends on the method and the region, never on the number of heads. */
VGHAN_API int vghan_anonymize(const vghan_job* job, void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
