/* vgh_video.h -- libvghvideo.so: video frames out of the MI355X head detector (gfx950 only) -- every head hidden directly in the luma and chroma planes of
 * an 8-bit YUV 4:2:0 frame (no RGB image is made, in place if wanted), and an RGB image packed into such planes for an encoder.
 *
 * The ninth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so,
 * libvghtrack.so and libvghanon.so.  Every output byte is defined by the integer arithmetic stated below; there is no floating point anywhere in the library.
 * It links no object of the other libraries and none of them loads it.  Every export carries the prefix vghy_; everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHY_OK (0) or a negative code, vghy_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_VIDEO_H
#define VGH_VIDEO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHY_API __attribute__((visibility("default")))
#else
#define VGHY_API
#endif

#define VGHY_OK 0
#define VGHY_ERR_INVALID (-1)
#define VGHY_ERR_HIP (-2)
#define VGHY_ERR_NOMEM (-3)

#define VGHY_MAX_SIDE 32767     /* frame height and width, and the sides of a head's geometry box */
#define VGHY_MAX_COORD 16777216 /* |x0|, |y0| of a geometry box stay below 2^24 */
#define VGHY_MAX_HEADS 65536    /* n_heads of one call */
#define VGHY_MAX_CELLS 64       /* cells along a side of a pixelated box */
#define VGHY_MAX_RADIUS 1024    /* blur taps on either side of the centre */
#define VGHY_TAP_SUM 65536      /* taps[0] + 2 * (taps[1] + ... + taps[r]) of every blur table */

#define VGHY_METHOD_FILL 0
#define VGHY_METHOD_PIXELATE 1
#define VGHY_METHOD_BLUR 2

#define VGHY_REGION_BOX 0     /* the luma owner map is painted from the luma geometry boxes */
#define VGHY_REGION_ELLIPSE 1 /* ... from the ellipses inscribed in them */
#define VGHY_REGION_MAP 2     /* the luma owner map is the caller's owner_dev (a mesh silhouette, a segmentation mask) */

/* One plane of a frame as the calls see it: sample (y, x) is the byte at src_dev + y * src_pitch + x * src_step, and at dst_dev + y * dst_pitch + x * dst_step.
 * A step is 1, or 2 for one of the two interleaved views of an NV12 / NV21 chroma plane (their pointers are one byte apart).  Pitches and steps are per
 * plane, so source and destination layouts may differ: NV12 in and I420 out of the same call is a by-product.  vghy_pack_rgb reads no plane: its src_* fields
 * are 0. */
typedef struct vghy_plane {
    const uint8_t* src_dev;
    uint8_t* dst_dev;
    int64_t src_pitch; /* bytes between rows; at least (plane width - 1) * src_step + 1 */
    int64_t dst_pitch;
    int32_t src_step; /* 1 or 2 */
    int32_t dst_step; /* 1 or 2 */
} vghy_plane;

/* THE ANONYMISATION RULE.  A frame is H x W luma samples (plane 0, Y) and CH x CW chroma samples, CH = (H + 1) / 2, CW = (W + 1) / 2, in each of plane 1 (U)
 * and plane 2 (V); chroma sample (cy, cx) colours the luma pixels {2 cy, 2 cy + 1} x {2 cx, 2 cx + 1} that lie in the frame.  Every plane is treated as a
 * one-channel image of its own size, PH x PW below.  n = n_heads.
 *
 * GEOMETRY BOX.  Head i has two rows: luma_heads[i] for plane 0 and chroma_heads[i] for planes 1 and 2.  A row's (x0, y0, x1, y1) is the head's box in THAT
 * plane's samples, half-open [x0, x1) x [y0, y1) and NOT clipped to the plane; Wb = x1 - x0 and Hb = y1 - y0 lie in 0 .. VGHY_MAX_SIDE.  A box with a zero
 * side contains no sample.  The library does not derive one row from the other: whoever calls chooses the chroma box (head_detector_amd.video takes
 * (x0 >> 1, y0 >> 1, (x1 + 1) >> 1, (y1 + 1) >> 1), which contains every chroma sample of every luma pixel of the luma box), the chroma cell side and the
 * chroma radius.  The two rows of all heads share the one tap table `taps`.
 *
 * LUMA OWNER MAP O[y, x], int32 [H, W], -1 = nobody:
 *   VGHY_REGION_BOX      the largest i whose luma box contains (x, y)
 *   VGHY_REGION_ELLIPSE  the largest i whose luma box contains (x, y) and for which, with dx = x - x0, dy = y - y0, in int64
 *                            (2 dx + 1 - Wb)^2 * Hb^2 + (2 dy + 1 - Hb)^2 * Wb^2 <= Wb^2 * Hb^2
 *                        (each side below 2^61 for sides <= 32767)
 *   VGHY_REGION_MAP      owner_dev[y, x]; a value outside [0, n) counts as -1
 * CHROMA OWNER MAP OC[cy, cx]: the maximum of O over the luma pixels {2 cy, 2 cy + 1} x {2 cx, 2 cx + 1} that lie in the frame, every value outside [0, n)
 * counting as -1.  A chroma sample is therefore replaced as soon as ANY luma pixel it colours is owned (the conservative choice for a privacy function), and
 * of several owners the later head wins, as everywhere else.  No second owner plane is stored: the maximum of four owners is taken where it is needed.
 * ONE RULE FOR EVERY REGION AND EVERY PLANE: a sample that its owner's box OF THAT PLANE does not contain is left unchanged.
 *
 * EFFECT on an owned sample (x, y) of head i (i = O[y, x] in plane 0, i = OC[y, x] in planes 1 and 2) inside the head's box of that plane; src is that
 * plane's source.  Every effect reads the source planes only, never the output of another head, so the result does not depend on scheduling.
 *   VGHY_METHOD_FILL      dst = the plane's byte of `color`, packed Y | U << 8 | V << 16
 *   VGHY_METHOD_PIXELATE  s = the row's cell >= 1.  The sample lies in cell ((x - x0) / s, (y - y0) / s) of a grid anchored at the plane's unclipped box
 *                         corner (x0, y0); a cell is the samples of the box with that pair (the last row and column of cells are ragged where s does not
 *                         divide the box).  The cell's value is (2 S + m) / (2 m) (integer division), S and m being the sum and the number of ALL samples of
 *                         the cell that lie in the plane, owned by the head or not, with S in 64 bits.  A cell with m = 0 is never referenced.  At most
 *                         VGHY_MAX_CELLS cells along either side: ceil(Wb / s), ceil(Hb / s) <= 64.  The luma and the chroma grid are independent.
 *   VGHY_METHOD_BLUR      r = the row's radius in 0 .. VGHY_MAX_RADIUS, t[k] = taps[tap_offset + k] for k = 0 .. r: t[k] >= 0 and
 *                         t[0] + 2 (t[1] + ... + t[r]) = 65536.  With replicate border at the plane's edge:
 *                             h(x, y) = (sum over k = -r .. r of t[|k|] * src[y, clamp(x + k, 0, PW - 1)] + 128) >> 8         (<= 65280: uint16)
 *                             dst     = (sum over k = -r .. r of t[|k|] * h(x, clamp(y + k, 0, PH - 1))   + 2^23) >> 24      (the sum is below 2^32)
 *                         A constant plane stays constant and r = 0 is the identity.  The taps are an input, so no result rests on an exp().
 *
 * IN PLACE.  Every destination plane is either EXACTLY its source plane -- the same pointer, pitch and step -- or overlaps no source plane; anything else is
 * refused.  A plane in place: only the samples that are owned and lie inside their owner's box are written; every other byte, those between width and pitch
 * included, is never touched.  A plane out of place: every sample of the destination plane is written (the source sample where nothing else applies) and no
 * byte outside its samples.  In place is safe because every effect value is staged in the workspace, computed from the source, before the pass that writes.
 *
 * LAUNCHES.  Whatever the number of heads, one call queues its staging copy and at most 11 more items: the clear of the owner plane (a memset; not with
 * VGHY_REGION_MAP), the owner painter, the value passes (pixelate: one for luma and one for chroma; blur: a horizontal and a vertical pass for each), one
 * write pass for luma and one for chroma, and one copy per plane that is out of place.  Every pass but the clear and the copies enumerates heads x tiles,
 * heads x cells or heads x row segments of the boxes clipped to their plane through prefix sums made on the host: in place, nothing but the clear of the
 * owner plane walks the frame.  Where U and V are the two interleaved views of one plane (step 2, pointers one byte apart in either order, the lower one
 * and the pitch even) a lane handles a (U, V) pair with one 16-bit access; planar chroma goes through the same kernels as two planes. */
typedef struct vghy_head {
    int32_t x0, y0, x1, y1; /* the geometry box in the samples of the row's plane */
    int32_t cell;           /* VGHY_METHOD_PIXELATE: the cell side s; otherwise ignored */
    int32_t radius;         /* VGHY_METHOD_BLUR: r; otherwise ignored */
    int32_t tap_offset;     /* VGHY_METHOD_BLUR: the row's table is taps[tap_offset .. tap_offset + r]; otherwise ignored */
    int32_t reserved;       /* 0 */
} vghy_head;

typedef struct vghy_anonymize_job {
    vghy_plane planes[3];          /* Y [H, W], U and V [CH, CW] */
    int32_t height;                /* H, 1 .. VGHY_MAX_SIDE */
    int32_t width;                 /* W, 1 .. VGHY_MAX_SIDE */
    int32_t n_heads;               /* 0 .. VGHY_MAX_HEADS */
    int32_t method;                /* VGHY_METHOD_* */
    int32_t region;                /* VGHY_REGION_* */
    int32_t color;                 /* VGHY_METHOD_FILL: Y | U << 8 | V << 16; the top byte is 0 */
    const vghy_head* luma_heads;   /* host, [n_heads] */
    const vghy_head* chroma_heads; /* host, [n_heads] */
    const int32_t* taps;           /* host, [n_taps]; VGHY_METHOD_BLUR only */
    int32_t n_taps;                /* >= 0 */
    int32_t reserved;              /* 0 */
    const int32_t* owner_dev;      /* i32 [H, W] on the device, dense: VGHY_REGION_MAP; NULL for the other regions */
} vghy_anonymize_job;

/* THE PACKER.  src[y, x, c] is the byte at src_dev + y * src_pitch_bytes + 3 * x + c (c = 0, 1, 2: R, G, B); the three destination planes are described
 * as above (their src_* fields are 0).  coef = (kyr, kyg, kyb, kur, kug, kub, kvr, kvg, kvb), 16.16 fixed point, each within +-2^20; >> is arithmetic:
 *     Y[y, x]        = clamp8(y_offset + ((kyr R + kyg G + kyb B + 32768) >> 16))
 *     (Rm, Gm, Bm)   = per channel (2 S + m) / (2 m), S and m the sum and the number of the pixels {2 cy, 2 cy + 1} x {2 cx, 2 cx + 1} that lie in the
 *                      image (m = 1, 2 or 4)
 *     U[cy, cx]      = clamp8(128 + ((kur Rm + kug Gm + kub Bm + 32768) >> 16))
 *     V[cy, cx]      = clamp8(128 + ((kvr Rm + kvg Gm + kvb Bm + 32768) >> 16))
 * The coefficients are an input, like the taps, so no result rests on a float.  Every sample of the three planes is written, and nothing outside them. */
typedef struct vghy_pack_job {
    const uint8_t* src_dev;  /* u8 [H, W, 3] on the device, pixels 3 bytes apart, rows src_pitch_bytes apart; never written */
    int64_t src_pitch_bytes; /* >= 3 * width */
    vghy_plane planes[3];    /* the destination: Y [H, W], U and V [CH, CW]; no plane may overlap the source */
    int32_t height;          /* 1 .. VGHY_MAX_SIDE */
    int32_t width;           /* 1 .. VGHY_MAX_SIDE */
    int32_t coef[9];
    int32_t y_offset;        /* 0 .. 255 */
} vghy_pack_job;

VGHY_API const char* vghy_version(void);
VGHY_API const char* vghy_last_error(void);

/* Bytes of device workspace vghy_anonymize needs for this job, a multiple of 16, each part starting at a multiple of 16: the luma owner map where the library
 * paints it (4 H W); pixelate: one byte per luma cell and two per chroma cell; blur: one byte per sample of every luma box clipped to its plane and two per
 * sample of every clipped chroma box, then the u16 h rows of every clipped box extended by r rows up and down (clamped to the plane), one u16 a luma sample and
 * two a chroma sample.  0 for a job vghy_anonymize would refuse (the message says why); a valid job needs at least 16.  No GPU is needed. */
VGHY_API int64_t vghy_anonymize_workspace_bytes(const vghy_anonymize_job* job);

/* The destination planes = the source planes with every head anonymised.  `workspace_dev`: caller-owned device memory of at least
 * vghy_anonymize_workspace_bytes(job) bytes, 16-byte aligned, used by this call alone until its work on `stream` has run.  The library allocates nothing but its
 * small per-device staging block for the head rows and taps.  Everything is checked before anything is queued, and the checks need no GPU: null pointers,
 * sizes, steps, pitches, sides and caps out of range, a tap offset outside the table, a negative tap or a tap sum other than 65536, more than VGHY_MAX_HEADS
 * heads, a destination plane that overlaps a source plane without being exactly it, a misaligned workspace; each refusal returns VGHY_ERR_INVALID with its
 * message. */
VGHY_API int vghy_anonymize(const vghy_anonymize_job* job, void* workspace_dev, void* stream);

/* RGB -> YUV 4:2:0 by the packer's rule: one launch, no workspace, nothing staged.  Refused with VGHY_ERR_INVALID before anything is queued: null pointers,
 * sizes, steps and pitches out of range, a coefficient beyond +-2^20, y_offset outside 0 .. 255, a destination plane that overlaps the source. */
VGHY_API int vghy_pack_rgb(const vghy_pack_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
