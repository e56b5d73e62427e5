/* vgh_osd.h -- libvghosd.so: the on-screen display of the MI355X head detector (gfx950 only): boxes, bars and bitmap text written into the planes a frame
 * already lies in (the Y, U and V planes of an 8-bit YUV 4:2:0 frame, or the three byte planes of an RGB image), in place if wanted.
 *
 * The eleventh library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so, libvghvis.so, libvghtex.so, libvgheval.so, libvghmerge.so,
 * libvghtrack.so, libvghanon.so, libvghvideo.so and libvghcrop.so.  It links no object of the other libraries, includes none of their headers and none of them
 * loads it.  Every export carries the prefix vgho_; everything else has hidden visibility.  Integer arithmetic only.
 *
 * Conventions as in vgh.h: functions return VGHO_OK (0) or a negative code, vgho_last_error() gives the message of the calling thread's last failure,
 * `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_OSD_H
#define VGH_OSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHO_API __attribute__((visibility("default")))
#else
#define VGHO_API
#endif

#define VGHO_OK 0
#define VGHO_ERR_INVALID (-1)
#define VGHO_ERR_HIP (-2)
#define VGHO_ERR_NOMEM (-3)

#define VGHO_MAX_SIDE 32767      /* height and width of a target; the sides of an item's box */
#define VGHO_MAX_COORD 16777215  /* |coordinate| of an item's box (< 2^24) */
#define VGHO_MAX_ITEMS 65536     /* n_items of one call */
#define VGHO_MAX_PLANES 3
#define VGHO_MAX_TEXT 64         /* glyph codes of one TEXT item */
#define VGHO_MAX_SCALE 16        /* integer scale of a TEXT item */
#define VGHO_MAX_ALPHA 256       /* opaque */
#define VGHO_MAX_TILES 16777216  /* (item, 16 x 16 tile) pairs of one call (2^24: the tile list of one launch) */
#define VGHO_GLYPHS 44           /* space, 0-9, A-Z, # % . : - + / in this order */
#define VGHO_GLYPH_ROWS 7
#define VGHO_GLYPH_COLS 5
#define VGHO_GLYPH_PITCH 6       /* columns from one glyph of a run to the next: the sixth is blank */

#define VGHO_BAR 0  /* every position of the box */
#define VGHO_RECT 1 /* an inward band of `thickness` positions along the four edges of the box */
#define VGHO_TEXT 2 /* a run of glyph codes at an integer scale */

/* THE RULE (the single statement of it; tests/osd_ref.py restates it in NumPy and the device equals that bit for bit).
 *
 * TARGET.  height x width "luma" positions and n_planes planes (1 .. 3).  Plane p has a shift s of 0 or 1 and ((height + (1 << s) - 1) >> s) rows of
 * ((width + (1 << s) - 1) >> s) samples; sample (py, px) is the byte at src_dev + py * src_pitch + px * src_step (read) and dst_dev + py * dst_pitch +
 * px * dst_step (written); steps are 1, 2 or 3.  An RGB image is three planes of shift 0 and step 3 whose pointers lie one byte apart; NV12, NV21 and I420 are
 * a Y plane of shift 0 and step 1 and U and V planes of shift 1 and step 2 or 1.  Nothing in the library knows one kind of target from the other.
 *
 * ITEMS are drawn in index order: a later item lies over an earlier one.  Item i has a box (x0, y0, x1, y1) in luma positions, half-open and NOT clipped
 * (sides 0 .. VGHO_MAX_SIDE, |coordinate| <= VGHO_MAX_COORD), one colour byte per plane, an alpha of 0 .. 256 and covers these positions (x, y) of its box:
 *   VGHO_BAR   all of them.
 *   VGHO_RECT  those with min(x - x0, x1 - 1 - x, y - y0, y1 - 1 - y) < thickness; thickness >= 1, and a band at least as thick as half the shorter side
 *              fills the box.
 *   VGHO_TEXT  a run of `length` codes (1 .. 64), codes[code_offset ..], at an integer `scale` (1 .. 16); its box is exactly (6 * scale * length - scale) wide
 *              and 7 * scale high.  With u = (x - x0) / scale and v = (y - y0) / scale (integer division): u % 6 < 5 and bit (u % 6) of
 *              font[codes[code_offset + u / 6]][v] is set.  Bit 0 of a font row is the glyph's LEFT column.  vgho_font() gives the table.
 * A position outside the target is covered by nothing.
 *
 * KEY.  K[y, x] = 1 + the largest index of an item that covers (x, y), 0 where none does.
 * OWNER of sample (py, px) of a plane of shift s: the maximum of K over the positions {py << s ..} x {px << s ..} (1 or 4 of them) that lie in the target,
 * minus 1.  For s = 0 that is the key itself; for the chroma planes of a 4:2:0 frame it is vgh_video.h's rule: the latest item that touches any of the (up to)
 * four luma pixels the sample colours.  -1 = nobody.
 * WRITTEN VALUE.  A sample with owner i >= 0, c = items[i].color[plane] and a = items[i].alpha becomes
 *     dst = (src * (256 - a) + c * a + 128) >> 8
 * The owner is blended ONCE with the SOURCE, never with an item below it: a = 256 gives c exactly, a = 0 gives src (a transparent top item still owns its
 * samples and leaves them as the source).  The result does not depend on scheduling.
 *
 * IN PLACE AND OUT OF PLACE, per plane, as in vgh_video.h: a destination plane is either exactly its source plane (same pointer, pitch and step) or overlaps
 * no source plane; anything else is refused.  In place only owned samples are written and no byte between a row's last sample and the pitch is touched; out of
 * place the plane's samples are copied first and the owned samples are then written.
 */
typedef struct vgho_plane {
    const uint8_t* src_dev; /* device */
    uint8_t* dst_dev;       /* device; == src_dev (with the same pitch and step): in place */
    int64_t src_pitch;      /* bytes between rows; >= (plane width - 1) * src_step + 1 */
    int64_t dst_pitch;
    int32_t src_step;       /* bytes between samples of a row: 1, 2 or 3 */
    int32_t dst_step;
    int32_t shift;          /* 0 or 1 */
    int32_t reserved;       /* 0 */
} vgho_plane;

typedef struct vgho_item {
    int32_t kind;           /* VGHO_BAR, VGHO_RECT or VGHO_TEXT */
    int32_t x0, y0, x1, y1; /* half-open, luma positions, not clipped */
    int32_t thickness;      /* RECT: >= 1; otherwise 0 */
    int32_t scale;          /* TEXT: 1 .. VGHO_MAX_SCALE; otherwise 0 */
    int32_t code_offset;    /* TEXT: the run is codes[code_offset .. code_offset + length); otherwise 0 */
    int32_t length;         /* TEXT: 1 .. VGHO_MAX_TEXT; otherwise 0 */
    int32_t alpha;          /* 0 .. VGHO_MAX_ALPHA */
    uint8_t color[3];       /* one byte per plane, in the order of the job's planes */
    uint8_t reserved;       /* 0 */
} vgho_item;

typedef struct vgho_job {
    vgho_plane planes[VGHO_MAX_PLANES]; /* the first n_planes are used */
    int32_t height, width;              /* 1 .. VGHO_MAX_SIDE */
    int32_t n_planes;                   /* 1 .. VGHO_MAX_PLANES */
    int32_t n_items;                    /* 0 .. VGHO_MAX_ITEMS */
    const vgho_item* items;             /* host, [n_items] */
    const uint8_t* codes;               /* host, [n_codes]: glyph codes, each < VGHO_GLYPHS */
    int32_t n_codes;                    /* >= 0 */
    int32_t reserved;                   /* 0 */
} vgho_job;

VGHO_API const char* vgho_version(void);
VGHO_API const char* vgho_last_error(void);

/* Bytes of the caller-owned workspace vgho_draw needs for this job (the key plane: uint32 [height, width], a multiple of 16, at least 16), or 0 with a message
 * for a job vgho_draw would refuse.  Needs no GPU. */
VGHO_API int64_t vgho_workspace_bytes(const vgho_job* job);

/* Draws the job's items.  workspace_dev: device memory of vgho_workspace_bytes(job) bytes, 16-byte aligned, holding ANYTHING (nothing of it is assumed clear,
 * and no pass clears more of it than the items' tiles).  A call queues a fixed sequence whatever n_items is: one staging upload (items, codes, font, the
 * (item, 16 x 16 tile) list), the copies of the planes that are out of place, a key clear over the items' tiles, a paint pass and one write pass per distinct
 * shift; n_items = 0 queues nothing in place and the copies alone out of place.  In place no pass walks the target: the work scales with what is drawn.
 * Everything is checked before anything is queued, and the checks need no GPU: null pointers, sizes, steps, shifts, pitches, caps, a code outside the font, a
 * code range outside `codes`, a TEXT box that is not its run's size, an alpha out of range, a misaligned workspace, a destination that overlaps a source
 * without being in place; each refusal returns VGHO_ERR_INVALID with a message that names the item and the field. */
VGHO_API int vgho_draw(const vgho_job* job, void* workspace_dev, void* stream);

/* The seven row bytes of glyph `code` (0 .. VGHO_GLYPHS - 1), bit 0 = the left column; VGHO_ERR_INVALID for any other code.  Needs no GPU. */
VGHO_API int vgho_font(int32_t code, uint8_t rows_out[7]);

#ifdef __cplusplus
}
#endif
#endif
