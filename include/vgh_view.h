/* vgh_view.h -- libvghview.so: result-side image helpers for the MI355X head detector (gfx950 only).
 *
 * A companion of libvgh.so (include/vgh.h), not a part of it: libvgh.so never loads it, it links none of libvgh's objects, and a client of
 * the detector's C ABI that wants no image helpers never pays for it.  Every export carries the prefix vghv_; everything else in the
 * library has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHV_OK (0) or a negative code, vghv_last_error() gives the message of the calling thread's
 * last failure, `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_VIEW_H
#define VGH_VIEW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHV_API __attribute__((visibility("default")))
#else
#define VGHV_API
#endif

#define VGHV_OK 0
#define VGHV_ERR_INVALID (-1)
#define VGHV_ERR_HIP (-2)
#define VGHV_ERR_NOMEM (-3)

#define VGHV_MAX_SIDE 32767 /* source coordinates travel as int16 in the arithmetic this restates */

/* One crop of an affinely warped u8 RGB image: OpenCV's 8-bit warpAffine(src, M, dsize, INTER_LINEAR), constant-0 border, evaluated only for
 * the crop_w x crop_h pixels that are kept.  The caller supplies the fixed-point tables of those pixels (all int32, built in double on the
 * host with round-half-to-even, A | b = the inverse of M, (cx, cy) = the crop's origin on the warped canvas):
 *     adelta[i] = rint(A00 * (cx + i) * 1024)                  i < crop_w
 *     bdelta[i] = rint(A10 * (cx + i) * 1024)                  i < crop_w
 *     x0[j]     = rint((A01 * (cy + j) + b0) * 1024) + 16      j < crop_h
 *     y0[j]     = rint((A11 * (cy + j) + b1) * 1024) + 16      j < crop_h
 * laid out [adelta | bdelta | x0 | y0] from tables[table_offset].  The kernel itself is integer arithmetic only.  An identity matrix makes the
 * crop a plain copy of src[cy : cy + crop_h, cx : cx + crop_w]. */
typedef struct vghv_crop {
    const uint8_t* src_dev;  /* u8 [src_h, src_w, 3] on the device */
    int64_t src_pitch_bytes; /* >= src_w * 3: distance of two rows (strided views are fine) */
    int32_t src_h, src_w;    /* 1 .. VGHV_MAX_SIDE */
    int32_t src_channels;    /* 3 */
    int32_t crop_w, crop_h;  /* >= 0; a crop with an empty side writes nothing */
    int64_t table_offset;    /* first of this crop's 2 * crop_w + 2 * crop_h entries in `tables` */
    int64_t dst_offset;      /* byte offset in dst_dev of the dense [crop_h, crop_w, 3] result */
} vghv_crop;

VGHV_API const char* vghv_version(void);
VGHV_API const char* vghv_last_error(void);

/* All n crops in ONE launch (descriptors, tile list and tables travel in one upload).  `tables` is host memory with n_tables entries; every
 * crop's table range must lie inside it and every crop's result inside dst_bytes (checked before anything is queued; results must not overlap). */
VGHV_API int vghv_warp_crops(const vghv_crop* crops, int n, const int32_t* tables, int64_t n_tables, uint8_t* dst_dev, int64_t dst_bytes, void* stream);

/* ---- drawing: PredictionResult.draw ---------------------------------------------------------------------------------------------------------
 * A copy of a u8 image with, for every head in order, up to three classes of primitives painted over it in this order (a later class paints
 * over an earlier one, a later head over an earlier head), with the pixel sets of OpenCV's
 *   class 0 box    cv2.rectangle(img, (x, y), (x + w, y + h), (255, 0, 0), 2)                          when boxes != NULL
 *   class 1 wire   cv2.polylines(img, [triangle], isClosed=True, color=(0, 0, 255), thickness=1)       for every row of triangles, n_triangles > 0
 *   class 2 dots   cv2.circle(img, point[indices[k]], radius, (255, 255, 255), -1)                    for every index, n_indices > 0
 * (colours go to channels 0, 1, 2 as written).  All primitives are expanded on the device from what this struct points to; the number of
 * launches does not depend on n_heads.  Painter's order is kept by an order key per pixel (1 + 3 * head + class, atomic max over a u32 plane of
 * library scratch) and a resolve pass that writes colour or source pixel to dst.  Exact rules: tests/draw_ref.py. */
#define VGHV_MAX_COORD 16777216 /* |point|, |box x, y| < 2^24; 0 <= box w, h < 2^24 */
#define VGHV_MAX_RADIUS 32
#define VGHV_MAX_DRAW_HEADS 65536

typedef struct vghv_draw_job {
    const uint8_t* src_dev;     /* u8 [height, width, 3] on the device */
    int64_t src_pitch_bytes;    /* >= width * 3 */
    uint8_t* dst_dev;           /* u8 [height, width, 3] on the device, dense, 4-byte aligned, not overlapping src */
    int32_t height, width;      /* 1 .. VGHV_MAX_SIDE */
    int32_t channels;           /* 3 */
    int32_t n_heads;            /* 0 .. VGHV_MAX_DRAW_HEADS; 0 makes dst a copy of src */
    int32_t n_vertices;         /* V: points per head */
    int32_t n_triangles;        /* T, 0 = no wire */
    int32_t n_indices;          /* K, 0 = no dots */
    int32_t radius;             /* 1 .. VGHV_MAX_RADIUS when n_indices > 0 */
    const int32_t* points;      /* host, [n_heads, V, 2]: x, y in pixels */
    const int32_t* boxes;       /* host, [n_heads, 4]: x, y, w, h; NULL = no boxes */
    const int32_t* triangles;   /* host, [T, 3]: indices < V, shared by all heads */
    const int32_t* indices;     /* host, [K]: indices < V, shared by all heads */
    const int32_t* half_widths; /* host, [radius + 1]: half the width of the filled circle's row at distance j from its centre row, 0 .. radius */
} vghv_draw_job;

/* Everything is checked (every index against V, every coordinate against VGHV_MAX_COORD) before anything is queued. */
VGHV_API int vghv_draw_heads(const vghv_draw_job* job, void* stream);

/* ---- shaded mesh: Sim3DR's get_normal and its alpha-blended _rasterize ------------------------------------------------------------------------
 * Vertex normals of n meshes of one topology, bit for bit Sim3DR's _get_normal (head_detector/Sim3DR/lib/rasterize_kernel.cpp): every vertex adds
 * the un-normalised cross products of its triangles in ascending triangle index, then normalises (a length <= 0 is replaced by 1e-6).
 * verts_dev, normals_dev: float32 [n, V, 3] on the device (they must not overlap); triangles: host, int32 [T, 3], indices < V. */
VGHV_API int vghv_vertex_normals(const float* verts_dev, int n, int V, const int32_t* triangles, int T, float* normals_dev, void* stream);

/* One image; for every head in order one Sim3DR _rasterize(image, vertices, triangles, colours, depth = -1e8 everywhere, alpha, reverse):
 * per pixel, every triangle (in index order) whose integer bounding box holds the pixel, whose three barycentric weights are > 0 and whose
 * interpolated depth is > the running depth of this head paints  byte = (unsigned char)((1 - alpha) * byte + alpha * 255 * colour)  per channel
 * in float32 and becomes the running depth.  Depth = z_sign * z.  dst is a dense copy of src with the heads painted; the number of launches does
 * not depend on n_heads.
 * Colours: shade == 0: colors_dev holds the caller's float32 per-vertex colours, [V, 3] for all heads (colors_per_head == 0) or [n, V, 3] (== 1).
 *          shade == 1: colors_dev [n, V, 3] (colors_per_head must be 1) is WRITTEN by the call before it is used: with N the normal of the
 *          vertices whose z is multiplied by z_sign,  s = |(Nx * light[0] + Ny * light[1]) + Nz * light[2]|,  t = min(1, ambient + diffuse * s),
 *          colour_k = t * color[k], all float32 without contraction.
 * bounds: host, per head (x0, y0, x1, y1), inclusive, inside the image, x1 < x0 or y1 < y0 = the head paints nothing.  A CONTRACT: every pixel
 * the head can paint lies inside them (max(ceil(min x), 0) .. min(floor(max x), width - 1) over the vertices its triangles name, y alike);
 * pixels outside them are not painted for that head. */
typedef struct vghv_mesh_job {
    const uint8_t* src_dev;   /* u8 [height, width, 3] on the device */
    int64_t src_pitch_bytes;  /* >= width * 3 */
    uint8_t* dst_dev;         /* u8 [height, width, 3] on the device, dense, not overlapping src */
    int32_t height, width;    /* 1 .. VGHV_MAX_SIDE */
    int32_t channels;         /* 3 */
    int32_t n_heads;          /* 0 .. VGHV_MAX_DRAW_HEADS; 0 makes dst a copy of src */
    int32_t n_vertices;       /* V */
    int32_t n_triangles;      /* T; 0 makes dst a copy of src */
    int32_t reverse;          /* 0 / 1: pixel (x, y) is read from and written to row height - 1 - y */
    int32_t colors_per_head;  /* 0 / 1 */
    int32_t shade;            /* 0 / 1 */
    float alpha;              /* 0 .. 1 */
    float z_sign;             /* +1 or -1 */
    float ambient, diffuse;   /* shade == 1: finite, >= 0 */
    const float* verts_dev;   /* f32 [n_heads, V, 3] on the device */
    const int32_t* triangles; /* host, [T, 3]: indices < V, shared by all heads */
    const int32_t* bounds;    /* host, [n_heads, 4] */
    float* colors_dev;        /* f32 on the device, read (shade == 0) or written and read (shade == 1) */
    float color[3];           /* shade == 1: 0 .. 1 */
    float light[3];           /* shade == 1: finite; the caller normalises it */
} vghv_mesh_job;

/* Everything is checked (every triangle index against V, every head's bounds against the image) before anything is queued. */
VGHV_API int vghv_render_meshes(const vghv_mesh_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
