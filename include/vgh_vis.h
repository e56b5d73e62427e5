/* vgh_vis.h -- libvghvis.so: head visibility buffers for the MI355X head detector (gfx950 only).
 *
 * The third library of the package, next to libvgh.so (include/vgh.h, the detector) and libvghview.so (include/vgh_view.h, pictures of the result).
 * This one returns measurements: which head and which triangle a pixel shows, where on the triangle, and how much of every head can be seen.  It
 * links no object of the other two and neither of them loads it.  Every export carries the prefix vghvis_; everything else has hidden visibility.
 *
 * Conventions as in vgh.h: functions return VGHVIS_OK (0) or a negative code, vghvis_last_error() gives the message of the calling thread's last
 * failure, `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_VIS_H
#define VGH_VIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHVIS_API __attribute__((visibility("default")))
#else
#define VGHVIS_API
#endif

#define VGHVIS_OK 0
#define VGHVIS_ERR_INVALID (-1)
#define VGHVIS_ERR_HIP (-2)
#define VGHVIS_ERR_NOMEM (-3)

#define VGHVIS_MAX_SIDE 32767 /* pixel coordinates travel as int16 */
#define VGHVIS_MAX_HEADS 65536

#define VGHVIS_MODE_ORDER 0 /* a later head paints over an earlier one (PNCCProcessor.__call__, render_mesh) */
#define VGHVIS_MODE_DEPTH 1 /* one z-buffer shared by all heads */

/* Sim3DR's rasterize_triangles (head_detector/Sim3DR/lib/rasterize_kernel.cpp, _rasterize_triangles) for n meshes of one topology.  One call of it,
 * per pixel: every triangle, in index order, whose integer bounding box holds the pixel and for which  u >= 0 && v >= 0 && u + v < 1  (is_point_in_tri;
 * u, v as in get_point_weight, so a zero-determinant triangle has u = v = 0 and holds every pixel of its box) and whose interpolated depth
 * (1 - u - v) * d0 + v * d1 + u * d2  is > the pixel's depth writes depth, triangle index and the weights (1 - u - v, v, u).  Depth = z_sign * z; all
 * arithmetic is float32 in the source's operation order without contraction.  A triangle with a non-finite x or y is skipped.
 *
 * The SOLO result of head i is one such call on fresh buffers (depth -1e8, triangle -1).
 *   mode ORDER: heads are composited in order: where head i's solo triangle is >= 0, its head index, triangle, depth and weights replace what is there.
 *   mode DEPTH: one call per head, in order, on the SAME buffers; head i owns the pixels whose depth changed during its call (strict >: on equal depth
 *               the earlier head and the earlier triangle keep the pixel; NaN never wins).
 * Background: depth -1e8, triangle -1, head -1, weights 0.
 *   covered_px[i]        pixels with triangle >= 0 in head i's solo result (both modes)
 *   visible_px[i]        pixels head i owns at the end
 *   vertex_visible[i, v] 1 when v is a corner of a triangle t such that some pixel ends with owner (i, t), else 0
 * The number of launches does not depend on n_heads.
 *
 * bounds: host, per head (x0, y0, x1, y1), inclusive, inside the image, x1 < x0 or y1 < y0 = the head covers nothing.  A CONTRACT, the one of
 * vghv_mesh_job.bounds: every pixel the head can cover lies inside them (max(ceil(min x), 0) .. min(floor(max x), width - 1) over the vertices its
 * triangles name, y alike); pixels outside them are not visited for that head. */
typedef struct vghvis_job {
    int32_t height, width;       /* 1 .. VGHVIS_MAX_SIDE */
    int32_t n_heads;             /* 0 .. VGHVIS_MAX_HEADS; 0 leaves pure background */
    int32_t n_vertices;          /* V */
    int32_t n_triangles;         /* T; 0 leaves pure background */
    int32_t mode;                /* VGHVIS_MODE_ORDER or VGHVIS_MODE_DEPTH */
    float z_sign;                /* +1 or -1 */
    const float* verts_dev;      /* f32 [n_heads, V, 3] on the device; never written */
    const int32_t* triangles;    /* host, [T, 3]: indices < V, shared by all heads */
    const int32_t* bounds;       /* host, [n_heads, 4] */
    float* depth_dev;            /* f32 [height, width] on the device */
    int32_t* triangle_dev;       /* i32 [height, width] on the device */
    int32_t* head_dev;           /* i32 [height, width] on the device */
    float* bary_dev;             /* f32 [height, width, 3] on the device, or NULL */
    int32_t* visible_px_dev;     /* i32 [n_heads] on the device, or NULL */
    int32_t* covered_px_dev;     /* i32 [n_heads] on the device, or NULL */
    uint8_t* vertex_visible_dev; /* u8 [n_heads, V] on the device, or NULL */
} vghvis_job;

VGHVIS_API const char* vghvis_version(void);
VGHVIS_API const char* vghvis_last_error(void);

/* Everything is checked (null pointers, sizes, mode, z_sign, every triangle index against V, every head's bounds against the image) before anything
 * is queued; the checks need no GPU. */
VGHVIS_API int vghvis_rasterize_triangles(const vghvis_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
