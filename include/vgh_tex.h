/* vgh_tex.h -- libvghtex.so: head textures for the MI355X head detector (gfx950 only).
 *
 * The fourth library of the package, next to libvgh.so (include/vgh.h, the detector), libvghview.so (include/vgh_view.h, pictures of the result) and
 * libvghvis.so (include/vgh_vis.h, visibility buffers).  This one moves colour between a photograph and the surface of the heads found in it: it paints
 * meshes from a texture image through per-vertex texture coordinates.  It links no object of the other three and none of them loads it.  Every export
 * carries the prefix vghtex_; everything else has hidden visibility.
 *
 * Conventions as in vgh_vis.h: functions return VGHTEX_OK (0) or a negative code, vghtex_last_error() gives the message of the calling thread's last
 * failure, `stream` is a hipStream_t (NULL = the default stream), work is queued on it and not waited for.
 */
#ifndef VGH_TEX_H
#define VGH_TEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VGHTEX_API __attribute__((visibility("default")))
#else
#define VGHTEX_API
#endif

#define VGHTEX_OK 0
#define VGHTEX_ERR_INVALID (-1)
#define VGHTEX_ERR_HIP (-2)
#define VGHTEX_ERR_NOMEM (-3)

#define VGHTEX_MAX_SIDE 32767 /* pixel coordinates travel as int16; the texture's sides have the same limit */
#define VGHTEX_MAX_HEADS 65536
#define VGHTEX_MAX_CHANNELS 16

#define VGHTEX_MODE_ORDER 0 /* a later head paints over an earlier one (PNCCProcessor.__call__, render_mesh) */
#define VGHTEX_MODE_DEPTH 1 /* one z-buffer shared by all heads */

#define VGHTEX_MAP_NEAREST 0  /* mapping_type 0 of the source */
#define VGHTEX_MAP_BILINEAR 1 /* any other mapping_type of the source */

#define VGHTEX_TEX_F32 0
#define VGHTEX_TEX_U8 1 /* a texel is converted to float exactly: the result is the one of the source fed texture.astype(float32) */

/* Sim3DR's render_texture (head_detector/Sim3DR/lib/rasterize_kernel.cpp, _render_texture_core) for n meshes of one topology: the result equals calling
 * it once per head, in head order.  One call of it, for every triangle t in index order:
 *   corners    p_k = (x, y) of vertices[triangles[3 t + k]], depth d_k = z_sign * z of the same vertex;
 *              texture corner q_k = (tex_coords[3 * tex_triangles[3 t + k]], tex_coords[3 * triangles[3 t + k] + 1]): x through the texture's triangle
 *              list, y through the MESH's (the source's indexing, kept as it is; tex_coords has stride 3, its third column is never read)
 *   box        x in max((int)ceil(min x), 0) .. min((int)floor(max x), width - 1), y alike; empty = the triangle is skipped.  A triangle with a non-finite
 *              x or y is skipped.
 *   per pixel (x, y) of the box:
 *     u, v     get_point_weight's: v0 = p2 - p0, v1 = p1 - p0, v2 = p - p0, inv = 1 / (dot00 * dot11 - dot01 * dot01), or 0 when that determinant is 0,
 *              u = (dot11 * dot02 - dot01 * dot12) * inv, v = (dot00 * dot12 - dot01 * dot02) * inv; weights w0 = 1 - u - v, w1 = v, w2 = u
 *     inside   x < 2 || x > width - 3 || y < 2 || y > height - 3 || (u >= 0 && v >= 0 && u + v < 1): inside a frame two pixels wide EVERY pixel of the box
 *              counts (the source's quirk, kept); a zero-determinant triangle has u = v = 0 and holds every pixel of its box
 *     depth    d = (w0 * d0 + w1 * d1) + w2 * d2; the pixel is painted when d > the pixel's depth (strict; NaN never wins), and the depth becomes d
 *     position q = (q0 * w0 + q1 * w1) + q2 * w2 per component, then x = max(min(x, tex_width - 1), 0), y = max(min(y, tex_height - 1), 0)
 *              (std::min / std::max: a NaN stays a NaN)
 *     colour   per channel k < channels, from texel(row, col) = texture[(row * tex_width + col) * tex_channels + k]:
 *              NEAREST   texel((int)round(y), (int)round(x)), halves away from zero
 *              BILINEAR  xd = x - floor(x), yd = y - floor(y), ul = texel(floor y, floor x), ur = texel(floor y, ceil x), dl = texel(ceil y, floor x),
 *                        dr = texel(ceil y, ceil x):  ((ul * (1 - xd) * (1 - yd) + ur * xd * (1 - yd)) + dl * (1 - xd) * yd) + dr * xd * yd, products left to right
 * All arithmetic is float32 in the source's operation order without contraction.  Non-finite texture coordinates or z give unspecified colours; the
 * integer texel indices are clamped into the texture, so nothing outside it is ever read.
 *
 * Composition over heads (the SOLO pass of head i = one such call on a fresh depth buffer of -1e8):
 *   mode ORDER: one call per head, in order, on the same image, each from a fresh depth of -1e8: a later head paints over an earlier one wherever its solo
 *               pass paints.  depth / triangle / head end as the last painting head left them.
 *   mode DEPTH: one call per head, in order, on the same image AND the same depth buffer (strict >: on equal depth the earlier head and the earlier triangle
 *               keep the pixel).
 *   dst_per_head = 1: head i paints slice i of dst / depth / triangle / head [n_heads, height, width, ...] and nothing else; the two modes coincide.
 * A pixel no triangle wins keeps its dst value; its depth is -1e8, its triangle and head are -1.  A painted pixel gets the colour of the last triangle that
 * won it, that triangle's index and its head's index.
 *
 * Every output pixel is owned by one thread that visits heads, then triangles, in index order: no float atomics, a deterministic result.  The number
 * of launches does not depend on n_heads.
 *
 * bounds: host, per head (x0, y0, x1, y1), inclusive, inside the image, x1 < x0 or y1 < y0 = the head covers nothing.  A CONTRACT, the one of
 * vghvis_job.bounds: every pixel the head can cover lies inside them (max(ceil(min x), 0) .. min(floor(max x), width - 1) over the vertices its
 * triangles name, y alike); pixels outside them are not visited for that head. */
typedef struct vghtex_job {
    int32_t height, width;        /* of dst: 1 .. VGHTEX_MAX_SIDE */
    int32_t channels;             /* c of dst: 1 .. VGHTEX_MAX_CHANNELS */
    int32_t n_heads;              /* 0 .. VGHTEX_MAX_HEADS; 0 paints nothing */
    int32_t n_vertices;           /* V */
    int32_t n_triangles;          /* T; 0 paints nothing */
    int32_t n_tex_vertices;       /* Vt */
    int32_t tex_height, tex_width; /* 1 .. VGHTEX_MAX_SIDE */
    int32_t tex_channels;         /* >= channels; the first `channels` of a texel are used */
    int32_t tex_dtype;            /* VGHTEX_TEX_F32 or VGHTEX_TEX_U8 */
    int32_t tex_per_head;         /* 0: one texture for all heads, 1: texture_dev is [n_heads, ...] */
    int32_t tex_coords_per_head;  /* 0: one set of texture coordinates for all heads, 1: tex_coords_dev is [n_heads, ...] */
    int32_t dst_per_head;         /* 0: all heads go into one image, 1: head i owns slice i of every destination */
    int32_t mapping;              /* VGHTEX_MAP_NEAREST or VGHTEX_MAP_BILINEAR */
    int32_t mode;                 /* VGHTEX_MODE_ORDER or VGHTEX_MODE_DEPTH */
    float z_sign;                 /* +1 or -1 */
    const float* verts_dev;       /* f32 [n_heads, V, 3] on the device; never written */
    const int32_t* triangles;     /* host, [T, 3]: indices < V and < Vt (a corner's texture y is read through them), shared by all heads */
    const float* tex_coords_dev;  /* f32 [n_heads or 1, Vt, 3] on the device; never written */
    const int32_t* tex_triangles; /* host, [T, 3]: indices < Vt */
    const void* texture_dev;      /* f32 or u8 [n_heads or 1, tex_height, tex_width, tex_channels] on the device; never written */
    const int32_t* bounds;        /* host, [n_heads, 4] */
    float* dst_dev;               /* f32 [height, width, channels] or [n_heads, height, width, channels] on the device; only painted pixels are written */
    float* depth_dev;             /* f32 [height, width] or [n_heads, height, width] on the device */
    int32_t* triangle_dev;        /* i32, shaped like depth_dev, or NULL */
    int32_t* head_dev;            /* i32, shaped like depth_dev, or NULL */
} vghtex_job;

VGHTEX_API const char* vghtex_version(void);
VGHTEX_API const char* vghtex_last_error(void);

/* Everything is checked (null pointers, sizes, flags, z_sign, every index of both triangle lists, every head's bounds against the image) before anything
 * is queued; the checks need no GPU. */
VGHTEX_API int vghtex_render_texture(const vghtex_job* job, void* stream);

#ifdef __cplusplus
}
#endif
#endif
