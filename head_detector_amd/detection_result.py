"""PredictionResult with the reference's surface (head_detector/detection_result.py:38-81).  ``heads`` is the
accelerated product.  ``get_pncc`` runs the HIP z-buffer rasteriser (csrc/raster.hip = the reference's Sim3DR kernel,
SURVEY.md 8(f) N3) and needs the reference's mesh assets (user-supplied, see ``head_detector_amd.pncc.MeshAssets``);
``save_meshes`` is pure file IO.  ``get_aligned_heads`` plans every head's crop on the host and warps all of them in one launch of
csrc/aligned.hip (libvghview.so, ``head_detector_amd.aligned``); it needs ``head_indices`` (assets/flame_indices/head_indices.npy of the
reference, user-supplied like the other mesh assets).  ``draw`` paints boxes, the mesh wireframe and landmark dots over a copy of the image
with the kernels of csrc/draw.hip (libvghview.so, ``head_detector_amd.draw``) for the methods "full", "bbox", "landmarks" and "points"; it needs
``triangles`` (assets/triangles.txt), ``head_indices`` and ``face_indices`` (assets/flame_indices/face.npy) as the method requires.  Its pixel
rules are OpenCV's as restated in tests/draw_ref.py (parity with cv2 itself is unpinned, like the warp of the aligned crops); "pose" raises
NotImplementedError instead of drawing something approximately right.  ``get_visibility`` measures instead of painting: per pixel the head and
triangle that show, per head the covered and the visible pixels and the visible vertices (csrc/visibility.hip, libvghvis.so,
``head_detector_amd.visibility``); like ``render_mesh`` it needs ``faces``.  ``get_textures`` and ``render_texture`` move colour between the photograph
and the heads' surface with Sim3DR's ``render_texture`` (csrc/texture.hip, libvghtex.so, ``head_detector_amd.texture``): the first cuts every head's UV
texture map out of the image, the second paints textures back onto the heads; both need ``faces`` and a per-vertex UV layout (``texture.cylindrical_uv``
makes one from the template mesh).  ``compare_meshes`` judges the heads against ground-truth meshes with the reference's benchmark metrics (Z_n, chamfer;
csrc/mesh_metrics.hip, libvgheval.so, ``head_detector_amd.mesh_metrics``).  ``detection_rows`` gives the boxes as the detection benchmarks take them
(``head_detector_amd.detection_metrics``: COCO-style AP, csrc/detection_ap.hip).  ``anonymize`` returns the image with every head pixelated, blurred or filled, by
box, ellipse or mesh silhouette (csrc/anonymize.hip, libvghanon.so, ``head_detector_amd.anonymize``): integer arithmetic only, a later head owns an overlap.
``get_head_tensors`` hands the heads to a next model: fixed-size, normalised crops of every head in one dense GPU tensor, cut from the image or from the video
frame's own planes in one launch (csrc/head_tensors.hip, libvghcrop.so, ``head_detector_amd.head_tensors``).  ``draw_overlay`` shows the result where it goes on:
boxes, label bars and bitmap text (track ids, scores) written into the video frame's own YUV planes or into the RGB image, in place if wanted (csrc/osd.hip,
libvghosd.so, ``head_detector_amd.overlay``)."""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np

from .head_info import HeadMetadata


class PredictionResult:
    def __init__(self, original_image: np.ndarray, heads: List[HeadMetadata], faces: Optional[np.ndarray] = None, pncc_processor=None, *,
                 head_indices: Optional[np.ndarray] = None, triangles: Optional[np.ndarray] = None, face_indices: Optional[np.ndarray] = None, source_frame=None):
        self.original_image = original_image  # (None for a frame input with rgb="none": no RGB copy was made)
        self.source_frame = source_frame  # the video.YUV420Frame / YUV420Frame16 the result was made from, or None (an RGB input)
        self.heads = heads
        self._faces = faces  # [F,3] 0-based triangle indices of the FLAME mesh
        self.pncc_processor = pncc_processor  # head_detector_amd.pncc.PNCCProcessor or None (no mesh assets supplied)
        self.head_indices = head_indices  # vertex subset of refined_head_bbox and of the landmark dots, or None (no mesh assets supplied)
        self.triangles = triangles  # [T, 3] vertex indices of the wireframe drawn by draw(), or None
        self.face_indices = face_indices  # vertex subset drawn by draw("points"), or None

    def draw(self, method: str = "full", to_host: bool = True):
        """detection_result.py:45-51: a NEW uint8 [H, W, 3] image with every head drawn over a copy of the original, in the order of ``heads``:
        "bbox" the box; "landmarks" the mesh wireframe and the ``head_indices`` dots; "points" the ``face_indices`` dots; "full" box, wireframe and
        dots.  ``to_host=False`` returns a GPU ``torch.uint8`` tensor.  Any other method raises KeyError like the reference's lookup, "pose"
        NotImplementedError, a method whose mesh asset is missing ``draw.DrawAssetsMissing`` (a FileNotFoundError and a NotImplementedError)."""
        from .draw import draw_heads

        return draw_heads(self.original_image, self.heads, method, triangles=self.triangles, head_indices=self.head_indices, face_indices=self.face_indices, to_host=to_host)

    def render_mesh(self, alpha: float = 0.7, color=(0.75, 0.75, 0.8), ambient: float = 0.35, diffuse: float = 0.65, light=(0.0, 0.0, 1.0), to_host: bool = True):
        """A NEW uint8 [H, W, 3] image: every head's solid mesh, lit (two-sided Lambert term from Sim3DR's vertex normals) and blended with ``alpha`` by
        Sim3DR's rasteriser over a copy of the original, in the order of ``heads`` (``head_detector_amd.mesh_render`` states the composition).  Needs
        the FLAME model's own triangles (``faces``).  Neither the image nor any head's ``vertices_3d`` is modified.  ``to_host=False`` returns a GPU
        ``torch.uint8`` tensor."""
        from .mesh_render import render_mesh

        return render_mesh(self.original_image, self.heads, self._faces, alpha=alpha, color=color, ambient=ambient, diffuse=diffuse, light=light, to_host=to_host)

    def anonymize(self, method: str = "pixelate", region: str = "ellipse", *, margin: float = 0.1, cells: int = 8, strength: float = 0.1, color=(0, 0, 0), faces=None,
                  to_host: bool = True):
        """A NEW uint8 [H, W, 3] image: the original with every head hidden (csrc/anonymize.hip, libvghanon.so, ``head_detector_amd.anonymize`` states the
        rules).  ``method``: "pixelate" (``cells`` cells along the longer side), "blur" (an integer Gaussian of sigma ``strength`` times the longer side) or
        "fill" (``color``).  ``region``: "box" (the ``bbox`` grown by ``margin``), "ellipse" (inscribed in that box) or "mesh" (the head's own silhouette as
        ``get_visibility`` sees it; needs ``faces``, the FLAME model's own unless given; hair lies outside it).  A later head owns the pixels it shares with
        an earlier one.  The original is never modified; a GPU ``original_image`` is used where it is.  ``to_host=False`` returns a GPU ``torch.uint8``
        tensor.  A result made from a ``video.YUV420Frame`` is hidden in the frame's own planes by ``anonymize_frame``."""
        from .anonymize import anonymize_heads

        return anonymize_heads(self.original_image, self.heads, method, region, margin=margin, cells=cells, strength=strength, color=color,
                               faces=self._faces if faces is None else faces, to_host=to_host)

    def anonymize_frame(self, method: str = "pixelate", region: str = "ellipse", *, margin: float = 0.1, cells: int = 8, strength: float = 0.1, color=(0, 0, 0), faces=None,
                        out=None):
        """``video.anonymize_frame(self.source_frame, self.heads, ...)``: every head hidden directly in the luma and chroma planes of the YUV 4:2:0 frame the
        result was made from (csrc/yuv_anonymize.hip, libvghvideo.so), with the keywords of ``anonymize``; no RGB image is made or needed (``rgb="none"``).
        ``out=None``: a new frame; ``out=self.source_frame``: in place; another ``video.YUV420Frame`` of the same size: written whole.  Returns the frame
        written.  ValueError if the result was not made from a frame: use ``anonymize()`` then; and if the frame is a deep ``video.YUV420Frame16``: pass
        ``source_frame.to_8bit()`` to ``video.anonymize_frame``."""
        if self.source_frame is None:
            raise ValueError("anonymize_frame: this result was not made from a video.YUV420Frame (source_frame is None); use anonymize() on its RGB original_image")
        from .video import anonymize_frame, require_8bit_frame

        require_8bit_frame("anonymize_frame", self.source_frame)
        return anonymize_frame(self.source_frame, self.heads, method, region, margin=margin, cells=cells, strength=strength, color=color,
                               faces=self._faces if faces is None else faces, out=out)

    def get_visibility(self, occlusion: str = "order", barycentric: bool = False, to_host: bool = True):
        """A ``visibility.HeadVisibility``: Sim3DR's ``rasterize_triangles`` over every head's mesh (the FLAME model's own triangles, ``faces``), depth = -z
        like get_pncc and render_mesh.  ``occlusion="order"``: a later head hides an earlier one, as in those pictures (FLAME's weak-perspective z is not
        calibrated between heads); ``"depth"``: one z-buffer for all heads.  No head's ``vertices_3d`` is modified.  ``to_host=False`` returns GPU tensors."""
        from .visibility import head_visibility

        shape = tuple(self.original_image.shape)
        if len(shape) < 2:
            raise ValueError(f"the image must be [H, W, ...], got {shape}")
        return head_visibility(self.heads, self._faces, shape[0], shape[1], occlusion=occlusion, barycentric=barycentric, to_host=to_host)

    def get_textures(self, uv, size=256, mapping: str = "bilinear", visible_only: bool = True, occlusion: str = "order", faces=None, to_host: bool = True):
        """A ``texture.HeadTextures``: every head's appearance as a UV texture map [n, th, tw, C] cut out of the image (``texture.unwrap_heads`` with the
        head's ``vertices_3d`` as texture coordinates).  ``uv`` [V, 2] in [0, 1] per vertex, ``size`` the atlas side or (th, tw), ``faces`` a triangle list
        to use instead of the FLAME model's own (``faces[keep]`` of ``texture.cylindrical_uv``).  ``mask`` marks the texels that were written; with
        ``visible_only`` their triangle must also own a pixel of that head in ``get_visibility(occlusion)``.  Nothing is modified.  ``to_host=False``
        returns GPU tensors."""
        from .texture import head_textures

        return head_textures(self.original_image, self.heads, self._faces if faces is None else faces, uv, size=size, mapping=mapping, visible_only=visible_only,
                             occlusion=occlusion, to_host=to_host)

    def render_texture(self, textures, uv, mapping: str = "bilinear", occlusion: str = "order", faces=None, to_host: bool = True):
        """A NEW uint8 [H, W, 3] image: every head painted from its own texture (``textures`` [n, th, tw, C] or a ``HeadTextures``) or from a shared one
        ([th, tw, C]), uint8 or float, over a copy of the original, depth = -z, composed like ``render_mesh`` (``occlusion="order"``) or through one
        z-buffer (``"depth"``).  The float32 result is clamped to [0, 255] and truncated to bytes.  Neither the image nor any head is modified.
        ``to_host=False`` returns a GPU ``torch.uint8`` tensor."""
        from .texture import paint_heads

        return paint_heads(self.original_image, self.heads, self._faces if faces is None else faces, textures, uv, mapping=mapping, occlusion=occlusion, to_host=to_host)

    def compare_meshes(self, gt_vertices, subset=None, top_k: int = 5, neighbours: str = "reference", to_host: bool = True, *, gt_landmarks7=None,
                       pred_landmarks7=None, chamfer_subset=None):
        """A ``mesh_metrics.HeadMeshMetrics``: every head's ``vertices_3d`` against its ground-truth mesh ``gt_vertices`` [n, V, 3] (the same topology, in the
        heads' order).  ``z_n`` is the reference's ``calc_zn`` on the vertices ``subset`` (its head_indices; default: all), per head, with ``neighbours`` =
        "reference" (the source as written) or "nearest" (``mesh_metrics`` states both); the source's caller negates the ground truth first
        (evaluate_dad.py:294), which is left to the caller here too.  With ``gt_landmarks7`` and ``pred_landmarks7`` [n, 7, 3] ``chamfer`` is filled as
        well (``mesh_metrics.chamfer_to_gt``, ``chamfer_subset`` = the source's face.npy).  No head's ``vertices_3d`` is modified.  ``to_host=False``
        returns GPU tensors."""
        from .mesh_metrics import compare_heads

        return compare_heads(self.heads, gt_vertices, subset=subset, top_k=top_k, neighbours=neighbours, gt_landmarks7=gt_landmarks7,
                             pred_landmarks7=pred_landmarks7, chamfer_subset=chamfer_subset, to_host=to_host)

    def detection_rows(self) -> list:
        """``[[x, y, w, h, score], ...]`` of ``heads``, in their order: the rows the reference's detection benchmarks hand to COCOeval
        (evaluation/evaluate_wider.py: parse_predictions) and ``detection_metrics.DetectionEvaluator.add`` takes."""
        return [[head.bbox.x, head.bbox.y, head.bbox.w, head.bbox.h, float(head.score)] for head in self.heads]

    def get_pncc(self):
        """detection_result.py:58-59: PNCC image of all heads (uint8 [H,W,3]); like the reference it negates z of every
        head's ``vertices_3d`` in place."""
        if self.pncc_processor is None:
            raise FileNotFoundError("get_pncc needs the reference's mesh assets (full_faces.npy, v_template.npy, flame_indices/head_w_ears.npy): "
                                    "construct HeadDetector(..., assets_dir=<reference>/head_detector/assets)")
        return self.pncc_processor(self.original_image, self.heads)

    def get_aligned_heads(self, to_host: bool = True):
        """detection_result.py:56-70: one upright, square crop per head (rotated by the head's roll about its skull centre when ``abs(yaw) < 60``),
        uint8 [h, w, 3] with the reference's shapes and bytes -- a crop that its Python slice leaves empty is returned empty, so there is one
        per head.  ``to_host=False`` returns GPU ``torch.uint8`` tensors (views into one packed buffer) for a next model on the device."""
        if self.head_indices is None:
            raise FileNotFoundError("get_aligned_heads needs the reference's mesh asset flame_indices/head_indices.npy: "
                                    "construct HeadDetector(..., assets_dir=<reference>/head_detector/assets) or pass head_indices= to PredictionResult")
        from .aligned import get_aligned_heads

        return get_aligned_heads(self.original_image, self.heads, self.head_indices, to_host=to_host)

    def get_head_tensors(self, size: int = 224, **kw):
        """``head_tensors.head_tensors(source, self.heads, size, **kw)``: every head as one ``size`` x ``size`` crop of ONE dense, normalised GPU tensor for a next
        model ([n, 3, size, size] float32 by default; csrc/head_tensors.hip, libvghcrop.so), with the matrices back to image coordinates.  The source is the
        ``source_frame`` if the result was made from a video frame (its YUV planes are used where they are: ``original_image`` may be None), otherwise the
        ``original_image``.  ``aligned=True`` (the default: the geometry of ``get_aligned_heads``) needs ``head_indices`` -- the result's own unless given;
        ``aligned=False`` needs no asset.  A deep ``video.YUV420Frame16`` is not a source: the ``original_image`` is used, and without one (``rgb="none"``) a
        ValueError names ``source_frame.to_8bit()``.  Keywords and errors: ``head_tensors.head_tensors``."""
        from .head_tensors import head_tensors

        from .video import YUV420Frame16, require_8bit_frame

        kw.setdefault("head_indices", self.head_indices)
        source = self.source_frame
        if isinstance(source, YUV420Frame16):  # the crops are cut from 8-bit planes: the RGB original if there is one
            if self.original_image is None:
                require_8bit_frame("get_head_tensors", source)
            source = None
        return head_tensors(source if source is not None else self.original_image, self.heads, size, **kw)

    def draw_overlay(self, *, out=None, to_host: bool = False, **plan_kw):
        """``overlay.draw_heads(target, self.heads, out=out, **plan_kw)``: every head's box and, with ``labels="id"``, ``"score"``, ``"id+score"`` or one string
        per head, its label bar and text, written with integer arithmetic into the surface itself (csrc/osd.hip, libvghosd.so; ``head_detector_amd.overlay``
        states the rule and the keywords of ``head_overlay_plan``).  The target is the ``source_frame`` if the result was made from a video frame -- its YUV
        planes are drawn in where they lie, ``original_image`` may be None (``rgb="none"``), ``out=self.source_frame`` is in place and a ``video.YUV420Frame``
        is returned (with ``to_host=True`` its (y, u, v) planes as NumPy arrays) -- otherwise the ``original_image`` (a GPU ``torch.uint8`` tensor is returned, a
        NumPy array with ``to_host=True``).  A
        ``TrackedPredictionResult`` passes its ``track_ids`` and ``coasting`` by itself.  ``draw()`` remains the picture with the reference's look."""
        from .overlay import draw_heads

        if not isinstance(to_host, (bool, np.bool_)):
            raise ValueError(f"draw_overlay: to_host must be True or False, got {to_host!r}")
        for name in ("track_ids", "coasting"):
            if getattr(self, name, None) is not None:
                plan_kw.setdefault(name, getattr(self, name))
        from .video import require_8bit_frame

        require_8bit_frame("draw_overlay", self.source_frame)
        target = self.source_frame if self.source_frame is not None else self.original_image
        if target is None:
            raise ValueError("draw_overlay: the result has neither a source_frame nor an original_image to draw into")
        drawn = draw_heads(target, self.heads, out=out, **plan_kw)
        if to_host:
            return tuple(p.cpu().numpy() for p in drawn.planes) if self.source_frame is not None else drawn.cpu().numpy()
        return drawn

    def save_meshes(self, save_folder: str):
        """One Wavefront OBJ per head, 'v x y z' / 'f a b c' with 1-based faces (detection_result.py:22-35,73-78)."""
        if self._faces is None:
            raise ValueError("no triangle list available (FLAME model without faces)")
        os.makedirs(save_folder, exist_ok=True)
        tri = np.asarray(self._faces).astype(np.int64) + 1
        for i, head in enumerate(self.heads):
            with open(os.path.join(save_folder, f"head_{i}.obj"), "w") as f:
                for v in head.vertices_3d:
                    f.write("v %.8f %.8f %.8f\n" % tuple(v))
                for t in tri:
                    f.write("f %d %d %d\n" % tuple(t))

    def __repr__(self):
        shape = (self.source_frame if self.original_image is None else self.original_image).shape
        return f"PredictionResult(original_image={shape}, num heads={len(self.heads)})"
