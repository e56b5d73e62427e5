"""Planted cases for head tensors (include/vgh_crop.h) at the smallest shapes where the kernel can still go wrong, and what the restatement
(tests/head_tensors_ref.py) makes of each.  A case is a list of (source, heads) pairs -- one pair runs through ``head_tensors``, several through ONE
``head_tensors_batch`` call -- with the crop size, the supersampling factor, the geometry mode and the normalisation.  RGB sources are pitched views of a wider
buffer (sentinel bytes between width and pitch); YUV sources are decoder surfaces of tests/yuv_ref.py with random bytes wherever no sample lies.

The restatement is driven by the coefficients of ``head_tensor_plan`` (tests/test_head_tensors_host.py pins those against hand-computed values and against the
ramp check), so what the GPU tests pin is the pixels."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_tensors_ref as ref  # noqa: E402
import yuv_ref  # noqa: E402

from head_detector_amd import head_tensors as ht  # noqa: E402
from head_detector_amd.head_info import RPY, Bbox  # noqa: E402
from head_detector_amd.video import YUV420Frame, yuv_coefficients  # noqa: E402

H, W, EXTRA, LEFT = 97, 131, 19, 7
HIDX = np.arange(0, 300, 3)
DTYPES = {"uint8": torch.uint8, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DEFAULT_NORM = dict(scale=1 / 255, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
OTHER_NORM = dict(scale=1.0, mean=(127.5, 100.0, 3.25), std=(128.0, 57.0, 0.7))


# ---- sources ------------------------------------------------------------------------------------------------------------------------------------------
def rgb_source(h=H, w=W, kind="random", seed=0):
    """A pitched uint8 image: columns LEFT .. LEFT + w of a buffer [h, w + EXTRA, 3]."""
    if kind == "random":
        buffer = np.random.default_rng(seed).integers(0, 256, (h, w + EXTRA, 3), dtype=np.uint8)
    elif kind == "white":  # the image is all 255, the bytes around it are not
        buffer = np.random.default_rng(seed).integers(0, 200, (h, w + EXTRA, 3), dtype=np.uint8)
        buffer[:, LEFT:LEFT + w] = 255
    else:
        raise KeyError(kind)
    return dict(kind="rgb", buffer=buffer, width=w)


def yuv_source(layout, h, w, *, full_range=False, matrix="bt709", saturating=False, pad=6, extra_rows=1, seed=0):
    y, u, v = yuv_ref.picture(h, w, seed, saturating)
    buffer, pitch, uv_offset = yuv_ref.surface(layout, y, u, v, pitch=2 * ((w + 1) // 2) + pad, extra_rows=extra_rows, seed=seed + 1)
    return dict(kind="yuv", layout=layout, y=y, u=u, v=v, buffer=buffer, pitch=pitch, uv_offset=uv_offset, height=h, width=w, matrix=matrix, full_range=full_range)


def rgb_of(source) -> np.ndarray:
    """The uint8 [h, w, 3] image the rule reads (a frame: every pixel converted and clamped first)."""
    if source["kind"] == "rgb":
        return np.ascontiguousarray(source["buffer"][:, LEFT:LEFT + source["width"]])
    return yuv_ref.yuv_to_rgb(source["y"], source["u"], source["v"], yuv_coefficients(source["matrix"], source["full_range"]))


def on_device(source, device):
    """-> (what ``head_tensors`` takes: a pitched GPU view or a YUV420Frame on a surface, the whole GPU buffer behind it)."""
    buffer = torch.from_numpy(source["buffer"]).to(device)
    if source["kind"] == "rgb":
        return buffer[:, LEFT:LEFT + source["width"]], buffer
    make = {"nv12": YUV420Frame.from_nv12, "nv21": YUV420Frame.from_nv21, "i420": YUV420Frame.from_i420}[source["layout"]]
    return make(buffer, source["height"], source["width"], pitch=source["pitch"], uv_offset=source["uv_offset"], matrix=source["matrix"], full_range=source["full_range"]), buffer


# ---- heads --------------------------------------------------------------------------------------------------------------------------------------------
def box_head(bbox):
    return types.SimpleNamespace(bbox=Bbox(*(int(v) for v in bbox)))


def mesh_head(cx, cy, r, roll, h=H, w=W, yaw=10.0, seed=0):
    """A head for ``aligned=True``: 300 vertices in a disc, the skull centre at (cx, cy), rotated by ``roll`` when ``abs(yaw) < 60``."""
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, 300), np.sqrt(rng.uniform(0, 1, 300))
    v = np.stack([cx + r * rad * np.cos(ang), cy + r * rad * np.sin(ang), rng.normal(0, 5, 300)], axis=1).astype(np.float32)
    s = 640 / max(h, w)
    t = torch.tensor([[cx * s + (640 - int(w * s)), cy * s + (640 - int(h * s)), 0.0]], dtype=torch.float32)
    return types.SimpleNamespace(vertices_3d=v, flame_params=types.SimpleNamespace(translation=t), head_pose=RPY(roll=float(roll), pitch=0.0, yaw=float(yaw)),
                                 bbox=Bbox(int(cx - r), int(cy - r), int(2 * r), int(2 * r)))


def case(pairs, size, supersample="auto", aligned=False, margin=0.1, fill=(7, 100, 250), norm=None):
    return dict(pairs=pairs, size=size, supersample=supersample, aligned=aligned, margin=margin, fill=fill, norm=norm or DEFAULT_NORM)


def _many(n, seed):
    rng = np.random.default_rng(seed)
    return [box_head((rng.integers(-10, 60), rng.integers(-10, 60), rng.integers(0, 40), rng.integers(0, 40))) for _ in range(n)]


def cases():
    big = rgb_source()
    c = {}
    # an upright head at scale 1 on integer coordinates: the crop is the source slice
    c["upright_identity"] = case([(big, [box_head((10, 20, 33, 33))])], 33, 1, margin=0.0)
    c["S17_K2_ragged"] = case([(big, [box_head((5, 9, 60, 41)), box_head((70, 30, 35, 50))])], 17, 2)
    c["S7_K3"] = case([(big, [box_head((40, 10, 50, 64)), box_head((0, 0, 20, 21))])], 7, 3, norm=OTHER_NORM)
    c["S1_K8"] = case([(big, [box_head((30, 30, 40, 40)), box_head((100, 70, 10, 9))])], 1, 8)
    c["S16_auto"] = case([(big, [box_head((3, 4, 90, 80)), box_head((60, 50, 16, 13)), box_head((20, 20, 40, 33))])], 16)  # K = 7, 2 and 3
    c["S33_K8"] = case([(rgb_source(64, 64, seed=3), [box_head((2, 3, 50, 55))])], 33, 8)
    # rolls, through the geometry of get_aligned_heads (an un-rotated profile head among them)
    c["roll_30"] = case([(big, [mesh_head(60.0, 50.0, 25.0, 30.0, seed=1)])], 17, aligned=True)
    c["roll_minus_170"] = case([(big, [mesh_head(70.0, 40.0, 30.0, -170.0, seed=2), mesh_head(40.0, 60.0, 12.0, 77.0, yaw=75.0, seed=3)])], 16, 2, aligned=True, norm=OTHER_NORM)
    # heads that leave the image: fill where there is no image, one tensor per head
    c["half_outside"] = case([(big, [box_head((-20, 30, 40, 40)), box_head((110, -15, 40, 30)), box_head((50, 80, 30, 36))])], 16)
    c["wholly_outside"] = case([(big, [box_head((200, 10, 20, 20)), box_head((-60, -60, 30, 30))])], 7, 2)
    c["far_away"] = case([(big, [box_head((40000, 40000, 30, 30)), box_head((-40000, 5, 64, 64)), box_head((10, 10, 30, 30))])], 16)  # positions beyond int32
    c["side_0"] = case([(big, [box_head((50, 40, 0, 0)), box_head((13, 17, 0, 0))])], 7, margin=0.0)
    c["many_heads"] = case([(rgb_source(64, 64, seed=5), _many(300, 6))], 7)
    c["no_heads"] = case([(big, [])], 16)
    c["image_2x3"] = case([(rgb_source(2, 3, seed=7), [box_head((0, 0, 3, 2)), box_head((-2, -2, 8, 8))])], 7, 2)
    c["image_1x1"] = case([(rgb_source(1, 1, seed=8), [box_head((0, 0, 1, 1)), box_head((-3, -3, 7, 7))])], 17, 3)
    # video frames of odd sizes, in their own planes
    c["nv12_limited"] = case([(yuv_source("nv12", 37, 51, seed=10), [box_head((5, 4, 30, 28)), box_head((-8, 20, 30, 30))])], 16, 2)
    c["nv21_full"] = case([(yuv_source("nv21", 51, 37, full_range=True, matrix="bt601", seed=11), [box_head((2, 9, 33, 40)), box_head((20, 30, 30, 30))])], 17)
    c["i420_limited"] = case([(yuv_source("i420", 33, 35, matrix="bt2020", seed=12), [box_head((0, 0, 35, 33)), box_head((30, 28, 9, 9))])], 7, 3)
    c["i420_full_saturating"] = case([(yuv_source("i420", 21, 19, full_range=True, saturating=True, seed=13), [box_head((-2, -2, 24, 24))])], 33, 1)
    c["nv12_saturating"] = case([(yuv_source("nv12", 35, 33, saturating=True, seed=14), [box_head((1, 1, 30, 30))])], 16, 8, norm=OTHER_NORM)
    # every sum at its bound: K = 8 on an all-255 image, every tap inside
    c["sum_at_its_bound"] = case([(rgb_source(64, 64, "white", seed=15), [box_head((8, 8, 48, 48))])], 16, 8, margin=0.0)
    # two sources of different sizes and kinds in ONE call (and a result without heads between them)
    c["two_sources"] = case([(big, [box_head((10, 10, 50, 50)), box_head((100, 60, 40, 40))]), (rgb_source(2, 3, seed=16), []),
                             (yuv_source("nv12", 37, 51, seed=17), [box_head((0, 0, 37, 37))]), (rgb_source(64, 64, seed=18), [box_head((30, 30, 40, 40))])], 17)
    return c


# ---- what the restatement makes of a case ---------------------------------------------------------------------------------------------------------------
def plan_of(c):
    """(coefficients [n, 6], supersample [n], source index [n], matrices [n, 2, 3]) of the whole case, from ``head_tensor_plan`` per pair."""
    plans = [ht.head_tensor_plan(rgb_of(source).shape, heads, c["size"], aligned=c["aligned"], margin=c["margin"], supersample=c["supersample"],
                                 head_indices=HIDX if c["aligned"] else None) for source, heads in c["pairs"]]
    index = np.concatenate([np.full(len(p), k, np.int64) for k, p in enumerate(plans)])
    return np.concatenate([p.coefficients for p in plans]), np.concatenate([p.supersample for p in plans]), index, np.concatenate([p.matrices for p in plans])


def expected_sums(c, order="rgb"):
    coefficients, ks, index, _ = plan_of(c)
    return ref.sums([rgb_of(source) for source, _ in c["pairs"]], coefficients, ks, index, c["size"], c["fill"], order), ks


def run(c, device, dtype="float32", layout="nchw", order="rgb", out=None, sources=None):
    """The case through the public interface -> HeadTensors.  ``sources``: what ``on_device`` made of the pairs' sources, to look at their buffers afterwards."""
    sources = sources or [on_device(source, device)[0] for source, _ in c["pairs"]]
    kw = dict(aligned=c["aligned"], margin=c["margin"], supersample=c["supersample"], fill=c["fill"], dtype=DTYPES[dtype], layout=layout, channel_order=order,
              head_indices=HIDX if c["aligned"] else None, out=out, **c["norm"])
    if len(sources) == 1:
        return ht.head_tensors(sources[0], c["pairs"][0][1], c["size"], **kw)
    results = [types.SimpleNamespace(source_frame=s if isinstance(s, YUV420Frame) else None, original_image=None if isinstance(s, YUV420Frame) else s, heads=heads,
                                     head_indices=None) for s, (_, heads) in zip(sources, c["pairs"])]
    return ht.head_tensors_batch(results, c["size"], **kw)
