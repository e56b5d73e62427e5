"""Helpers shared by the aligned-head tests: the fixture recorded from the reference (tests/golden/aligned_heads.npz, written by
tests/golden/make_golden_aligned.py) and the integer formula of its images."""
import os
import types

import numpy as np
import torch

from head_detector_amd.head_info import RPY

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    return np.load(os.path.join(GOLDEN, "aligned_heads.npz"))


def formula_image(h: int, w: int) -> np.ndarray:
    """The images of the fixture: an integer formula of (x, y, c), the same as in tests/golden/make_golden_aligned.py."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((x * 7 + y * 13 + c * 71 + (x * y) % 251 + ((x >> 3) ^ (y >> 3)) * 5) & 255).astype(np.uint8)


def fixture_heads(g, which=None):
    """-> [(index in the fixture, image letter, head)]: heads as SimpleNamespaces with the attributes the planner reads."""
    out = []
    for i in range(len(g["names"])):
        if which is not None and str(g["image"][i]) != which:
            continue
        fp = types.SimpleNamespace(translation=torch.from_numpy(g["translation"][i : i + 1].copy()))
        out.append((i, str(g["image"][i]), types.SimpleNamespace(vertices_3d=g["vertices"][i].copy(), flame_params=fp,
                                                                  head_pose=RPY(roll=float(g["roll"][i]), pitch=0.0, yaw=float(g["yaw"][i])))))
    return out


def fixture_crops(g):
    sizes = [int(np.prod(s)) for s in g["crop_shape"]]
    at = np.concatenate([[0], np.cumsum(sizes)])
    assert at[-1] == g["crop_bytes"].size
    return [g["crop_bytes"][at[i] : at[i + 1]].reshape(tuple(g["crop_shape"][i])) for i in range(len(sizes))]
