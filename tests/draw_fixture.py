"""Helpers shared by the draw tests: the fixture recorded from the reference's own PredictionResult.draw (tests/golden/draw_heads.npz, written by
tests/golden/make_golden_draw.py), heads as the planner reads them, and the CPU picture of a plan (tests/draw_ref.py driven by draw.py's plan)."""
import os
import types

import numpy as np

import draw_ref
from aligned_fixture import formula_image
from head_detector_amd import draw
from head_detector_amd.head_info import Bbox

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ("full", "bbox", "landmarks", "points")


def load_fixture():
    return np.load(os.path.join(GOLDEN, "draw_heads.npz"))


def fixture_image(g, letter):
    return formula_image(*(int(v) for v in g[f"shape_{letter}"]))


def fixture_heads(g, letter):
    return [make_head(v, b) for v, b in zip(g[f"vertices_{letter}"], g[f"bbox_{letter}"])]


def fixture_result(g, letter, method):
    """The image the reference returned (recorded as result XOR original)."""
    return fixture_image(g, letter) ^ g[f"delta_{letter}_{method}"]


def fixture_assets(g):
    return dict(triangles=g["triangles"], head_indices=g["head_indices"], face_indices=g["face_indices"])


def make_head(vertices, bbox):
    return types.SimpleNamespace(vertices_3d=np.array(vertices, dtype=np.float32), bbox=Bbox(*(int(v) for v in bbox)))


def render_plan(image, plan, **kw):
    """tests/draw_ref.py driven by the product's own plan: what the GPU must produce."""
    return draw_ref.render(image, plan.points, plan.boxes, plan.triangles, plan.indices, plan.radius, **kw)


def expected(image, heads, method, **assets):
    return render_plan(image, draw.draw_plan(image.shape, heads, method, **assets))
