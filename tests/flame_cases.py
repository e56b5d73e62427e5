"""Planted inputs of the FLAME decode tests (no GPU, no library): a table of heads with one named property each, a different un-pad row per
head, small FLAME-shaped models that reach the kernel paths the 5023 / 400 / 5 model never enters, and the float64 references -- all of them from
oracle/flame_oracle.py.  tests/test_flame_cases_host.py checks from the oracle alone that every case is what its name says;
tests/test_gpu_flame_cases.py feeds them to csrc/flame.hip.

Parameter layout (FlameParams.from_3dmm's read order): [shape 300 | expression 100 | jaw 3 | rot6 | translation 3 | scale 1]."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import flame_oracle as fo

JAW, ROT6, TRANS, SCALE = slice(400, 403), slice(403, 409), slice(409, 412), 412
LIVE = (128, 64)  # live shape / expression coefficients of the planted table

# the project's own bars (tests/test_gpu_parity.py)
TOL_VERTS = 2e-6       # detector-mode vertices and R
TOL_PROJ_REL = 1e-6    # projected: TOL_PROJ_REL * max(1000, max |q64| of THIS head)
TOL_LBS = 5e-6         # general-pose lbs vertices; joints get the same
TOL_REBUILD = 1e-5     # |from_euler(device angles) - device R^T| on matrix entries (the fp32 formula's own distance on the CPU is ~1.5e-7)
TOL_RPY_DEG = 1e-3     # circular distance to scipy, where the angles are well conditioned

# Per-case bars that are NOT the project's: twice the distance of the float32 ORACLE from the float64 oracle, measured on the CPU by
# tests/test_flame_cases_host.py::test_f32_oracle_is_within_half_of_every_tolerance (never from a device result).  {case: {"verts" | "R" | "proj_rel": bar}}.
# Empty: every planted case and every small model stays within half of the project's bars (largest measured fractions of a bar, fp32 oracle vs
# fp64 oracle, as that test prints them: vertices 0.048, R 0.052, projected 0.216, small-model lbs vertices and joints 0.010).
MEASURED_TOL: Dict[str, Dict[str, float]] = {}


def tol(case: str, what: str) -> float:
    base = {"verts": TOL_VERTS, "R": TOL_VERTS, "proj_rel": TOL_PROJ_REL}[what]
    return MEASURED_TOL.get(case, {}).get(what, base)


# --------------------------------------------------------------------------------------------------------------
# planted head table
# --------------------------------------------------------------------------------------------------------------
def _snap(m: np.ndarray) -> np.ndarray:
    """cos(90 deg) is 6e-17 in float64, not 0: entries that are 0 or +-1 up to double rounding become exactly that ("yaw EXACTLY 90")."""
    m = m.copy()
    m[np.abs(m) < 1e-15] = 0.0
    for s in (1.0, -1.0):
        m[np.abs(m - s) < 1e-15] = s
    return m


def rot6_of_euler(a_deg: float, b_deg: float, c_deg: float) -> np.ndarray:
    """rot6 = (column 1, column 2) of R, where R^T = Rotation.from_euler("xyz", [a, b, c]) is what calculate_rpy hands to scipy:
    pitch = a - 180, yaw = b, roll = c."""
    from scipy.spatial.transform import Rotation

    Rt = _snap(Rotation.from_euler("xyz", [a_deg, b_deg, c_deg], degrees=True).as_matrix())
    R = Rt.T
    return np.concatenate([R[:, 0], R[:, 1]])


# (name, rot6 as float64) -- angles are (x, y, z) of the extrinsic "xyz" sequence
def _rot_cases() -> List[Tuple[str, np.ndarray]]:
    par = np.array([0.5, 0.5, 0.5])
    return [
        ("rot_identity", rot6_of_euler(0, 0, 0)),
        ("lock_yaw_p90", rot6_of_euler(0, 90, 0)),
        ("lock_yaw_m90", rot6_of_euler(0, -90, 0)),
        ("lock_yaw_p90_roll_pitch", rot6_of_euler(30, 90, -50)),
        ("lock_yaw_m90_roll_pitch", rot6_of_euler(-40, -90, 25)),
        ("near_lock_yaw_89.99", rot6_of_euler(20, 89.99, -35)),
        ("near_lock_yaw_89.9999", rot6_of_euler(20, 89.9999, -35)),
        ("rotx_180", rot6_of_euler(180, 0, 0)),
        ("rotx_p179.9999", rot6_of_euler(179.9999, 0, 0)),
        ("rotx_m179.9999", rot6_of_euler(-179.9999, 0, 0)),
        ("wrap_rotx_p1e-4", rot6_of_euler(1e-4, 0, 0)),
        ("wrap_rotx_m1e-4", rot6_of_euler(-1e-4, 0, 0)),
        ("rotz_180", rot6_of_euler(0, 0, 180)),
        ("rotz_m179.9999", rot6_of_euler(0, 0, -179.9999)),
        ("degenerate_first_zero", np.array([0.0, 0.0, 0.0, 0.3, -0.8, 0.5])),                 # b1 = 0 -> b3 = b2 = 0
        ("degenerate_second_parallel", np.concatenate([par, 2.0 * par])),                      # b1 x vy = 0 -> b3 = b2 = 0
        ("degenerate_first_tiny", np.concatenate([1e-20 * np.array([0.6, 0.0, 0.8]), [0.0, 1.0, 0.0]])),  # |vx| below F.normalize's eps: b1 = vx / 1e-12
        ("rot_generic", rot6_of_euler(17.0, -33.0, 71.0) * 1.7),
    ]


LOCK_CASES = ("lock_yaw_p90", "lock_yaw_m90", "lock_yaw_p90_roll_pitch", "lock_yaw_m90_roll_pitch")
WRAP_CASES = ("wrap_rotx_p1e-4", "wrap_rotx_m1e-4")
ZERO_COLUMN_CASES = {"degenerate_first_zero": (0, 1, 2), "degenerate_second_parallel": (1, 2)}  # columns of R that are exactly zero
DEGENERATE_CASES = ("degenerate_first_zero", "degenerate_second_parallel", "degenerate_first_tiny")  # R is no rotation: roll / pitch / yaw undefined
CLAMP_CASES = ("scale_0", "scale_m3", "scale_1e-9", "scale_1e-8")

_SCALE_CASES = [("scale_0", 0.0), ("scale_m3", -3.0), ("scale_1e-9", 1e-9), ("scale_1e-8", 1e-8), ("scale_1e4", 1e4)]
_JAW_DIR = np.array([2.0, -1.0, 2.0]) / 3.0
_JAW_CASES = [
    ("jaw_zero", np.zeros(3)),
    ("jaw_1e-7_one_axis", np.array([0.0, 1e-7, 0.0])),
    ("jaw_pi", np.pi * _JAW_DIR),
    ("jaw_2pi", 2.0 * np.pi * _JAW_DIR),
    ("jaw_10", 10.0 * _JAW_DIR),
]

_PLANTED = None


def planted_heads() -> Tuple[torch.Tensor, List[str]]:
    """([n, 413] float32, case names): one named property per head; everything a case does not plant is fo.synthetic_params (live 128 / 64)."""
    global _PLANTED
    if _PLANTED is None:
        rot = _rot_cases()
        names = [n for n, _ in rot] + [n for n, _ in _SCALE_CASES] + [n for n, _ in _JAW_CASES] + ["betas_zero"]
        p = fo.synthetic_params(len(names), seed=41, live_shape=LIVE[0], live_expr=LIVE[1], dtype=torch.float64)
        for i, (_, r6) in enumerate(rot):
            p[i, ROT6] = torch.from_numpy(r6)
        for i, (_, s) in enumerate(_SCALE_CASES, start=len(rot)):
            p[i, SCALE] = s
        for i, (_, j) in enumerate(_JAW_CASES, start=len(rot) + len(_SCALE_CASES)):
            p[i, JAW] = torch.from_numpy(j)
        p[len(names) - 1, :400] = 0.0
        _PLANTED = (p.to(torch.float32), names)
    return _PLANTED[0].clone(), list(_PLANTED[1])


def distinct_unpad(n: int, seed: int = 5) -> torch.Tensor:
    """[n, 3] (pad_x, pad_y, scale_factor), a different row for every head: pads in [0, 140], scale in [0.3, 2.5]."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, generator=g, dtype=torch.float64)
    u[:, :2] *= 140.0
    u[:, 2] = 0.3 + 2.2 * u[:, 2]
    u = u.to(torch.float32)
    assert len({tuple(r) for r in u.tolist()}) == n
    return u


def unpad_ref(proj64: torch.Tensor, unpad: torch.Tensor) -> torch.Tensor:
    """detector.py:67-69 per head, in proj64's precision: (x - pad_x, y - pad_y, z) / scale_factor with head h's OWN row unpad[h]."""
    u = unpad.to(proj64.dtype)
    q = proj64.clone()
    q[:, :, 0] -= u[:, None, 0]
    q[:, :, 1] -= u[:, None, 1]
    return q / u[:, None, 2:3]


def reference(model, params: torch.Tensor, unpad: Optional[torch.Tensor], dtype=torch.float64):
    """(vertices, R, projected [un-padded with each head's own row]) of fo.reproject in `dtype`."""
    c = fo.FlameConstants(model, dtype)
    v, R, q = fo.reproject(c, params.to(dtype))
    return v, R, (unpad_ref(q, unpad) if unpad is not None else q)


def proper_rotation(R32: torch.Tensor) -> torch.Tensor:
    """[n] bool: R is a rotation (the fp32 oracle's R R^T is the identity to 1e-5); false for the degenerate rot6 rows."""
    R = R32.double()
    return ((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().amax(dim=(1, 2)) < 1e-5)


# --------------------------------------------------------------------------------------------------------------
# roll / pitch / yaw: the closed form csrc/flame.hip evaluates, restated in fp32 numpy
# --------------------------------------------------------------------------------------------------------------
def _limit_angle_f32(g: np.float32) -> np.float32:
    f = np.float32
    if g < f(-180.0):
        q = int(g / f(180.0))
        fl = q // 2
        g = f(g + f(-2.0) * f(fl) * f(180.0))
    if g > f(180.0):
        g = f(g - f(2.0) * f((int(g / f(180.0)) + 1) // 2) * f(180.0))
    return g


def closed_form_rpy_f32(R: np.ndarray, lock_sign_inverted: bool = False) -> Tuple[np.ndarray, float]:
    """((roll, pitch, yaw) degrees, cb) of one fp32 R [3,3] by the kernel's formula: M = R^T = Rz(c) Ry(b) Rx(a); b = atan2(-M20, cb),
    cb = |(M00, M10)|; cb > 1e-6: a = atan2(M21, M22), c = atan2(M10, M00); else c = 0 and a = atan2(+-M01, M11).
    `lock_sign_inverted` is the mutation the tests must catch (the `m20 < 0` test turned round)."""
    f = np.float32
    R = np.asarray(R, dtype=np.float32)
    m00, m10, m20, m21, m22, m01, m11 = R[0, 0], R[0, 1], R[0, 2], R[1, 2], R[2, 2], R[1, 0], R[1, 1]
    RAD = f(57.29577951308232)
    cb = np.sqrt(f(m00 * m00) + f(m10 * m10), dtype=np.float32)
    eb = np.arctan2(-m20, cb, dtype=np.float32)
    if cb > f(1e-6):
        ea, ec = np.arctan2(m21, m22, dtype=np.float32), np.arctan2(m10, m00, dtype=np.float32)
    else:
        ec = f(0.0)
        neg = (m20 < 0) != lock_sign_inverted
        ea = np.arctan2(m01, m11, dtype=np.float32) if neg else np.arctan2(-m01, m11, dtype=np.float32)
    ang = [f(ec * RAD), f(f(ea * RAD) - f(180.0)), f(eb * RAD)]
    return np.array([_limit_angle_f32(g) for g in ang], dtype=np.float32), float(cb)


def rebuild_from_rpy(rpy: np.ndarray) -> np.ndarray:
    """R^T [3,3] float64 from (roll, pitch, yaw): Rotation.from_euler("xyz", [pitch + 180, yaw, roll]) -- calculate_rpy backwards."""
    from scipy.spatial.transform import Rotation

    r, p, y = (float(v) for v in rpy)
    return Rotation.from_euler("xyz", [p + 180.0, y, r], degrees=True).as_matrix()


def circ_dist_deg(a, b) -> np.ndarray:
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


# --------------------------------------------------------------------------------------------------------------
# small models
# --------------------------------------------------------------------------------------------------------------
def small_flame_model(V: int, NB: int, NJ: int, parents: List[int], seed: int) -> Dict[str, np.ndarray]:
    """fo.synthetic_flame_model's statistics at any (V, NB, NJ, tree): shapedirs / posedirs ~ N(0, 1e-3) (shapedirs with the decaying spectrum),
    J_regressor rows sparse (support min(64, V)), non-negative, summing to 1; skinning weights = softmax rows.  A function of its own, so the
    default model's draws -- and every golden file made from them -- stay as they are."""
    assert len(parents) == NJ and parents[0] == -1 and all(0 <= parents[j] < j for j in range(1, NJ))
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(V, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v_template = u * np.array([0.10, 0.16, 0.11]) + np.array([0.0, -0.03, -0.04])
    shapedirs = rng.normal(0, 1e-3, size=(V, 3, NB)) * (1.0 / np.sqrt(1.0 + np.arange(NB) / 10.0))[None, None, :]
    posedirs = rng.normal(0, 1e-3, size=(V, 3, (NJ - 1) * 9))
    sup = min(64, V)
    J_regressor = np.zeros((NJ, V))
    for j in range(NJ):
        idx = rng.choice(V, size=sup, replace=False)
        w = rng.random(sup)
        J_regressor[j, idx] = w / w.sum()
    logits = rng.normal(0, 2.0, size=(V, NJ))
    weights = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    kintree = np.array([[4294967295] + [int(p) for p in parents[1:]], list(range(NJ))], dtype=np.int64)
    return {"v_template": v_template, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": J_regressor, "kintree_table": kintree, "weights": weights,
            "f": rng.integers(0, V, size=(2 * V, 3))}


def _chain(nj: int) -> List[int]:
    return [-1] + list(range(nj - 1))


# name -> (V, NB, NJ, parents, seed): what each one exercises is in the table of test_gpu_flame_cases.py::test_model_shapes
SMALL_MODELS = {
    "A": (70, 8, 5, [-1, 0, 1, 1, 1], 11),          # component-split (c3) tiles with K = 44
    "B": (33, 10, 3, _chain(3), 12),                # NB % 8 != 0: no c3 tiles, the register-fed matrix-core kernel
    "C": (31, 13, 8, [-1, 0, 1, 2, 0, 4, 4, 6], 13),  # odd K: VALU only; 8 joints: jbase up to 21
    "D": (5, 1, 1, [-1], 14),                       # NP = 0, V below one 32-vertex group, NB < 64 and odd
    "E": (40, 8, 1, [-1], 15),                      # NP = 0 with the c3 conditions met (K == NB: an empty pose-feature run)
    "F": (64, 72, 7, _chain(7), 16),                # 54 pose features, two lane passes over NB, a chain-shaped tree
    "G": (40, 456, 5, [-1, 0, 1, 1, 1], 17),        # second chunk of the WIDE prologue (448 coefficients per pass)
}
MODEL_NS = (1, 3, 5, 9, 33, 130)

_MODELS: Dict[str, Dict[str, np.ndarray]] = {}
_LBS_REF: Dict[tuple, tuple] = {}


def small_model(name: str) -> Dict[str, np.ndarray]:
    if name not in _MODELS:
        V, NB, NJ, parents, seed = SMALL_MODELS[name]
        _MODELS[name] = small_flame_model(V, NB, NJ, parents, seed)
    return _MODELS[name]


def model_constants(model: Dict[str, np.ndarray], dtype=torch.float64) -> fo.FlameConstants:
    """fo.FlameConstants, also for a single-joint model (its posedirs [V, 3, 0] has no pose feature to reshape by)."""
    if model["posedirs"].shape[-1] > 0:
        return fo.FlameConstants(model, dtype)
    c = fo.FlameConstants.__new__(fo.FlameConstants)
    c.dtype = dtype
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
    c.v_template, c.shapedirs, c.J_regressor, c.lbs_weights = t(model["v_template"]), t(model["shapedirs"]), t(model["J_regressor"]), t(model["weights"])
    c.posedirs = torch.zeros(0, 3 * model["v_template"].shape[0], dtype=dtype)
    c.parents = torch.tensor([-1], dtype=torch.int64)
    c.faces = np.asarray(model["f"]).astype(np.int64)
    return c


def lbs_inputs(NB: int, NJ: int, n: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(betas [n, NB], pose [n, 3 NJ]) float32 = randn * 0.3."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, NB, generator=g) * 0.3, torch.randn(n, 3 * NJ, generator=g) * 0.3


def lbs_reference(c: fo.FlameConstants, betas: torch.Tensor, pose: torch.Tensor, dtype=torch.float64):
    """(vertices [n, V, 3], posed joints [n, NJ, 3]) of fo.lbs in `dtype`."""
    c = c.to(dtype)
    n = betas.shape[0]
    return fo.lbs(betas.to(dtype), pose.to(dtype), c.v_template.unsqueeze(0).repeat(n, 1, 1), c.shapedirs, c.posedirs, c.J_regressor, c.parents, c.lbs_weights)


def small_model_case(name: str, n: int):
    """(betas, pose, vertices64, joints64) of small model `name` at n heads; computed once."""
    if (name, n) not in _LBS_REF:
        V, NB, NJ, _, seed = SMALL_MODELS[name]
        betas, pose = lbs_inputs(NB, NJ, n, 1000 * seed + n)
        v64, j64 = lbs_reference(model_constants(small_model(name)), betas, pose)
        _LBS_REF[(name, n)] = (betas, pose, v64, j64)
    return _LBS_REF[(name, n)]
