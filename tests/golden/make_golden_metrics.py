"""Records tests/golden/mesh_metrics.npz by RUNNING THE REFERENCE's own yolo_head_training/evaluation/dad_utils.py (only the absent ``smplx`` leaf is
substituted; none of the recorded functions touches it): ``calc_zn``, ``procrustes``, ``align_pred_to_gt``, ``mesh_points_by_barycentric_coordinates``,
``get_7_landmarks_from_68``, and the two rotation metrics of evaluate_dad.py:256-266 through scipy's ``Rotation``.  Outputs and seeds only: the inputs are
regenerated from the seeds by tests/mesh_metrics_ref.py (the template comes from tests/golden/flame_decode.npz); the one list no other fixture holds in
full, the reference's head_indices, is stored here.  Run from the repository root:  python tests/golden/make_golden_metrics.py

Z_n.  The reference ranks float32 ``torch.cdist`` distances; the device ranks float64 ones.  For every recorded case the generator ASSERTS that the
reference's own ``argsort(cdist)`` equals the float64 (distance, index) order in the columns 1 .. 5 that ``calc_zn`` reads, and moves to the next seed if
it does not: only then is the recorded value a statement about the arithmetic-free part of the metric, which the device must meet exactly."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))

import mesh_metrics_ref as mr  # noqa: E402


def load_dad_utils():
    smplx = types.ModuleType("smplx")  # absent here; dad_utils needs it for the landmark embedding files only
    utils = types.ModuleType("smplx.utils")
    utils.Struct = type("Struct", (), {})
    lbs = types.ModuleType("smplx.lbs")
    lbs.find_dynamic_lmk_idx_and_bcoords = None
    sys.modules.update({"smplx": smplx, "smplx.utils": utils, "smplx.lbs": lbs})
    spec = importlib.util.spec_from_file_location("dad_utils", os.path.join(REF, "yolo_head_training", "evaluation", "dad_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def orders_agree(gt, top_k=5):
    """The reference's float32 argsort(cdist) against the float64 (distance, index) order, in the columns calc_zn reads."""
    g = torch.from_numpy(gt)
    ref = torch.argsort(torch.cdist(g, g), dim=0)[:, 1:top_k + 1].numpy()
    return np.array_equal(ref, mr.column_order(gt, np.arange(1, top_k + 1)))


def main():
    du = load_dad_utils()
    from scipy.spatial.transform import Rotation

    v_template = np.load(os.path.join(HERE, "flame_decode.npz"))["v_template"]
    head_indices = np.load(os.path.join(REF, "head_detector", "assets", "flame_indices", "head_indices.npy")).astype(np.int64)
    assert head_indices.shape == (2470,) and head_indices.max() < 5023
    out = {"head_indices": head_indices.astype(np.int16)}

    seed = 100
    for name in mr.ZN_CASES:
        seeds = []
        while len(seeds) < (2 if name == "two_heads" else 1):
            seed += 1
            _, gt = mr.zn_inputs(name, [seed], v_template, head_indices)
            ok = orders_agree(gt[0])
            print(f"{name}: seed {seed}: float32 cdist order {'=' if ok else '!='} float64 order")
            if ok:
                seeds.append(seed)
        pred, gt = mr.zn_inputs(name, seeds, v_template, head_indices)
        value = float(du.calc_zn(torch.from_numpy(pred), torch.from_numpy(gt)))
        N = gt.shape[1]
        ratio, count = mr.z_order(pred, gt, 5, "reference")
        # result_tmp is float32 0/1 and its mean is taken per head in float32: the recorded value is the mean over heads of count / (N * 5) to ~1e-7
        assert abs(value - ratio.mean()) < 1e-6, (name, value, ratio)
        if len(seeds) == 1:
            assert round(value * N * 5) == count[0], (name, value, count)
        intended = mr.z_order(pred, gt, 5, "nearest")[0]
        print(f"{name}: N = {N}, calc_zn = {value:.6f}, restated reference {ratio.tolist()}, nearest {intended.tolist()}")
        assert not np.array_equal(ratio, intended), "the case does not tell the two readings apart"
        out[f"zn.{name}.seeds"] = np.array(seeds, dtype=np.int64)
        out[f"zn.{name}.value"] = np.float64(value)

    for k, (s, scaling, reflection) in enumerate(mr.PROCRUSTES_CASES):
        X, Y = mr.procrustes_inputs(s)
        d, Z, tform = du.procrustes(X.copy(), Y.copy(), scaling=scaling, reflection=reflection)
        out[f"procrustes.{k}.d"] = np.float64(d)
        out[f"procrustes.{k}.Z"] = np.asarray(Z, dtype=np.float64)
        out[f"procrustes.{k}.rotation"] = np.asarray(tform["rotation"], dtype=np.float64)
        out[f"procrustes.{k}.scale"] = np.float64(tform["scale"])
        out[f"procrustes.{k}.translation"] = np.asarray(tform["translation"], dtype=np.float64)
        print(f"procrustes {k}: scaling={scaling} reflection={reflection}: d = {d:.6f}, det = {np.linalg.det(tform['rotation']):+.3f}, scale = {tform['scale']:.4f}")

    pv, pl, gl = mr.align_inputs()
    out["align.vertices"] = du.align_pred_to_gt(torch.from_numpy(pv), pl.copy(), gl.copy()).numpy()  # float32: the source ends in torch.Tensor(...)

    vertices, faces, idx, b = mr.embedding_inputs()
    out["embedding.landmarks"] = np.stack([du.mesh_points_by_barycentric_coordinates(torch.from_numpy(v), torch.from_numpy(faces), torch.from_numpy(idx),
                                                                                     torch.from_numpy(b)).numpy() for v in vertices])
    out["seven_of_68"] = du.get_7_landmarks_from_68(torch.arange(68 * 3).reshape(68, 3))[:, 0] // 3

    Rp, Rg = mr.rotation_inputs()
    rot, ang = [], []
    for a, b_ in zip(Rp, Rg):
        R = a @ b_.T
        rot.append(np.linalg.norm(np.eye(3) - R, "fro"))
        deg = np.rad2deg(np.linalg.norm(Rotation.from_matrix(R).as_rotvec()))
        ang.append(min(abs(deg), abs(deg - 180.0), abs(deg + 180.0)))
    out["rotation.rot_error"], out["rotation.angle_error"] = np.array(rot), np.array(ang)
    print("angle errors:", np.round(ang, 4).tolist())

    np.savez_compressed(mr.GOLDEN, **out)
    print(mr.GOLDEN, os.path.getsize(mr.GOLDEN), "bytes")
    assert os.path.getsize(mr.GOLDEN) < 64 * 1024


if __name__ == "__main__":
    main()
