"""CPU: the planted FLAME cases (tests/flame_cases.py) are what their names say.  Every property is read from the ORACLE (oracle/flame_oracle.py, fp32 and
fp64), never from a kernel: this is the check of the inputs, of the references and of the tolerances that tests/test_gpu_flame_cases.py then holds
csrc/flame.hip to."""
import numpy as np
import pytest
import torch

import flame_cases as fc
from conftest import golden
from oracle import flame_oracle as fo


@pytest.fixture(scope="module")
def table():
    p, names = fc.planted_heads()
    R32 = fo.rot_mat_from_6dof(p[:, fc.ROT6])
    return p, names, R32


def _row(names, name):
    return names.index(name)


def test_table_has_one_row_per_case_and_keeps_the_header_contract(table):
    p, names, _ = table
    assert p.shape == (len(names), fo.NUM_PARAMS) and p.dtype == torch.float32 and len(set(names)) == len(names)
    for group in (fc.LOCK_CASES, fc.WRAP_CASES, fc.DEGENERATE_CASES, fc.CLAMP_CASES, tuple(fc.ZERO_COLUMN_CASES)):
        assert set(group) <= set(names)
    # coefficients beyond the live counts MUST be exactly zero (include/vgh.h)
    assert not p[:, fc.LIVE[0] : 300].any() and not p[:, 300 + fc.LIVE[1] : 400].any()
    assert not p[_row(names, "betas_zero"), :400].any() and torch.isfinite(p).all()
    q, _ = fc.planted_heads()
    assert torch.equal(p, q)


def test_lock_rows_are_exact_gimbal_lock_in_fp32(table):
    _, names, R32 = table
    for name in fc.LOCK_CASES:
        R = R32[_row(names, name)].numpy()
        assert abs(R.T[2, 0]) == np.float32(1.0), name                # |R^T[2,0]| == 1
        assert R[0, 0] == 0.0 and R[0, 1] == 0.0, name                # cb = |(M00, M10)| == 0 exactly
        assert np.sign(R.T[2, 0]) == (-1.0 if "_p90" in name else 1.0), name  # M20 = -sin(yaw)
        rpy = fo.calculate_rpy(torch.from_numpy(fc._rot_cases()[_row(names, name)][1]).float())
        assert rpy[0] == 0.0 and abs(abs(rpy[2]) - 90.0) < 1e-4, (name, rpy)  # scipy: third angle (roll) 0 at lock
    for name, cb_max in (("near_lock_yaw_89.99", 2e-4), ("near_lock_yaw_89.9999", 2e-6)):
        R = R32[_row(names, name)].numpy()
        cb = float(np.hypot(R[0, 0], R[0, 1]))
        assert 1e-6 < cb < cb_max, (name, cb)  # beside the lock branch's threshold, not in it


def test_wrap_rows_sit_on_both_sides_of_the_pitch_wrap(table):
    p, names, _ = table
    pitch = [fo.calculate_rpy(p[_row(names, n), fc.ROT6])[1] for n in fc.WRAP_CASES]
    assert pitch[0] * pitch[1] < 0
    for v in pitch:
        assert abs(abs(v) - 180.0) < 1e-3 and abs(v) <= 180.0
    near0 = [fo.calculate_rpy(p[_row(names, n), fc.ROT6])[1] for n in ("rotx_p179.9999", "rotx_m179.9999")]
    assert near0[0] * near0[1] < 0 and max(abs(v) for v in near0) < 1e-3


def test_degenerate_rot6_rows_give_exact_zero_columns(table):
    _, names, R32 = table
    for name, cols in fc.ZERO_COLUMN_CASES.items():
        R = R32[_row(names, name)]
        for c in range(3):
            assert bool((R[:, c] == 0).all()) == (c in cols), (name, c)
    tiny = R32[_row(names, "degenerate_first_tiny")]
    assert 0 < float(tiny[:, 0].norm()) < 1e-7 and abs(float(tiny[:, 2].norm()) - 1.0) < 1e-6  # b1 = vx / eps, b3 a unit vector
    proper = fc.proper_rotation(R32)
    assert [n for n, ok in zip(names, proper.tolist()) if not ok] == list(fc.DEGENERATE_CASES)


def test_clamp_rows_clamp_and_the_large_scale_does_not(table):
    p, names, _ = table
    for name in fc.CLAMP_CASES:
        s = p[_row(names, name), fc.SCALE]
        assert float(torch.clamp(s, 1e-8)) == float(torch.tensor(1e-8, dtype=torch.float32)), name
    assert float(p[_row(names, "scale_1e4"), fc.SCALE]) == 1e4
    jaw = p[:, fc.JAW].double().norm(dim=1)
    assert float(jaw[_row(names, "jaw_zero")]) == 0.0
    for name, want in (("jaw_1e-7_one_axis", 1e-7), ("jaw_pi", np.pi), ("jaw_2pi", 2 * np.pi), ("jaw_10", 10.0)):
        assert abs(float(jaw[_row(names, name)]) / want - 1.0) < 1e-6, name


def test_distinct_unpad_has_no_repeated_row():
    for n in (1, 11, 33, 64):
        u = fc.distinct_unpad(n)
        assert u.shape == (n, 3) and u.dtype == torch.float32 and len({tuple(r) for r in u.tolist()}) == n
        assert float(u[:, :2].min()) >= 0 and float(u[:, :2].max()) <= 140 and float(u[:, 2].min()) >= 0.3 and float(u[:, 2].max()) <= 2.5
    assert torch.equal(fc.distinct_unpad(11), fc.distinct_unpad(11))


def test_default_model_is_still_the_one_behind_the_golden_file(flame_model):
    """small_flame_model is a function of its own: fo.synthetic_flame_model's draws, and the vectors made from them, are untouched."""
    g = golden("flame_decode.npz")
    c32 = fo.FlameConstants(flame_model, torch.float32)
    v, R, q = fo.reproject(c32, torch.from_numpy(g["params"]))
    assert np.abs(v.numpy() - g["vertices"]).max() < 1e-5 and np.abs(R.numpy() - g["R"]).max() < 1e-5
    assert np.abs(q.numpy() - g["projected"]).max() < 1e-6 * max(1000.0, np.abs(g["projected"]).max())
    plain = fo.synthetic_flame_model(seed=int(g["seed"]), v_template=g["v_template"].astype(np.float64))
    for k in ("shapedirs", "posedirs", "J_regressor", "weights", "kintree_table", "f"):
        assert np.array_equal(plain[k], flame_model[k]), k
    rng = np.random.default_rng(int(g["seed"]))  # the first draw behind shapedirs, restated
    assert np.array_equal(plain["shapedirs"][:2, :, 0], rng.normal(0, 1e-3, size=(5023, 3, 400))[:2, :, 0])


def test_f32_oracle_is_within_half_of_every_tolerance(table, flame_model, capsys):
    """The reference CPU path in fp32 against the fp64 arbiter, per case with each head's own un-pad row: half of the bar the device is held to
    (or, for a case listed in fc.MEASURED_TOL, the bar is twice what is measured here)."""
    p, names, _ = table
    unpad = fc.distinct_unpad(len(names))
    v64, R64, q64 = fc.reference(flame_model, p, unpad, torch.float64)
    v32, R32, q32 = fc.reference(flame_model, p, unpad, torch.float32)
    worst = {"verts": 0.0, "R": 0.0, "proj_rel": 0.0}
    for h, name in enumerate(names):
        ev = float((v32[h].double() - v64[h]).abs().max())
        eR = float((R32[h].double() - R64[h]).abs().max())
        eq = float((q32[h].double() - q64[h]).abs().max()) / max(1000.0, float(q64[h].abs().max()))
        for what, e in (("verts", ev), ("R", eR), ("proj_rel", eq)):
            worst[what] = max(worst[what], e / fc.tol(name, what))
            assert e <= 0.5 * fc.tol(name, what), (name, what, e)
    with capsys.disabled():
        print(f"\n[flame cases] fp32 oracle / bar: {worst}")


@pytest.mark.parametrize("name", sorted(fc.SMALL_MODELS))
def test_small_models_have_the_shapes_of_the_table_and_a_quiet_f32_oracle(name, capsys):
    V, NB, NJ, parents, _ = fc.SMALL_MODELS[name]
    m = fc.small_model(name)
    assert m["v_template"].shape == (V, 3) and m["shapedirs"].shape == (V, 3, NB) and m["posedirs"].shape == (V, 3, 9 * (NJ - 1))
    assert m["J_regressor"].shape == (NJ, V) and m["weights"].shape == (V, NJ)
    assert ((m["J_regressor"] > 0).sum(1) == min(64, V)).all() and np.allclose(m["J_regressor"].sum(1), 1) and np.allclose(m["weights"].sum(1), 1)
    c = fc.model_constants(m)
    assert c.parents.tolist() == parents
    worst = 0.0
    for n in (5, 33):
        betas, pose, v64, j64 = fc.small_model_case(name, n)
        v32, j32 = fc.lbs_reference(c, betas, pose, torch.float32)
        ev, ej = float((v32.double() - v64).abs().max()), float((j32.double() - j64).abs().max())
        worst = max(worst, ev / fc.TOL_LBS, ej / fc.TOL_LBS)
        assert ev <= 0.5 * fc.TOL_LBS and ej <= 0.5 * fc.TOL_LBS, (name, n, ev, ej)
        assert v64.shape == (n, V, 3) and j64.shape == (n, NJ, 3)
    with capsys.disabled():
        print(f"\n[flame cases] model {name}: fp32 oracle / lbs bar {worst:.3f}")


def test_closed_form_rpy_in_fp32_meets_the_bars_the_device_is_held_to(table):
    """The kernel's roll / pitch / yaw formula, restated in fp32 numpy on the fp32 oracle's R: angles inside [-180, 180], the rotation rebuilt from them is
    R^T to fc.TOL_REBUILD, and where the angles are well conditioned (cb >= 1e-2) or the lock is exact (cb == 0) they are scipy's to fc.TOL_RPY_DEG.
    The same formula with the lock branch's sign test inverted must NOT pass: the rebuild check is what catches that mutation."""
    p, names, R32 = table
    proper = fc.proper_rotation(R32)
    worst_rebuild, worst_deg, mutant_caught = 0.0, 0.0, []
    for h, name in enumerate(names):
        if not proper[h]:
            continue
        R = R32[h].numpy()
        rpy, cb = fc.closed_form_rpy_f32(R)
        assert (np.abs(rpy) <= 180.0).all(), (name, rpy)
        err = float(np.abs(fc.rebuild_from_rpy(rpy) - R.T.astype(np.float64)).max())
        worst_rebuild = max(worst_rebuild, err)
        assert err < fc.TOL_REBUILD, (name, err)
        if cb >= 1e-2 or cb == 0.0:
            d = float(fc.circ_dist_deg(rpy, fo.calculate_rpy(p[h, fc.ROT6])).max())
            worst_deg = max(worst_deg, d)
            assert d < fc.TOL_RPY_DEG, (name, d)
        if cb == 0.0:
            assert rpy[0] == 0.0, name
        bad, _ = fc.closed_form_rpy_f32(R, lock_sign_inverted=True)
        if float(np.abs(fc.rebuild_from_rpy(bad) - R.T.astype(np.float64)).max()) >= fc.TOL_REBUILD:
            mutant_caught.append(name)
    assert worst_rebuild < 0.1 * fc.TOL_REBUILD and worst_deg < 0.1 * fc.TOL_RPY_DEG  # the bars leave the fp32 formula a wide margin
    assert set(mutant_caught) >= {"lock_yaw_p90_roll_pitch", "lock_yaw_m90_roll_pitch"}, mutant_caught
