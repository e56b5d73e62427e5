"""GPU (-m gpu): csrc/flame.hip on the planted cases of tests/flame_cases.py -- what tests/test_gpu_parity.py's random 413-vectors on the one model shape
never reach: the prologue's branches (gimbal lock, the pitch wrap, F.normalize's eps, the scale clamp, zero and large jaws), a different un-pad row per
head, vgh_flame_decode_indirect called directly (permuted / repeated head_row, non-monotone head_image, live count below capacity, the capacity-dependent
dispatch), the chunk loop beyond max_heads, odd and empty live ranges, joints_dev, and models of other shapes than 5023 / 400 / 5.

References: oracle/flame_oracle.py in float64 (reproject, lbs, calculate_rpy).  Tolerances: the project's own (flame_cases.TOL_*), the projected one per head;
tests/test_flame_cases_host.py holds the float32 oracle to half of each.  Bit-identity: every vertex kernel against the VALU one (mode 0), and a head against
itself in another batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import flame_cases as fc
from oracle import flame_oracle as fo

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
VGH_ERR_INVALID = -1


def _dev():
    return torch.device("cuda", 0)


def _sp():
    return torch.cuda.current_stream().cuda_stream


def _layer(flame_model, max_heads):
    from head_detector_amd.flame import FLAMELayer

    return FLAMELayer(model=flame_model, device=_dev(), max_heads=max_heads)


@pytest.fixture(scope="module")
def layer64(gpu_lib, flame_model):
    return _layer(flame_model, 64)


@pytest.fixture(scope="module")
def planted(flame_model):
    """The table, its un-pad rows and the float64 reference: computed once, never modified."""
    p, names = fc.planted_heads()
    unpad = fc.distinct_unpad(len(names))
    v64, R64, q64 = fc.reference(flame_model, p, unpad, torch.float64)
    R32 = fo.rot_mat_from_6dof(p[:, fc.ROT6])
    return {"p": p, "names": names, "unpad": unpad, "v64": v64, "R64": R64, "q64": q64, "R32": R32, "proper": fc.proper_rotation(R32)}


def _modes(gpu_lib, modes, fn):
    """{mode: fn()} under vgh_flame_set_matrix_path(mode); the automatic mode is restored whatever happens."""
    outs = {}
    try:
        for mode in modes:
            assert gpu_lib.vgh_flame_set_matrix_path(mode) == 0
            outs[mode] = fn()
    finally:
        gpu_lib.vgh_flame_set_matrix_path(1)
    return outs


def _assert_heads_vs_f64(names, v, R, q, v64, R64, q64, skip_R=()):
    """Per head: vertices and R within 2e-6, projected within 1e-6 * max(1000, max |q64| of that head) (or the measured bar of fc.MEASURED_TOL)."""
    worst = {"verts": 0.0, "R": 0.0, "proj_rel": 0.0}
    fails = []
    for h, name in enumerate(names):
        errs = {"verts": float((v[h].double() - v64[h]).abs().max()), "R": float((R[h].double() - R64[h]).abs().max()),
                "proj_rel": float((q[h].double() - q64[h]).abs().max()) / max(1000.0, float(q64[h].abs().max()))}
        for what, e in errs.items():
            if what == "R" and name in skip_R:
                continue
            worst[what] = max(worst[what], e / fc.tol(name, what))
            if not e < fc.tol(name, what):  # (also a NaN)
                fails.append((name, what, e))
    print(f"[flame cases] device / bar: {worst}")
    assert not fails, fails


def _decode_indirect(lib, layer, params, head_row, head_image, n_live, capacity, unpad, verts, rot, rpy, proj, live=fc.LIVE):
    n_dev = torch.tensor([n_live], dtype=torch.int32, device=_dev())
    from head_detector_amd import _lib

    return lib.vgh_flame_decode_indirect(layer._need_handle(), _lib.ptr(params), _lib.ptr(head_row), _lib.ptr(head_image), _lib.ptr(n_dev), capacity, live[0], live[1],
                                         _lib.ptr(unpad), _lib.ptr(verts), _lib.ptr(rot), _lib.ptr(rpy), _lib.ptr(proj), _sp())


# ======================================================================================================
# 1. planted heads through vgh_flame_decode, a different un-pad row per head
# ======================================================================================================
def test_planted_heads_direct(gpu_lib, layer64, planted):
    p, unpad, names = planted["p"].to(_dev()), planted["unpad"].to(_dev()), planted["names"]
    outs = _modes(gpu_lib, (0, 1, 2, 6, 7), lambda: [t.clone() for t in layer64.decode(p, unpad=unpad, shape_live=fc.LIVE[0], expr_live=fc.LIVE[1])])
    for mode in (1, 2, 6, 7):
        for a, b in zip(outs[mode], outs[0]):
            assert torch.equal(a, b), mode
    v, R, q = (t.cpu() for t in outs[0])
    assert torch.isfinite(v).all() and torch.isfinite(R).all() and torch.isfinite(q).all()
    for name, cols in fc.ZERO_COLUMN_CASES.items():  # the fp32 oracle's exact zero columns, exactly
        h = names.index(name)
        for c in range(3):
            assert bool((R[h][:, c] == 0).all()) == (c in cols) == bool((planted["R32"][h][:, c] == 0).all()), (name, c)
    _assert_heads_vs_f64(names, v, R, q, planted["v64"], planted["R64"], planted["q64"])


# ======================================================================================================
# 2. roll / pitch / yaw of the planted rotations (vgh_flame_decode_indirect, identity head list)
# ======================================================================================================
def test_planted_heads_roll_pitch_yaw(gpu_lib, layer64, planted):
    names, n = planted["names"], len(planted["names"])
    p, unpad = planted["p"].to(_dev()), planted["unpad"].to(_dev())
    ident = torch.arange(n, dtype=torch.int32, device=_dev())
    rot = torch.full((n, 3, 3), SENTINEL, device=_dev())
    rpy = torch.full((n, 3), SENTINEL, device=_dev())
    proj = torch.full((n, layer64.num_vertices, 3), SENTINEL, device=_dev())
    assert _decode_indirect(gpu_lib, layer64, p, ident, ident, n, n, unpad, None, rot, rpy, proj) == 0
    _, R_direct, q_direct = layer64.decode(p, unpad=unpad, shape_live=fc.LIVE[0], expr_live=fc.LIVE[1], want_vertices=False)
    assert torch.equal(rot, R_direct) and torch.equal(proj, q_direct)
    rot, rpy = rot.cpu().numpy(), rpy.cpu().numpy()
    assert not (rpy == SENTINEL).any() and np.isfinite(rpy).all()  # every row written, the degenerate ones too
    worst_rebuild, worst_deg, fails = 0.0, 0.0, []
    for h, name in enumerate(names):
        if not planted["proper"][h]:
            continue  # R is no rotation: the reference is undefined
        if not (np.abs(rpy[h]) <= 180.0).all():
            fails.append((name, "range", rpy[h].tolist()))
        # (b) the device's angles rebuild the device's own R^T: holds near gimbal lock too, where the two free angles may be split differently
        err = float(np.abs(fc.rebuild_from_rpy(rpy[h]) - rot[h].T.astype(np.float64)).max())
        worst_rebuild = max(worst_rebuild, err)
        if not err < fc.TOL_REBUILD:
            fails.append((name, "rebuild", err))
        # (c) scipy's angles where they are well conditioned, and its convention (third angle 0) at exact lock
        cb = float(np.sqrt(np.float32(rot[h][0, 0] * rot[h][0, 0]) + np.float32(rot[h][0, 1] * rot[h][0, 1])))
        if cb >= 1e-2 or cb == 0.0:
            d = float(fc.circ_dist_deg(rpy[h], fo.calculate_rpy(planted["p"][h, fc.ROT6])).max())
            worst_deg = max(worst_deg, d)
            if not d < fc.TOL_RPY_DEG:
                fails.append((name, "scipy", d, rpy[h].tolist()))
        if name in fc.LOCK_CASES and not (cb == 0.0 and rpy[h][0] == 0.0):
            fails.append((name, "lock", cb, rpy[h].tolist()))
    print(f"[flame cases] rpy: rebuild {worst_rebuild:.3g} (bar {fc.TOL_REBUILD}), scipy {worst_deg:.3g} deg (bar {fc.TOL_RPY_DEG})")
    assert not fails, fails


# ======================================================================================================
# 3. vgh_flame_decode_indirect against vgh_flame_decode of the gathered rows
# ======================================================================================================
@pytest.fixture(scope="module")
def layer4096(gpu_lib, flame_model):
    return _layer(flame_model, 4096)


@pytest.fixture(scope="module")
def head_list():
    """40 source rows; 33 heads that read them through a permutation with repeats (15 rows never used) and un-pad rows through a non-monotone head_image."""
    rng = np.random.default_rng(8)
    perm = rng.permutation(40)[:25]
    rows = rng.permutation(np.concatenate([perm, perm[:8]])).astype(np.int32)
    image = rng.integers(0, 7, size=33).astype(np.int32)
    assert len(set(rows.tolist())) == 25 and (np.diff(image) < 0).any() and (np.diff(image) > 0).any() and len(set(image.tolist())) == 7
    src = fo.synthetic_params(40, seed=77, live_shape=fc.LIVE[0], live_expr=fc.LIVE[1])
    return {"src": src, "rows": torch.from_numpy(rows), "image": torch.from_numpy(image), "unpad": fc.distinct_unpad(7, seed=9), "direct": {}}


@pytest.mark.parametrize("capacity", [8, 128, 129, 4096])
def test_indirect_equals_direct(gpu_lib, layer4096, head_list, capacity):
    """Capacity decides the launch (4-wave c3 blocks up to 128, 128-vertex blocks beyond, the multi-head prologue from 4 096), the live count on the device
    decides what is written: rows < n are the bits of a direct decode of the gathered rows, rows >= n are untouched."""
    dev, V = _dev(), layer4096.num_vertices
    src, unpad7 = head_list["src"].to(dev), head_list["unpad"].to(dev)
    want_verts = capacity < 4096  # (memory)
    verts = torch.empty(capacity, V, 3, device=dev) if want_verts else None
    proj, rot, rpy = torch.empty(capacity, V, 3, device=dev), torch.empty(capacity, 3, 3, device=dev), torch.empty(capacity, 3, device=dev)
    for n in (0, 1, 5, 33):
        if n > capacity:
            continue
        rows, image = torch.zeros(capacity, dtype=torch.int32), torch.zeros(capacity, dtype=torch.int32)  # beyond the live count: valid, and never to be read
        rows[:n], image[:n] = head_list["rows"][:n], head_list["image"][:n]
        for t in (verts, proj, rot, rpy):
            if t is not None:
                t.fill_(SENTINEL)
        assert _decode_indirect(gpu_lib, layer4096, src, rows.to(dev), image.to(dev), n, capacity, unpad7, verts, rot, rpy, proj) == 0
        for name, t in (("verts", verts), ("proj", proj), ("rot", rot), ("rpy", rpy)):
            if t is not None:
                assert bool((t[n:] == SENTINEL).all()), (name, n, "rows beyond the live count were written")
        if n == 0:
            continue
        if n not in head_list["direct"]:
            g_rows, g_img = head_list["rows"][:n].long().to(dev), head_list["image"][:n].long().to(dev)
            head_list["direct"][n] = layer4096.decode(src[g_rows].contiguous(), unpad=unpad7[g_img].contiguous(), shape_live=fc.LIVE[0], expr_live=fc.LIVE[1])
        dv, dR, dq = head_list["direct"][n]
        assert torch.equal(proj[:n], dq), ("proj", n)
        assert torch.equal(rot[:n], dR), ("rot", n)
        if want_verts:
            assert torch.equal(verts[:n], dv), ("verts", n)
        assert not bool((rpy[:n] == SENTINEL).any()) and bool(torch.isfinite(rpy[:n]).all())
    if capacity == 4096:  # a capacity above max_heads is refused on the host, before anything is queued
        big = torch.zeros(4097, dtype=torch.int32, device=dev)
        rot.fill_(SENTINEL)
        assert _decode_indirect(gpu_lib, layer4096, src, big, big, 1, 4097, unpad7, None, rot, None, None) == VGH_ERR_INVALID
        assert b"exceeds max_heads" in gpu_lib.vgh_last_error()
        assert bool((rot == SENTINEL).all())


# ======================================================================================================
# 4. the chunk loop of run_decode_on (n > max_heads)
# ======================================================================================================
def test_chunk_loop_beyond_max_heads(gpu_lib, flame_model, layer64, planted):
    from head_detector_amd import _lib

    dev = _dev()
    small = _layer(flame_model, 4)
    p, unpad = planted["p"][:11].to(dev), planted["unpad"][:11].to(dev)
    a = small.decode(p, unpad=unpad, shape_live=fc.LIVE[0], expr_live=fc.LIVE[1])  # chunks of 4, 4, 3
    b = layer64.decode(p, unpad=unpad, shape_live=fc.LIVE[0], expr_live=fc.LIVE[1])
    for name, x, y in zip(("verts", "rot", "proj"), a, b):
        assert torch.equal(x, y), name
    betas, pose = (t.to(dev) for t in fc.lbs_inputs(400, 5, 11, seed=44))
    outs = []
    for layer in (small, layer64):
        verts, joints = torch.full((11, layer.num_vertices, 3), SENTINEL, device=dev), torch.full((11, 5, 3), SENTINEL, device=dev)
        assert gpu_lib.vgh_flame_lbs(layer._need_handle(), _lib.ptr(betas), _lib.ptr(pose), 11, _lib.ptr(verts), _lib.ptr(joints), _sp()) == 0
        outs.append((verts, joints))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not bool((outs[0][0] == SENTINEL).any()) and not bool((outs[0][1] == SENTINEL).any())


# ======================================================================================================
# 5. a non-finite head leaves every other head's bits alone
# ======================================================================================================
def test_other_heads_do_not_depend_on_a_non_finite_head(gpu_lib, layer64):
    """(The two poisoned heads' own values are not asserted: fmaxf(NaN, 1e-8) and torch.clamp(NaN, 1e-8) differ by design -- include/vgh.h.)"""
    dev, n = _dev(), 33
    clean = fo.synthetic_params(n, seed=55, live_shape=fc.LIVE[0], live_expr=fc.LIVE[1])
    bad = clean.clone()
    bad[7] = float("nan")
    bad[20, fc.SCALE] = float("inf")
    unpad = fc.distinct_unpad(n, seed=6).to(dev)
    keep = torch.tensor([h for h in range(n) if h not in (7, 20)], device=dev)

    def run(p):
        return [t.clone() for t in layer64.decode(p.to(dev), unpad=unpad, shape_live=fc.LIVE[0], expr_live=fc.LIVE[1])]

    modes = (0, 1, 2, 6)
    ref, got = _modes(gpu_lib, modes, lambda: run(clean)), _modes(gpu_lib, modes, lambda: run(bad))
    for mode in modes:
        for name, x, y in zip(("verts", "rot", "proj"), got[mode], ref[mode]):
            assert torch.equal(x[keep], y[keep]), (mode, name)
            assert bool(torch.isfinite(y).all()), (mode, name)


# ======================================================================================================
# 6. odd and empty live ranges (they turn every matrix-core path off, or leave it nothing but the pose features)
# ======================================================================================================
@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("live", [(0, 0), (1, 1), (127, 63), (300, 0)])
def test_odd_and_empty_live_ranges(gpu_lib, layer64, flame_model, live, n):
    dev = _dev()
    p = fo.synthetic_params(n, seed=300 + 7 * live[0] + n, live_shape=live[0], live_expr=live[1])  # exact zeros outside the live ranges, as the header requires
    assert not p[:, live[0] : 300].any() and not p[:, 300 + live[1] : 400].any()
    unpad = fc.distinct_unpad(n, seed=7)
    v64, R64, q64 = fc.reference(flame_model, p, unpad, torch.float64)
    outs = _modes(gpu_lib, (0, 1, 2), lambda: [t.clone() for t in layer64.decode(p.to(dev), unpad=unpad.to(dev), shape_live=live[0], expr_live=live[1])])
    for mode in (1, 2):
        for a, b in zip(outs[mode], outs[0]):
            assert torch.equal(a, b), mode
    v, R, q = (t.cpu() for t in outs[0])
    _assert_heads_vs_f64([f"live{live}_head{h}" for h in range(n)], v, R, q, v64, R64, q64)


# ======================================================================================================
# 7. joints_dev of vgh_flame_lbs
# ======================================================================================================
@pytest.fixture(scope="module")
def c64(flame_model):
    return fo.FlameConstants(flame_model, torch.float64)


def _lbs_modes(gpu_lib, handle, betas, pose, V, NJ, modes=(0, 1, 2, 6, 7)):
    from head_detector_amd import _lib

    dev, n = _dev(), betas.shape[0]
    b, q = betas.to(dev).contiguous(), pose.to(dev).contiguous()

    def run():
        verts, joints = torch.full((n, V, 3), SENTINEL, device=dev), torch.full((n, NJ, 3), SENTINEL, device=dev)
        assert gpu_lib.vgh_flame_lbs(handle, _lib.ptr(b), _lib.ptr(q), n, _lib.ptr(verts), _lib.ptr(joints), _sp()) == 0
        return verts, joints

    outs = _modes(gpu_lib, modes, run)
    for mode in modes[1:]:
        assert torch.equal(outs[mode][0], outs[0][0]), ("verts", mode)
        assert torch.equal(outs[mode][1], outs[0][1]), ("joints", mode)
    return outs[0][0].cpu(), outs[0][1].cpu()


@pytest.mark.parametrize("n", [1, 6, 40])
def test_lbs_joints_vs_oracle_f64(gpu_lib, layer64, c64, n):
    betas, pose = fc.lbs_inputs(400, 5, n, seed=500 + n)  # full 15-value poses, randn * 0.3
    v64, j64 = fc.lbs_reference(c64, betas, pose)
    verts, joints = _lbs_modes(gpu_lib, layer64._need_handle(), betas, pose, layer64.num_vertices, 5)
    ev, ej = float((verts.double() - v64).abs().max()), float((joints.double() - j64).abs().max())
    print(f"[flame cases] lbs n={n}: vertices {ev:.3g}, joints {ej:.3g} (bar {fc.TOL_LBS})")
    assert ev < fc.TOL_LBS and ej < fc.TOL_LBS


# ======================================================================================================
# 8. other model shapes than 5023 / 400 / 5
# ======================================================================================================
@pytest.mark.parametrize("name", sorted(fc.SMALL_MODELS))
def test_model_shapes(gpu_lib, name):
    """A: c3 tiles with K = 44.  B: NB % 8 != 0 (no c3 tiles).  C: odd K (VALU only), 8 joints.  D: one joint, one coefficient, 5 vertices.  E: one joint with
    the c3 conditions met (K == NB, an empty pose-feature run).  F: 54 pose features, NB > 64, a chain.  G: NB = 456 (the WIDE prologue's second chunk)."""
    from head_detector_amd import _lib

    V, NB, NJ, parents, _ = fc.SMALL_MODELS[name]
    c32 = fc.model_constants(fc.small_model(name), torch.float32)
    arrs = [np.ascontiguousarray(t.numpy()) for t in (c32.v_template, c32.shapedirs, c32.posedirs, c32.J_regressor, c32.lbs_weights)]
    if arrs[2].size == 0:
        arrs[2] = np.zeros(1, dtype=np.float32)  # NP = 0: no pose feature is read, the pointer only has to be non-null
    par = np.asarray(parents, dtype=np.int32)
    h = C.c_void_p()
    _lib.check(gpu_lib.vgh_flame_create(0, V, NB, NJ, _lib.ptr(arrs[0]), _lib.ptr(arrs[1]), _lib.ptr(arrs[2]), _lib.ptr(arrs[3]), _lib.ptr(par), _lib.ptr(arrs[4]), 256, C.byref(h)))
    try:
        worst = 0.0
        for n in fc.MODEL_NS:
            betas, pose, v64, j64 = fc.small_model_case(name, n)
            verts, joints = _lbs_modes(gpu_lib, h, betas, pose, V, NJ)
            ev, ej = float((verts.double() - v64).abs().max()), float((joints.double() - j64).abs().max())
            worst = max(worst, ev, ej)
            assert ev < fc.TOL_LBS and ej < fc.TOL_LBS, (name, n, ev, ej)
        print(f"[flame cases] model {name}: worst {worst:.3g} (bar {fc.TOL_LBS})")
    finally:
        torch.cuda.synchronize()
        gpu_lib.vgh_flame_destroy(h)
