"""Constant parameter blocks of the BAL front end without a GPU: the restatement (tests/constant_blocks_reference.py) against things
that do not depend on it — the unwrapped evaluators and minimizer of tests/frontend_reference.py — and the library's host-side reduction
(ceres_hip_debug_bal_reduce, csrc/constant_blocks.inc) against the restatement's, exactly."""
import ctypes

import numpy as np
import pytest

import constant_blocks_reference as CB
import frontend_reference as F
from conftest import pkg
from test_gpu_frontend_matrix import LOSS_PARAMS, clean_scene, edge_scene

hs = pkg.hip_solver
EPS = np.finfo(np.float64).eps
HUBER = ("huber",) + LOSS_PARAMS["huber"] + (1.0,)


@pytest.fixture(scope="module")
def scenes(oracle):
    return {"clean": clean_scene(oracle), "edge": edge_scene(oracle)}


def state(sc, model):
    nc, npts, _, _, _, par = sc
    cams, pts = par[:9 * nc], par[9 * nc:]
    if model:
        c9 = cams.reshape(-1, 9)
        cams = np.concatenate([hs.angle_axis_to_quaternion(c9[:, :3]), c9[:, 3:]], axis=1).reshape(-1)
    return np.concatenate([pts, cams])


def unwrapped(oracle, sc, model, loss, rows=None):
    nc, npts, cam, pt, obs, _ = sc
    order = np.argsort(pt, kind="stable") if rows is None else rows
    return F.problem(oracle.snavely_batch, model, nc, npts, cam, pt, obs, order, loss)


@pytest.mark.parametrize("model,loss", [(0, None), (0, HUBER), (1, HUBER), (2, None)])
def test_nothing_constant_is_the_unwrapped_problem(oracle, scenes, model, loss):
    sc = scenes["clean"]
    nc, npts, cam, pt, obs, _ = sc
    x0 = state(sc, model)
    ev = unwrapped(oracle, sc, model, loss)
    w = CB.Problem(oracle.snavely_batch, model, nc, npts, cam, pt, obs, None, [], loss)
    assert w.n == ev.n and np.array_equal(w.row_order, np.argsort(pt, kind="stable")) and w.fixed_cost(x0) == 0.0
    a, b = ev.evaluate(x0), w.evaluate(x0)
    assert a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]))
    assert np.array_equal(ev.dense_jacobian(a[2]), w.dense_jacobian(b[2]))
    for strategy in ("lm", "subspace"):
        xa, Sa = F.minimize(ev, x0, strategy, max_num_iterations=5)
        xb, Sb = F.minimize(w, x0, strategy, max_num_iterations=5)
        assert np.array_equal(xa, xb) and Sa == Sb
    if model == 0:
        inner = w.inner_ordering("automatic")
        import inner_reference as IR
        ref = IR.ordering(nc, npts, cam, pt, "automatic")
        assert np.array_equal(inner[0], ref[0]) and inner[1] == ref[1]
        xa, Sa = F.minimize(ev, x0, "lm", inner=ref, max_num_iterations=3)
        xb, Sb = F.minimize(w, x0, "lm", inner=inner, max_num_iterations=3)
        assert np.array_equal(xa, xb) and Sa == Sb


@pytest.mark.parametrize("scene", ["clean", "edge"])
@pytest.mark.parametrize("name", CB.MASK_SETS)
@pytest.mark.parametrize("model,loss", [(0, None), (0, HUBER), (1, HUBER), (2, HUBER)])
def test_reduced_program_is_the_full_one_with_blocks_deleted(oracle, scenes, scene, name, model, loss):
    sc = scenes[scene]
    nc, npts, cam, pt, obs, _ = sc
    cc, cp = CB.mask_set(name, nc, npts, cam, pt)
    x0 = state(sc, model)
    ev = unwrapped(oracle, sc, model, loss)
    full_order = np.argsort(pt, kind="stable")
    w = CB.Problem(oracle.snavely_batch, model, nc, npts, cam, pt, obs, cc, cp, loss)
    cost_f, r_f, vals_f, g_f = ev.evaluate(x0)
    cost_r, r_r, vals_r, g_r = w.evaluate(x0)
    J_f, J_r = ev.dense_jacobian(vals_f), w.dense_jacobian(vals_r)
    # columns: the constant blocks' deleted — stated here from the masks, not from the wrapper
    cw, cs = (10 if model == 1 else 9), (10 if model else 9)
    keep_col = np.ones(J_f.shape[1], bool)
    for q in cp:
        keep_col[3 * q:3 * q + 3] = False
    for c in cc:
        keep_col[3 * npts + cw * c:3 * npts + cw * (c + 1)] = False
    # rows: a row of the full problem is deleted when both its blocks are constant; the kept ones permuted by the row order
    pos_of_obs = np.empty(cam.shape[0], np.int64)
    pos_of_obs[full_order] = np.arange(cam.shape[0])
    both = np.isin(cam, cc) & np.isin(pt, cp)
    assert set(w.row_order.tolist()) == set(np.flatnonzero(~both).tolist()) and w.row_order.size == np.count_nonzero(~both)
    rows = pos_of_obs[w.row_order]
    sel = (2 * rows[:, None] + np.arange(2)).reshape(-1)
    assert np.array_equal(J_r, J_f[sel][:, keep_col])
    assert np.array_equal(r_r, r_f[sel])
    assert w.n == np.count_nonzero(keep_col) and vals_r.size == 6 * w.n_rows_e + 2 * cw * np.count_nonzero(~np.isin(cam[w.row_order], cc))
    # the rows without an E cell come last, in observation order; the others are grouped by point, stable
    tail = w.row_order[w.n_rows_e:]
    assert np.all(np.isin(pt[tail], cp)) and np.all(np.diff(tail) > 0)
    head = w.row_order[:w.n_rows_e]
    assert not np.any(np.isin(pt[head], cp)) and np.all(np.diff(pt[head]) >= 0)
    assert all(np.all(np.diff(head[pt[head] == q]) > 0) for q in np.unique(pt[head])[:20])
    # the fixed cost is the unwrapped evaluator's cost over the deleted rows; reduced + fixed = full up to summation error
    removed = np.flatnonzero(both)
    fixed = unwrapped(oracle, sc, model, loss, rows=removed).cost(x0) if removed.size else 0.0
    assert w.fixed_cost(x0) == fixed
    assert (name == "both_constant") <= (removed.size > 0 and fixed > 0.0)
    n_rows = cam.shape[0]
    assert abs(cost_r + fixed - cost_f) <= n_rows * EPS * cost_f
    # the gradient: the free blocks' entries of the FULL problem's (the removed rows touch constant blocks only)
    assert np.max(np.abs(g_r - g_f[keep_col])) <= n_rows * EPS * np.max(np.abs(g_f))
    # Plus: constant blocks untouched, free blocks as the unwrapped Plus moves them
    rng = np.random.default_rng(3)
    delta = 1e-3 * rng.standard_normal(w.n)
    x1 = w.plus(x0, delta)
    const = np.zeros(x0.size, bool)
    for q in cp:
        const[3 * q:3 * q + 3] = True
    for c in cc:
        const[3 * npts + cs * c:3 * npts + cs * (c + 1)] = True
    assert np.array_equal(x1[const], x0[const])
    d_full = np.zeros(J_f.shape[1])
    d_full[keep_col] = delta
    assert np.array_equal(x1[~const], ev.plus(x0, d_full)[~const])
    assert np.count_nonzero(x1[~const] != x0[~const]) >= w.n - 4 * nc   # (a quaternion's four move together; nothing else stays)


@pytest.mark.parametrize("scene", ["clean", "edge"])
@pytest.mark.parametrize("name", CB.MASK_SETS)
def test_library_reduction_equals_the_restatement(scenes, scene, name):
    nc, npts, cam, pt, _, _ = scenes[scene]
    cc, cp = CB.mask_set(name, nc, npts, cam, pt)
    rows_r, ne_r, ccol_r, pcol_r, removed = CB.reduce(nc, npts, cam, pt, cc, cp)
    for as_mask in (False, True):
        a = CB.mask(cc, nc) if as_mask else cc
        b = CB.mask(cp, npts) if as_mask else cp
        rows, ne, ccol, pcol = hs.debug_bal_reduce(nc, npts, cam, pt, a, b)
        assert np.array_equal(rows, rows_r) and ne == ne_r and np.array_equal(ccol, ccol_r) and np.array_equal(pcol, pcol_r)
    assert rows_r.size + removed.size == cam.shape[0]
    if name == "none":
        assert np.array_equal(rows_r, np.argsort(pt, kind="stable")) and ne_r == cam.shape[0]
    if name == "camera_of_constant_points":
        assert ne_r < rows_r.size and removed.size == 0
    if name == "both_constant":
        assert removed.size >= 1
    if name == "point_of_constant_cameras":
        q = int(np.argmin(np.bincount(pt, minlength=npts)))
        assert pcol_r[q] >= 0 and np.all(ccol_r[cam[pt == q]] < 0)


def test_library_reduction_refuses(scenes):
    nc, npts, cam, pt, _, _ = scenes["clean"]
    lib = hs.load_library()
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    nr, ne = ctypes.c_int64(), ctypes.c_int64()

    def call(cam_, pt_, cm=None, pm=None, nc_=nc, npts_=npts):
        return lib.ceres_hip_debug_bal_reduce(nc_, npts_, cam.shape[0], i32(cam_) if cam_ is not None else None, i32(pt_) if pt_ is not None else None,
                                              u8(cm) if cm is not None else None, u8(pm) if pm is not None else None, ctypes.byref(nr),
                                              ctypes.byref(ne), None, None, None)

    msg = lambda: lib.ceres_hip_bal_last_error(None).decode()
    assert call(cam, pt) == 0 and nr.value == ne.value == cam.shape[0]   # outputs are NULL-able
    assert call(cam, pt, np.ones(nc, np.uint8)) == hs.E_INVALID
    assert "every camera is constant" in msg() and "LinearSolverForZeroEBlocks" in msg() and "this front end does not" in msg()
    assert call(cam, pt, None, np.ones(npts, np.uint8)) == hs.E_INVALID
    assert "every point is constant" in msg() and "LinearSolverForZeroEBlocks" in msg()
    assert call(None, pt) == hs.E_INVALID and "bad arguments" in msg()
    assert call(cam, None) == hs.E_INVALID and "bad arguments" in msg()
    bad = cam.copy()
    bad[5] = nc
    assert call(bad, pt) == hs.E_INVALID and "out of range" in msg()
    bad = pt.copy()
    bad[7] = -1
    assert call(cam, bad) == hs.E_INVALID and "out of range" in msg()
    assert call(cam, pt, nc_=0) == hs.E_INVALID
    with pytest.raises(hs.HipError, match="every camera is constant"):
        hs.debug_bal_reduce(nc, npts, cam, pt, np.ones(nc, bool), None)
    with pytest.raises(ValueError):
        hs.debug_bal_reduce(nc, npts, cam, pt, [nc], None)


def test_option_validation_before_device(scenes):
    """What ceres_hip_bal_create_with_constant_blocks refuses, it refuses before any device call: the same messages with and without
    a GPU."""
    nc, npts, cam, pt, obs, _ = scenes["clean"]
    o = hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI)
    with pytest.raises(hs.HipError) as e:
        hs.BalProblem(o, nc, npts, cam, pt, obs, constant_cameras=np.ones(nc, bool))
    assert "ceres_hip_bal_create_with_constant_blocks: every camera is constant" in str(e.value) and "LinearSolverForZeroEBlocks" in str(e.value)
    with pytest.raises(hs.HipError) as e:
        hs.BalProblem(o, nc, npts, cam, pt, obs, camera_model="quaternion", constant_points=np.arange(npts))
    assert "ceres_hip_bal_create_with_constant_blocks: every point is constant" in str(e.value)
    with pytest.raises(hs.HipError) as e:
        hs.BalProblem(o, nc, npts, cam, pt, obs, camera_model=7, constant_cameras=[0])
    assert "ceres_hip_bal_create_with_constant_blocks: unknown camera_model 7" in str(e.value)
    bad = cam.copy()
    bad[0] = nc
    with pytest.raises(hs.HipError) as e:
        hs.BalProblem(o, nc, npts, bad, pt, obs, constant_cameras=[0])
    assert "observation index out of range" in str(e.value)
    for kw in (dict(constant_cameras=[nc]), dict(constant_points=[-1]), dict(constant_cameras=np.ones(nc + 1, bool))):
        with pytest.raises(ValueError):
            hs.BalProblem(o, nc, npts, cam, pt, obs, **kw)
    # the masks are accepted and the call gets as far as the device
    if hs.device_count() == 0:
        with pytest.raises(hs.HipError) as e:
            hs.BalProblem(o, nc, npts, cam, pt, obs, constant_cameras=[0])
        assert "no HIP device" in str(e.value) or "no CPU fallback" in str(e.value)
