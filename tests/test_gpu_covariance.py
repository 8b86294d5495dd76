"""ceres_hip_bal_covariance on the device, through the C ABI, against the numpy restatement (tests/covariance_reference.py, held to the
reference's known answers and to its own second route by tests/test_covariance_cpu.py) on the scenes of tests/covariance_cases.py.

PARITY.  Every requested block against route (a), np.linalg.inv(J^T J), in the correlation scale |Delta_ij| / sqrt(Cov_ii Cov_jj) with
the diagonal from the reference.  The bound is 10 y, y = the larger, over all cases, of the restatement's own route (a) against route
(b) deviation and of route (a)'s deviation when every Jacobian value is multiplied by 1 + 1e-15 N(0, 1) (seeds 1 and 2) — computed from
the restatement at run time, never from the device.  The factor ten is the one design/14_cluster_jacobi.md §14.3 gives the cluster
preconditioner, for the same reason: the device factors the matrix its own elimination formed.  design/17_covariance.md records y and
the device's figures."""
import ctypes

import numpy as np
import pytest

import covariance_cases as CC
import covariance_reference as CR

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


@pytest.fixture(scope="module")
def bound(oracle, hip):
    y, per = CC.yardstick(oracle, hip)
    for name, (route, noise) in per.items():
        print(f"yardstick {name}: route (a) against (b) {route:.3e}, Jacobian noise 1e-15 {noise:.3e}")
    print(f"yardstick y = {y:.3e}, bound 10 y = {10 * y:.3e}")
    return 10.0 * y


_device = {}


def device_blocks(hip, oracle, name):
    """The device's blocks of a success case, computed once and shared: (blocks, summary)."""
    if name not in _device:
        c = CC.case(oracle, name)
        gp = c.device_problem(hip)
        try:
            _device[name] = gp.covariance(c.state(hip), c.pairs)
        finally:
            gp.close()
    return _device[name]


def parity(hip, oracle, name, blocks, apply_loss_function=True):
    c = CC.case(oracle, name)
    layout, _, a, _ = CC.reference_results(oracle, hip, name, apply_loss_function)
    return CR.correlation_deviation(blocks, layout.blocks(a, c.pairs), layout.scales(np.diag(a), c.pairs))


@pytest.mark.parametrize("name", CC.SUCCESS)
def test_parity_with_the_dense_inverse(hip, oracle, bound, name):
    blocks, S = device_blocks(hip, oracle, name)
    _, _, _, b = CC.reference_results(oracle, hip, name)
    dev = parity(hip, oracle, name, blocks)
    print(f"{name}: device against route (a) {dev:.3e} (bound {bound:.3e}); pivots device {S.min_point_pivot:.3e} / {S.min_schur_pivot:.3e}, "
          f"restatement {b['min_point_pivot']:.3e} / {b['min_schur_pivot']:.3e}; device_bytes {S.device_bytes}")
    assert S.termination_type == hip.SUCCESS and S.message == b"Success."
    assert all(np.all(np.isfinite(blk)) for blk in blocks)
    assert dev <= bound, (dev, bound)
    # the pivots are the restatement's to the digits a pivot of that size keeps (float64, unit-diagonal matrices: 1e-12 absolute is ample)
    assert abs(S.min_point_pivot - b["min_point_pivot"]) <= 1e-9 and abs(S.min_schur_pivot - b["min_schur_pivot"]) <= 1e-9
    layout = CC.reference_results(oracle, hip, name)[0]
    assert S.device_bytes >= 8 * (layout.cw * layout.nfc) ** 2 + 8 * 9 * layout.nfp   # the second n x n buffer and the point blocks at least


def test_scene_a_residual(hip, oracle):
    """The whole matrix of scene A assembled from the blocks: |J^T J Cov - I|_max is at most ten times numpy's own figure for inv."""
    name = "A-cameras01"
    c = CC.case(oracle, name)
    blocks, _ = device_blocks(hip, oracle, name)
    layout, J, a, _ = CC.reference_results(oracle, hip, name)
    cov = np.zeros((layout.n, layout.n))
    for (p, q), blk in zip(c.pairs, blocks):
        rp, rq = layout.columns(int(p)), layout.columns(int(q))
        if rp is not None and rq is not None:
            cov[np.ix_(rp, rq)] = blk
    H = J.T @ J
    own = float(np.max(np.abs(H @ a - np.eye(layout.n))))
    dev = float(np.max(np.abs(H @ cov - np.eye(layout.n))))
    print(f"{name}: |J^T J Cov - I|_max device {dev:.3e}, numpy inv {own:.3e}")
    assert np.array_equal(cov, cov.T)
    assert dev <= 10.0 * own, (dev, own)


@pytest.mark.parametrize("name", CC.SUCCESS)
def test_structure_and_repeatability(hip, oracle, name):
    """(b, a) is the exact transpose of (a, b); a repeated pair has identical bits; pairs with a constant block are exactly zero; a second
    call and a fresh handle give identical bits."""
    c = CC.case(oracle, name)
    layout = CC.reference_results(oracle, hip, name)[0]
    first, _ = device_blocks(hip, oracle, name)
    seen = {}
    n_transposed = n_repeated = n_constant = 0
    for (p, q), blk in zip(c.pairs.tolist(), first):
        assert blk.shape == (layout.size(p), layout.size(q))
        if (p, q) in seen:
            assert np.array_equal(seen[(p, q)], blk)
            n_repeated += 1
        if (q, p) in seen and p != q:
            assert np.array_equal(seen[(q, p)].T, blk)
            n_transposed += 1
        if layout.columns(p) is None or layout.columns(q) is None:
            assert not blk.any()
            n_constant += 1
        seen[(p, q)] = blk
    assert n_transposed > 0 and n_constant > 0 and (n_repeated > 0 or name.startswith("A-"))
    gp = c.device_problem(hip)
    try:
        x = c.state(hip)
        again, _ = gp.covariance(x, c.pairs)
        twice, _ = gp.covariance(x, c.pairs)
    finally:
        gp.close()
    assert all(np.array_equal(u, v) for u, v in zip(first, again))    # a fresh handle
    assert all(np.array_equal(u, v) for u, v in zip(again, twice))    # a second call


def test_apply_loss_function(hip, oracle, bound):
    """apply_loss_function = 0 on the Huber handle is the no-loss handle's result (within the parity bound, against the restatement
    without a loss), and differs from the loss-corrected one; the handle's loss is still in force afterwards."""
    name = "C-angle_axis-huber"
    c = CC.case(oracle, name)
    x = c.state(hip)
    with_loss, _ = device_blocks(hip, oracle, name)
    gp = c.device_problem(hip)
    try:
        cost_before = gp.evaluate(x)[0]
        off, _ = gp.covariance(x, c.pairs, apply_loss_function=False)
        assert gp.evaluate(x)[0] == cost_before
        on_again, _ = gp.covariance(x, c.pairs)
    finally:
        gp.close()
    nc, npts, cam, pt, obs, _ = c.scene
    plain = hip.BalProblem(hip.LinearSolverOptions(type=hip.DENSE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, max_num_iterations=100), nc, npts, cam, pt,
                           obs, camera_model=c.camera, constant_cameras=c.cc, constant_points=c.cp)
    try:
        no_loss, _ = plain.covariance(x, c.pairs)
    finally:
        plain.close()
    dev = parity(hip, oracle, name, off, apply_loss_function=False)
    dev_plain = parity(hip, oracle, name, no_loss, apply_loss_function=False)
    print(f"{name}: apply_loss_function = 0 against route (a) without a loss {dev:.3e}, the no-loss handle {dev_plain:.3e} (bound {bound:.3e})")
    assert dev <= bound and dev_plain <= bound
    assert all(np.array_equal(u, v) for u, v in zip(off, no_loss))   # the same kernels on the same Jacobian
    assert parity(hip, oracle, name, with_loss, apply_loss_function=False) > 1e3 * bound   # the Huber correction is visible
    assert all(np.array_equal(u, v) for u, v in zip(with_loss, on_again))


def raw(gp, hip, c, **kw):
    out = np.full(int(sum(gp.covariance_block_size(int(p)) * gp.covariance_block_size(int(q)) for p, q in c.pairs)), SENTINEL)
    rc, out, S = gp.covariance_raw(c.state(hip), c.pairs, out=out, **kw)
    return rc, out, S


@pytest.mark.parametrize("name", CC.FAILURE)
def test_rank_deficient_problems_fail(hip, oracle, name):
    """A free gauge (only camera 0 constant, nothing constant), the Euclidean quaternion camera and a point of one observation: the call
    returns 0 with FAILURE, the message names the factorisation, blocks_out is not written."""
    c = CC.case(oracle, name)
    gp = c.device_problem(hip)
    try:
        rc, out, S = raw(gp, hip, c)
        print(f"{name}: pivots {S.min_point_pivot:.3e} / {S.min_schur_pivot:.3e}: {S.message.decode()}")
        assert rc == 0 and S.termination_type == hip.FAILURE
        assert np.all(out == SENTINEL)
        msg = S.message.decode()
        assert "rank deficient" in msg
        if c.stage == "point":
            assert msg.startswith("The point factorization failed") and S.min_point_pivot <= 1e-8 and S.min_schur_pivot == -1.0
        else:
            assert msg.startswith("The Schur complement factorization failed") and S.min_point_pivot > 1e-4 and S.min_schur_pivot <= 1e-8
        with pytest.raises(hip.HipError) as e:
            gp.covariance(c.state(hip), c.pairs)
        assert "factorization failed" in str(e.value)
    finally:
        gp.close()


def test_zero_limit_still_succeeds_on_a_full_rank_scene(hip, oracle, bound):
    name = "A-cameras01"
    c = CC.case(oracle, name)
    gp = c.device_problem(hip)
    try:
        blocks, S = gp.covariance(c.state(hip), c.pairs, min_scaled_pivot=0.0)
    finally:
        gp.close()
    assert S.termination_type == hip.SUCCESS
    assert all(np.array_equal(u, v) for u, v in zip(blocks, device_blocks(hip, oracle, name)[0]))


def test_refusals_leave_the_handle_usable(hip, oracle):
    name = "A-cameras01"
    c = CC.case(oracle, name)
    x = c.state(hip)
    lib = hip.load_library()
    it = c.device_problem(hip, solver_type=hip.ITERATIVE_SCHUR)
    try:
        rc, out, _ = raw(it, hip, c)
        assert rc == -2 and np.all(out == SENTINEL)
        assert b"DENSE_SCHUR" in lib.ceres_hip_bal_last_error(it._h)
        assert it.evaluate(x)[0] > 0.0
    finally:
        it.close()
    gp = c.device_problem(hip)
    try:
        nblocks = c.nc + c.npts
        for bad in ([(0, nblocks)], [(-1, 0)], [(nblocks + 5, 1)]):
            out = np.full(200, SENTINEL)
            rc, out, _ = gp.covariance_raw(x, bad, out=out)
            assert rc == -1 and np.all(out == SENTINEL)
            assert b"out of range" in lib.ceres_hip_bal_last_error(gp._h)
        for value in (float("nan"), float("inf"), -1e-3):
            rc, out, _ = raw(gp, hip, c, min_scaled_pivot=value)
            assert rc == -1 and np.all(out == SENTINEL)
            assert b"min_scaled_pivot" in lib.ceres_hip_bal_last_error(gp._h)
        S = hip.CCovarianceSummary()
        a = np.zeros(1, dtype=np.int32)
        ip = a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out = np.full(9, SENTINEL)
        assert lib.ceres_hip_bal_covariance(gp._h, None, None, 1, ip, ip, hip._p(out), ctypes.byref(S)) == -1       # state
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), 1, None, ip, hip._p(out), ctypes.byref(S)) == -1  # pair arrays
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), 1, ip, None, hip._p(out), ctypes.byref(S)) == -1
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), 1, ip, ip, None, ctypes.byref(S)) == -1           # output
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), 1, ip, ip, hip._p(out), None) == -1               # summary
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), -1, ip, ip, hip._p(out), ctypes.byref(S)) == -1
        assert np.all(out == SENTINEL)
        # options == NULL: the defaults; no pairs: the factorisations alone
        assert lib.ceres_hip_bal_covariance(gp._h, None, hip._p(x), 0, None, None, None, ctypes.byref(S)) == 0 and S.termination_type == hip.SUCCESS
        blocks, _ = gp.covariance(x, c.pairs)
    finally:
        gp.close()
    assert all(np.array_equal(u, v) for u, v in zip(blocks, device_blocks(hip, oracle, name)[0]))


@pytest.mark.parametrize("generic", [True, False], ids=["generic", "fused"])
def test_minimize_is_not_affected(hip, oracle, generic):
    """minimize on a fresh handle gives the same summary and state whether or not covariance was called on it before.  On the generic
    kernels (every sum in a fixed order) the two runs agree bit for bit.  The fused kernels' sums in LDS are not bitwise repeatable between
    two handles with or without this feature (test_gpu_frontend_matrix.EDGE_DEVICE_UNREPEATABLE: accepted iterates of two plain runs
    agree to 4e-12): there the flags, the counts and the termination are compared exactly, costs, radii and the state to 1e-10 relative —
    a diagonal, a loss or values left behind by covariance would move them by far more."""
    c = CC.case(oracle, "B-cameras01-points3")
    x = c.state(hip)
    nc, npts, cam, pt, obs, _ = c.scene
    runs = []
    for call_first in (False, True):
        o = hip.LinearSolverOptions(type=hip.DENSE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=100,
                                    force_generic_path=generic)
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=c.camera, constant_cameras=c.cc, constant_points=c.cp)
        try:
            if call_first:
                gp.covariance(x, c.pairs)
                gp.covariance(x, c.pairs[:7], apply_loss_function=False)
            runs.append(gp.minimize(x, max_num_iterations=6))
        finally:
            gp.close()
    (x0, s0), (x1, s1) = runs
    rtol = 0.0 if generic else 1e-10
    same = lambda u, v: u == v if isinstance(u, (int, bytes)) else abs(u - v) <= rtol * max(abs(u), abs(v))
    assert s0.num_iterations_logged == s1.num_iterations_logged and s0.num_iterations_logged >= 3
    for f in ("initial_cost", "final_cost", "num_successful_steps", "num_unsuccessful_steps", "num_linear_solves", "termination_type", "message"):
        assert same(getattr(s0, f), getattr(s1, f)), (f, getattr(s0, f), getattr(s1, f))
    for i in range(s0.num_iterations_logged):
        for f, _ in hip.CIterationSummary._fields_:
            u, v = getattr(s0.iterations[i], f), getattr(s1.iterations[i], f)
            if f == "cost_change" and not generic:   # (a difference of two costs: to the costs' own tolerance)
                assert abs(u - v) <= rtol * s0.iterations[i].cost, (i, f, u, v)
            elif f in ("relative_decrease", "gradient_max_norm", "step_norm") and not generic:   # (quantities that shrink towards convergence: differences of nearly equal numbers)
                assert abs(u - v) <= 1e-6 * max(abs(u), 1.0), (i, f, u, v)
            else:
                assert same(u, v), (i, f, u, v)
    print(f"generic = {generic}: largest state difference {np.max(np.abs(x0 - x1)):.3e}, final costs {s0.final_cost!r} {s1.final_cost!r}")
    assert np.all(np.abs(x0 - x1) <= rtol * (1.0 + np.abs(x0)))
    assert s0.final_cost < s0.initial_cost


def test_poisoned_allocations_do_not_reach_the_blocks(hip, oracle, bound, monkeypatch):
    """CERES_HIP_DEBUG_POISON=nan, set before the handle is created, fills every new floating-point device buffer with NaN: the second
    n x n buffer, the point blocks and the output must be written before they are read."""
    monkeypatch.setenv("CERES_HIP_DEBUG_POISON", "nan")
    name = "B-cameras01-points3"
    c = CC.case(oracle, name)
    gp = c.device_problem(hip)
    try:
        blocks, S = gp.covariance(c.state(hip), c.pairs)
    finally:
        gp.close()
    assert S.termination_type == hip.SUCCESS
    assert all(np.all(np.isfinite(blk)) for blk in blocks)
    assert parity(hip, oracle, name, blocks) <= bound
