"""ceres_hip_bal_covariance on handles with shared intrinsics (poses, points and groups; design/28_shared_covariance.md) on the device,
through the C ABI, against the numpy restatement: tests/shared_covariance_cases.py's scenes, pairs and layout, the shared-intrinsics
restatement's dense Jacobian through tests/covariance_reference.py's two routes (held to each other and to covariance_cases' 9-wide
camera blocks by tests/test_shared_covariance_cpu.py).

PARITY is tests/test_gpu_covariance.py's rule and factor, unchanged: every requested block against route (a), np.linalg.inv(J^T J), in
the correlation scale |Delta_ij| / sqrt(Cov_ii Cov_jj) with the diagonal from the reference; the bound is 10 y, y = the larger, over
these cases, of route (a) against route (b) and of route (a)'s move when every Jacobian value is multiplied by 1 + 1e-15 N(0, 1) (seeds 1
and 2) — computed from the restatement at run time, never from the device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import covariance_reference as CR
import shared_covariance_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
MESSAGE_27_1 = "the intrinsics of a group must be bit-identical"


@pytest.fixture(scope="module")
def bound(oracle):
    y, per = SC.yardstick(oracle)
    for name, (route, noise) in per.items():
        print(f"yardstick {name}: route (a) against (b) {route:.3e}, Jacobian noise 1e-15 {noise:.3e}")
    print(f"yardstick y = {y:.3e}, bound 10 y = {10 * y:.3e}")
    return 10.0 * y


_device = {}


def device_blocks(hip, oracle, name):
    """The device's blocks of a success case, computed once and shared: (blocks, summary)."""
    if name not in _device:
        c = SC.case(oracle, name)
        gp = c.device_problem(hip)
        try:
            _device[name] = gp.covariance(c.state(), c.pairs)
        finally:
            gp.close()
    return _device[name]


def parity(oracle, name, blocks, apply_loss_function=True):
    c = SC.case(oracle, name)
    layout, _, a, _ = SC.reference_results(oracle, name, apply_loss_function)
    return CR.correlation_deviation(blocks, layout.blocks(a, c.pairs), layout.scales(np.diag(a), c.pairs))


@pytest.mark.parametrize("name", SC.SUCCESS)
def test_parity_with_the_dense_inverse(hip, oracle, bound, name):
    c = SC.case(oracle, name)
    blocks, S = device_blocks(hip, oracle, name)
    layout, _, _, b = SC.reference_results(oracle, name)
    dev = parity(oracle, name, blocks)
    print(f"{name}: device against route (a) {dev:.3e} (bound {bound:.3e}); pivots device {S.min_point_pivot:.3e} / {S.min_schur_pivot:.3e}, "
          f"restatement {b['min_point_pivot']:.3e} / {b['min_schur_pivot']:.3e}; device_bytes {S.device_bytes}")
    assert S.termination_type == hip.SUCCESS and S.message == b"Success."
    assert [blk.shape for blk in blocks] == [(layout.size(int(p)), layout.size(int(q))) for p, q in c.pairs]
    assert all(np.all(np.isfinite(blk)) for blk in blocks)
    assert dev <= bound, (dev, bound)
    # the pivots are the restatement's to the digits a pivot of that size keeps (float64, unit-diagonal matrices)
    assert abs(S.min_point_pivot - b["min_point_pivot"]) <= 1e-9 and abs(S.min_schur_pivot - b["min_schur_pivot"]) <= 1e-9
    assert S.device_bytes >= 8 * layout.n_f ** 2 + 8 * 9 * layout.nfp   # the second n x n buffer and the point blocks at least


def test_scene_a_residual(hip, oracle):
    """The whole matrix of A-one, the group's rows and columns included, assembled from the blocks: |J^T J Cov - I|_max is at most ten
    times numpy's own figure for inv."""
    name = "A-one"
    c = SC.case(oracle, name)
    blocks, _ = device_blocks(hip, oracle, name)
    layout, J, a, _ = SC.reference_results(oracle, name)
    cov = np.full((layout.n, layout.n), np.nan)
    for (p, q), blk in zip(c.pairs, blocks):
        rp, rq = layout.columns(int(p)), layout.columns(int(q))
        if rp is not None and rq is not None:
            cov[np.ix_(rp, rq)] = blk
    assert np.all(np.isfinite(cov))   # (every entry came back)
    H = J.T @ J
    own = float(np.max(np.abs(H @ a - np.eye(layout.n))))
    dev = float(np.max(np.abs(H @ cov - np.eye(layout.n))))
    print(f"{name}: |J^T J Cov - I|_max device {dev:.3e}, numpy inv {own:.3e}")
    assert np.array_equal(cov, cov.T)
    assert dev <= 10.0 * own, (dev, own)


@pytest.mark.parametrize("name", SC.SUCCESS)
def test_structure_and_repeatability(hip, oracle, name):
    """(b, a) is the exact transpose of (a, b); a repeated pair has identical bits; pairs with a constant pose are exactly zero; a
    second call and a fresh handle give identical bits."""
    c = SC.case(oracle, name)
    layout = SC.reference_results(oracle, name)[0]
    first, _ = device_blocks(hip, oracle, name)
    seen = {}
    n_transposed = n_repeated = n_constant = 0
    for (p, q), blk in zip(c.pairs.tolist(), first):
        if (p, q) in seen:
            assert np.array_equal(seen[(p, q)], blk)
            n_repeated += 1
        if (q, p) in seen and p != q:
            assert np.array_equal(seen[(q, p)].T, blk)
            n_transposed += 1
        if p == q:
            assert np.array_equal(blk, blk.T)
        if layout.columns(p) is None or layout.columns(q) is None:
            assert not blk.any()
            n_constant += 1
        else:
            assert blk.any()
        seen[(p, q)] = blk
    assert n_transposed > 0 and n_constant > 0 and (n_repeated > 0 or name == "A-one")
    gp = c.device_problem(hip)
    try:
        x = c.state()
        again, _ = gp.covariance(x, c.pairs)
        twice, _ = gp.covariance(x, c.pairs)
    finally:
        gp.close()
    assert all(np.array_equal(u, v) for u, v in zip(first, again))    # a fresh handle
    assert all(np.array_equal(u, v) for u, v in zip(again, twice))    # a second call


def test_apply_loss_function(hip, oracle, bound):
    """apply_loss_function = 0 on the Huber handle: inside the bound against the restatement without a loss, bit-identical to a handle
    that never set a loss, different from the loss-corrected result; the handle's loss is still in force afterwards."""
    name = "C-two-huber"
    c = SC.case(oracle, name)
    x = c.state()
    with_loss, _ = device_blocks(hip, oracle, name)
    gp = c.device_problem(hip)
    try:
        cost_before = gp.evaluate(x)[0]
        off, _ = gp.covariance(x, c.pairs, apply_loss_function=False)
        assert gp.evaluate(x)[0] == cost_before
        on_again, _ = gp.covariance(x, c.pairs)
    finally:
        gp.close()
    plain = c.device_problem(hip, loss=None)
    try:
        no_loss, _ = plain.covariance(x, c.pairs)
    finally:
        plain.close()
    dev = parity(oracle, name, off, apply_loss_function=False)
    dev_plain = parity(oracle, name, no_loss, apply_loss_function=False)
    print(f"{name}: apply_loss_function = 0 against route (a) without a loss {dev:.3e}, the no-loss handle {dev_plain:.3e} (bound {bound:.3e})")
    assert dev <= bound and dev_plain <= bound
    assert all(np.array_equal(u, v) for u, v in zip(off, no_loss))   # the same kernels on the same Jacobian
    assert parity(oracle, name, with_loss, apply_loss_function=False) > 1e3 * bound   # the Huber correction is visible
    assert all(np.array_equal(u, v) for u, v in zip(with_loss, on_again))


def raw(gp, c, **kw):
    out = np.full(int(sum(gp.covariance_block_size(int(p)) * gp.covariance_block_size(int(q)) for p, q in c.pairs)), SENTINEL)
    rc, out, S = gp.covariance_raw(c.state(), c.pairs, out=out, **kw)
    return rc, out, S


@pytest.mark.parametrize("name", SC.FAILURE)
def test_a_free_gauge_fails_at_the_schur_stage(hip, oracle, name):
    """One constant pose leaves the scale free, none the whole gauge: rc 0, FAILURE, the message names the Schur complement, the output
    is not written, BalProblem.covariance raises."""
    c = SC.case(oracle, name)
    gp = c.device_problem(hip)
    try:
        rc, out, S = raw(gp, c)
        print(f"{name}: pivots {S.min_point_pivot:.3e} / {S.min_schur_pivot:.3e}: {S.message.decode()}")
        assert rc == 0 and S.termination_type == hip.FAILURE
        assert np.all(out == SENTINEL)
        msg = S.message.decode()
        assert "rank deficient" in msg and msg.startswith("The Schur complement factorization failed")
        assert S.min_point_pivot > 1e-4 and S.min_schur_pivot <= 1e-8
        with pytest.raises(hip.HipError) as e:
            gp.covariance(c.state(), c.pairs)
        assert "Schur complement factorization failed" in str(e.value)
    finally:
        gp.close()


def test_index_limits_and_the_group_invariant(hip, oracle):
    """A group index one past the last is CERES_HIP_E_INVALID; so is any index >= num_points + num_cameras on a plain handle, as before;
    a state whose group is not bit-identical is refused with the message of the evaluation, before any device call."""
    lib = hip.load_library()
    c = SC.case(oracle, "B-three")
    x = c.state()
    gp = c.device_problem(hip)
    try:
        nblocks = c.npts + c.nc + 3
        assert gp.num_covariance_blocks == nblocks
        assert [gp.covariance_block_size(b) for b in (0, c.npts, c.npts + c.nc - 1, c.npts + c.nc, nblocks - 1)] == [3, 6, 6, 3, 3]
        for bad in ([(0, nblocks)], [(nblocks, nblocks - 1)], [(-1, 0)], [(nblocks + 5, 1)]):
            out = np.full(200, SENTINEL)
            rc, out, _ = gp.covariance_raw(x, bad, out=out)
            assert rc == hip.E_INVALID and np.all(out == SENTINEL)
            assert b"out of range" in lib.ceres_hip_bal_last_error(gp._h)
        blocks, _ = gp.covariance(x, [(nblocks - 1, nblocks - 1), (nblocks - 1, 0)])   # the last group is in range
        assert blocks[0].shape == (3, 3) and blocks[1].shape == (3, 3)
        # one bit of one camera's k2: camera 4 is in group 1 with camera 1, its first
        y = x.copy()
        at = 3 * c.npts + 9 * 4 + 8
        y[at] = np.nextafter(y[at], np.inf)
        out = np.full(200, SENTINEL)
        rc, out, _ = gp.covariance_raw(y, [(0, 0), (nblocks - 1, 0)], out=out)
        msg = lib.ceres_hip_bal_last_error(gp._h).decode()
        print(msg)
        assert rc == hip.E_INVALID and np.all(out == SENTINEL)
        assert "ceres_hip_bal_covariance" in msg and "camera 4 coordinate 8 differs from camera 1, the first of group 1" in msg and MESSAGE_27_1 in msg
        again, _ = gp.covariance(x, c.pairs)   # the handle is usable afterwards
    finally:
        gp.close()
    assert all(np.array_equal(u, v) for u, v in zip(again, device_blocks(hip, oracle, c.name)[0]))
    nc, npts, cam, pt, obs, _ = c.scene
    o = hip.LinearSolverOptions(type=hip.DENSE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=100)
    plain = hip.BalProblem(o, nc, npts, cam, pt, obs)   # ceres_hip_bal_create
    try:
        assert plain.num_covariance_blocks == npts + nc and plain.covariance_block_size(npts + nc - 1) == 9
        for bad in ([(0, npts + nc)], [(npts + nc, npts + nc)], [(npts + nc + 2, 1)]):
            out = np.full(200, SENTINEL)
            rc, out, _ = plain.covariance_raw(x, bad, out=out)
            assert rc == hip.E_INVALID and np.all(out == SENTINEL)
            assert b"out of range" in lib.ceres_hip_bal_last_error(plain._h)
    finally:
        plain.close()


def test_remaining_refusals(hip, oracle):
    """An ITERATIVE_SCHUR handle with shared intrinsics answers CERES_HIP_E_UNSUPPORTED, writes nothing and stays usable."""
    lib = hip.load_library()
    c = SC.case(oracle, "A-one")
    it = c.device_problem(hip, solver_type=hip.ITERATIVE_SCHUR)
    try:
        out = np.full(200, SENTINEL)
        rc, out, _ = it.covariance_raw(c.state(), [(0, 0), (c.npts + c.nc, c.npts + c.nc)], out=out)
        assert rc == hip.E_UNSUPPORTED and np.all(out == SENTINEL)
        assert b"DENSE_SCHUR" in lib.ceres_hip_bal_last_error(it._h)
        assert it.evaluate(c.state())[0] > 0.0
    finally:
        it.close()


@pytest.mark.parametrize("layout", ["three", "one"])
def test_minimize_is_not_affected(hip, oracle, layout):
    """minimize on a fresh handle gives the same summary and state whether or not covariance ran on it first.  Three groups run the
    generic kernels (every sum in a fixed order): bit for bit.  One group runs the fused strip shapes, whose sums in LDS are not
    bitwise repeatable between two handles: flags, counts and termination exactly, costs, radii and the state to 1e-10 relative — the
    limit and the reason of test_gpu_covariance.test_minimize_is_not_affected."""
    three = SC.case(oracle, "B-three")
    c = three if layout == "three" else SC.Case("B-one", three.scene, "one", [0, 1], None, [], True)
    ng = int(c.groups.max()) + 1
    pairs = [(0, 0), (0, c.npts + 5), (c.npts + c.nc, c.npts + c.nc), (c.npts + c.nc + ng - 1, 3), (c.npts + 5, c.npts + c.nc), (1, 2)]
    x = c.state()
    runs = []
    for call_first in (False, True):
        gp = c.device_problem(hip)
        try:
            info = gp.solver_info()
            assert (info.kernel_path == hip.PATH_BAL) == (layout == "one"), info.kernel_path
            if call_first:
                gp.covariance(x, pairs)
                gp.covariance(x, pairs[:3], apply_loss_function=False)
            runs.append(gp.minimize(x, max_num_iterations=6))
        finally:
            gp.close()
    (x0, s0), (x1, s1) = runs
    generic = layout == "three"
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
            elif f in ("relative_decrease", "gradient_max_norm", "step_norm") and not generic:   # (differences of nearly equal numbers)
                assert abs(u - v) <= 1e-6 * max(abs(u), 1.0), (i, f, u, v)
            else:
                assert same(u, v), (i, f, u, v)
    print(f"{layout}: largest state difference {np.max(np.abs(x0 - x1)):.3e}, final costs {s0.final_cost!r} {s1.final_cost!r}")
    assert np.all(np.abs(x0 - x1) <= rtol * (1.0 + np.abs(x0)))
    assert s0.final_cost < s0.initial_cost


# ---- poison ---------------------------------------------------------------------------------------------------------------------------
POISON_CASES = ("B-each", "C-two-huber")


def child_main():
    """In the child interpreter (CERES_HIP_DEBUG_POISON=nan): every poison case on a fresh handle; one JSON line each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hip = pkg.hip_solver
    hip.load_library()
    for name in POISON_CASES:
        c = SC.case(oracle, name)
        gp = c.device_problem(hip)
        try:
            blocks, S = gp.covariance(c.state(), c.pairs)
        finally:
            gp.close()
        print(json.dumps(dict(name=name, blocks=[b.tolist() for b in blocks], termination=S.termination_type)), flush=True)
    return 0


def test_poisoned_allocations_do_not_reach_the_blocks(hip, oracle, bound):
    """CERES_HIP_DEBUG_POISON=nan (read once per process: a child interpreter) fills every new floating-point device buffer with NaN:
    the second n x n buffer, the point blocks, the lists' neighbours and the output must be written before they are read — finite, inside
    the bound, and the bits of a run without poison."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_shared_covariance as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr
    got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [g["name"] for g in got] == list(POISON_CASES)
    for g in got:
        blocks = [np.array(b) for b in g["blocks"]]
        assert g["termination"] == hip.SUCCESS
        assert all(np.all(np.isfinite(blk)) for blk in blocks)
        dev = parity(oracle, g["name"], blocks)
        print(f"{g['name']} under poison: {dev:.3e} (bound {bound:.3e})")
        assert dev <= bound
        assert all(np.array_equal(u, v) for u, v in zip(blocks, device_blocks(hip, oracle, g["name"])[0]))
