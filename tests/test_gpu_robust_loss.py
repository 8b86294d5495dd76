"""Robust losses in the BAL front end (ceres_hip_bal_set_loss): the device evaluator and ceres_hip_bal_minimize against the numpy
restatement of the losses, the Corrector and the trust-region loop (tests/robust_reference.py, Jacobians from the oracle's dual
numbers).  Ceres applies the loss in the Evaluator, before the linear solver sees J (internal/ceres/residual_block.cc:161-195)."""
import numpy as np
import pytest

import robust_reference as R
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

# parameters that put observations of the scenes below on every branch: Huber / Tukey both sides of a^2, Tolerant both sides of
# x = (s - a) / b = 36.7 (outliers of 30+ px are beyond it), the exact hits at s = 0
LOSS_CASES = [("trivial", 1.0, 1.0), ("huber", 2.0, 1.0), ("soft_l_one", 2.0, 1.0), ("cauchy", 2.0, 1.0), ("arctan", 3.0, 1.0),
              ("tolerant", 4.0, 1.0), ("tukey", 10.0, 1.0)]


def outlier_scene(oracle, nc, npts, nobs, seed, frac=0.1, lo=30.0, hi=300.0, hits=True):
    """A synthetic BAL problem with `frac` of its observations displaced by lo .. hi pixels in random directions and (hits) a few
    observations that the initial state reproduces exactly (s = 0: a camera with zero rotation and translation (0, 0, t_z) and a point on
    its axis, observed at the image centre).  Returns (num_cameras, num_points, cam, pt, clean obs, obs, x0, outlier mask)."""
    op = oracle.BalProblem.generate(nc, npts, nobs, seed=seed)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x0 = op.state()
    rng = np.random.default_rng(seed + 1000)
    k = int(frac * cam.shape[0])
    out = np.zeros(cam.shape[0], bool)
    out[rng.choice(cam.shape[0], k, replace=False)] = True
    ang, mag = rng.uniform(0.0, 2.0 * np.pi, k), rng.uniform(lo, hi, k)
    obs2 = obs.copy()
    obs2[out, 0] += mag * np.cos(ang)
    obs2[out, 1] += mag * np.sin(ang)
    if hits:
        i0 = int(np.flatnonzero(~out)[0])
        c0, p0 = int(cam[i0]), int(pt[i0])
        cb = 3 * op.num_points + 9 * c0
        x0[cb:cb + 5] = 0.0                                   # angle-axis and t_x, t_y
        x0[3 * p0:3 * p0 + 3] = [0.0, 0.0, -5.0 - x0[cb + 5]]  # on the camera's axis, in front of it
        obs2[(cam == c0) & (pt == p0)] = 0.0
    return op.num_cameras, op.num_points, cam, pt, obs, obs2, x0, out


def device_problem(hip, nc, npts, cam, pt, obs, solver_type=5, pre=2, max_it=500):
    o = hip.LinearSolverOptions(type=solver_type, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=max_it)
    return hip.BalProblem(o, nc, npts, cam, pt, obs)


@pytest.fixture(scope="module")
def eval_scene(oracle):
    return outlier_scene(oracle, 12, 700, 4000, seed=21)


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("kind,a,b", LOSS_CASES)
def test_evaluate_matches_the_reference(hip, oracle, eval_scene, kind, a, b, scale):
    nc, npts, cam, pt, _, obs, x0, _ = eval_scene
    gp = device_problem(hip, nc, npts, cam, pt, obs)
    order = gp.row_order()
    assert np.array_equal(order, np.argsort(pt, kind="stable"))
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, order, loss=(kind, a, b, scale))
    cost_o, res_o, vals_o, g_o, g_plain = ev.evaluate(x0, corrector_free_gradient=True)
    s = np.sum(ev._blocks(x0)[0] ** 2, axis=1)
    assert np.any(s == 0.0) and np.any(np.sqrt(s) > 30.0)   # exact hits and gross outliers are in the scene
    gp.set_loss(kind, a, b, scale)
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    for v in (res, grad, vals):
        assert np.all(np.isfinite(v))
    assert np.isfinite(cost)
    assert abs(cost - cost_o) <= 1e-12 * abs(cost_o), (cost, cost_o)
    assert rel(res, res_o) <= 1e-12
    assert rel(vals, vals_o) <= 1e-12
    assert rel(grad, g_o) <= 1e-12
    assert rel(grad, g_plain) <= 1e-12        # J~^T r~ = sum rho' J^T r
    if kind == "tukey":                      # beyond the cut-off the blocks vanish
        far = np.flatnonzero(s > a * a)
        assert far.size and np.all(res.reshape(-1, 2)[far] == 0.0)
    # cost only (the candidate's evaluation in the loop): the same cost
    c2, r2, _, _ = gp.evaluate(x0)
    assert c2 == cost and r2 is None
    # the loss stays in force until set again
    assert gp.evaluate(x0)[0] == cost
    gp.close()


def test_trivial_loss_is_bit_for_bit_the_squared_loss(hip, oracle):
    """set_loss("trivial") (scale 1), and Huber then Trivial again, evaluate exactly what a problem that never set a loss evaluates:
    cost, residuals and Jacobian bit for bit.  The gradient and the loop go through the camera sums of J^T r, which the fused kernels
    accumulate with LDS atomics (kernels_bal.inc: their order is not fixed), so two runs of the squared loss alone differ in the last
    bits there: those are held to the agreement two such runs show, and the loop's initial cost — an evaluation — bit for bit."""
    nc, npts, cam, pt, _, obs, x0, _ = outlier_scene(oracle, 12, 800, 3600, seed=5, frac=0.05, lo=30.0, hi=100.0, hits=False)
    gp = device_problem(hip, nc, npts, cam, pt, obs)

    def run():
        e = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
        x, S = gp.minimize(x0, max_num_iterations=6)
        return e, x, S

    def same(u, v):
        (eu, xu, Su), (ev, xv, Sv) = u, v
        assert eu[0] == ev[0], (eu[0], ev[0])
        assert np.array_equal(eu[1], ev[1]) and np.array_equal(eu[3], ev[3])   # residuals, Jacobian values
        assert rel(eu[2], ev[2]) <= 1e-14                                     # gradient
        assert Su.initial_cost == Sv.initial_cost
        assert Su.num_iterations_logged == Sv.num_iterations_logged
        for i in range(Su.num_iterations_logged):
            a, b = Su.iterations[i], Sv.iterations[i]
            assert (a.step_is_successful, a.step_is_valid, a.linear_solver_iterations) == (b.step_is_successful, b.step_is_valid, b.linear_solver_iterations), i
            assert abs(a.cost - b.cost) <= 1e-12 * a.cost, i
        assert rel(xu, xv) <= 1e-10 and Su.termination_type == Sv.termination_type

    base = run()
    same(base, run())
    gp.set_loss("trivial")
    same(base, run())
    gp.set_loss("huber", 1.0)
    huber = run()
    assert huber[0][0] < base[0][0]
    assert huber[2].initial_cost == pytest.approx(huber[0][0], rel=1e-14)   # (the loop's evaluator sums in tile order)
    gp.set_loss("trivial", scale=1.0)
    same(base, run())
    gp.close()


@pytest.mark.parametrize("solver_type,pre", [(5, 2), (6, 1), (3, 0)])
@pytest.mark.parametrize("kind,a,b", [("huber", 1.0, 1.0), ("cauchy", 1.0, 1.0), ("tolerant", 4.0, 1.0)])
def test_minimize_follows_the_reference_loop(hip, oracle, solver_type, pre, kind, a, b):
    """ITERATIVE_SCHUR + SCHUR_JACOBI, CGNR + JACOBI and DENSE_SCHUR, eta small enough that CG is exact for this purpose, against the
    reference loop with a dense solve.  (Tolerant(4, 1) rejects steps on this scene: the rejection path is covered.)  Costs agree to
    1e-8 where the Schur complement is solved; CGNR's 500 Jacobi-preconditioned iterations on the normal equations of this scene stop
    short of the exact step (1e-6, the tolerance of test_gpu_bal_frontend.py's oracle loop), and Tolerant(4, 1) — most weight on the
    gross residuals, inliers nearly switched off — is the least well conditioned of the three (ten times looser)."""
    nc, npts, cam, pt, _, obs, x0, _ = outlier_scene(oracle, 10, 200, 1200, seed=5, frac=0.05, lo=30.0, hi=100.0, hits=False)
    gp = device_problem(hip, nc, npts, cam, pt, obs, solver_type, pre)
    gp.set_loss(kind, a, b)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order(), loss=(kind, a, b, 1.0))
    n_it = 8
    cost_tol = (1e-6 if solver_type == hip.CGNR else 1e-8) * (10.0 if kind == "tolerant" else 1.0)
    xr, Sr = R.minimize(ev, x0, max_num_iterations=n_it)
    x, S = gp.minimize(x0, max_num_iterations=n_it, eta=1e-12)
    assert S.initial_cost == pytest.approx(Sr["initial_cost"], rel=1e-12)
    its = Sr["iterations"]
    assert S.num_iterations_logged == len(its) >= 7
    for i, it in enumerate(its):
        d = S.iterations[i]
        assert (d.step_is_successful, d.step_is_valid) == (it["step_is_successful"], it["step_is_valid"]), i
        assert abs(d.cost - it["cost"]) <= cost_tol * abs(it["cost"]), (i, d.cost, it["cost"])
    assert S.termination_type == Sr["termination_type"]
    assert S.final_cost == pytest.approx(Sr["final_cost"], rel=cost_tol)
    assert gp.evaluate(x)[0] == pytest.approx(S.final_cost, rel=1e-12)   # the returned state is the one whose cost is reported
    assert rel(x, xr) <= 100.0 * cost_tol
    gp.close()


@pytest.mark.parametrize("solver_type,pre,shape", [(5, 2, (12, 800, 3600)), (6, 1, (12, 800, 3600)), (5, 2, (2600, 1500, 9000)), (5, 2, (100, 30, 2400))])
def test_evaluator_forms_agree_with_a_loss(hip, oracle, monkeypatch, solver_type, pre, shape):
    """CERES_HIP_EVAL_TILES = 1 / 2 / 3 / 0 (tiles from the evaluator; the camera-major pass evaluating its F cells or reading them; the
    two-pass form) on the shapes test_gpu_bal_frontend.py::test_evaluator_writing_the_tiles_is_the_two_pass_form uses, with a Huber loss:
    every kernel that produces Jacobian values corrects them the same way."""
    nc, npts, nobs = shape
    nc, npts, cam, pt, _, obs, x0, _ = outlier_scene(oracle, nc, npts, nobs, seed=5, frac=0.05, lo=30.0, hi=100.0, hits=False)
    gp = device_problem(hip, nc, npts, cam, pt, obs, solver_type, pre)
    assert gp.solver_info().kernel_path == hip.PATH_BAL
    gp.set_loss("huber", 1.0)
    runs, blocks = {}, {}
    for form in ("1", "2", "3", "0"):
        monkeypatch.setenv("CERES_HIP_EVAL_TILES", form)
        gp.minimize(x0, max_num_iterations=0)
        if solver_type == hip.ITERATIVE_SCHUR:
            blocks[form] = gp.preconditioner_blocks(not_inverted=True)
        runs[form] = gp.minimize(x0, max_num_iterations=6)
    if blocks:
        for form in ("1", "2", "3"):
            assert rel(blocks[form], blocks["0"]) <= 1e-13, form
    xb, Sb = runs["0"]
    for form in ("1", "2", "3"):
        xa, Sa = runs[form]
        assert Sa.num_iterations_logged == Sb.num_iterations_logged and Sa.num_iterations_logged >= 4
        for i in range(Sa.num_iterations_logged):
            a, b = Sa.iterations[i], Sb.iterations[i]
            assert (a.step_is_successful, a.step_is_valid) == (b.step_is_successful, b.step_is_valid), (form, i)
            assert a.linear_solver_iterations == b.linear_solver_iterations, (form, i)
            assert abs(a.cost - b.cost) <= 1e-9 * abs(a.cost) and abs(a.gradient_max_norm - b.gradient_max_norm) <= 1e-7 * abs(a.gradient_max_norm), (form, i)
        assert rel(xa, xb) <= 1e-7, form
    # the loop's costs are the robust ones: 1/2 sum rho at the returned state
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order(), loss=("huber", 1.0, 1.0, 1.0))
    assert Sb.final_cost == pytest.approx(ev.cost(xb), rel=1e-12)
    assert Sb.initial_cost == pytest.approx(ev.cost(x0), rel=1e-12)
    gp.close()


def test_robust_losses_resist_outliers(hip, oracle):
    """About 5 % of the observations 30-100 px off: from the same start, Huber(1) and Cauchy(1) reach a far lower reprojection RMS over
    the inliers (against the clean pixels) than the squared loss.  Reference loop, this scene, 20 iterations: squared 6.1-6.4 px,
    Huber 1.6-2.0, Cauchy 0.60 (seeds 5, 6) — the thresholds below are half and a quarter of the squared loss's RMS."""
    nc, npts, cam, pt, clean, obs, x0, out = outlier_scene(oracle, 10, 200, 1200, seed=6, frac=0.05, lo=30.0, hi=100.0, hits=False)
    gp = device_problem(hip, nc, npts, cam, pt, obs)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, clean, np.arange(cam.shape[0]))

    def inlier_rms(x):
        r = ev._blocks(x)[0]
        return float(np.sqrt(np.mean(np.sum(r[~out] ** 2, axis=1))))

    rms = {}
    for kind in ("trivial", "huber", "cauchy"):
        gp.set_loss(kind, 1.0)
        x, S = gp.minimize(x0, max_num_iterations=20)
        assert S.termination_type != hip.MINIMIZER_FAILURE
        rms[kind] = inlier_rms(x)
    print("inlier RMS", rms)
    assert rms["huber"] < 0.5 * rms["trivial"]
    assert rms["cauchy"] < 0.25 * rms["trivial"]
    gp.close()


def test_invalid_losses_are_rejected(hip, oracle):
    nc, npts, cam, pt, _, obs, x0, _ = outlier_scene(oracle, 6, 80, 400, seed=3, hits=False)
    gp = device_problem(hip, nc, npts, cam, pt, obs)
    cost0 = gp.evaluate(x0)[0]
    nan, inf = float("nan"), float("inf")
    bad = [(7, 1.0, 1.0, 1.0, "loss_type"), (-1, 1.0, 1.0, 1.0, "loss_type")]
    for kind in ("huber", "soft_l_one", "cauchy", "arctan", "tukey"):
        bad += [(kind, 0.0, 1.0, 1.0, "a"), (kind, -1.0, 1.0, 1.0, "a"), (kind, nan, 1.0, 1.0, "a"), (kind, inf, 1.0, 1.0, "a")]
    bad += [("tolerant", -1.0, 1.0, 1.0, "a"), ("tolerant", nan, 1.0, 1.0, "a"), ("tolerant", 1.0, 0.0, 1.0, "b"),
            ("tolerant", 1.0, -2.0, 1.0, "b"), ("tolerant", 1.0, inf, 1.0, "b")]
    for kind in ("trivial", "huber", "tolerant"):
        bad += [(kind, 1.0, 1.0, 0.0, "scale"), (kind, 1.0, 1.0, -1.0, "scale"), (kind, 1.0, 1.0, nan, "scale"), (kind, 1.0, 1.0, inf, "scale")]
    for kind, a, b, scale, name in bad:
        with pytest.raises(hip.HipError, match=rf"\b{name}\b"):
            gp.set_loss(kind, a, b, scale)
    with pytest.raises(ValueError, match="kind"):
        gp.set_loss("l1")
    # a rejected call leaves the loss in force as it was (here: none)
    assert gp.evaluate(x0)[0] == cost0
    gp.set_loss("tolerant", 0.0, 1.0)   # a = 0 is allowed for Tolerant
    # the C entry point with a NULL handle
    lib = hip.load_library()
    assert lib.ceres_hip_bal_set_loss(None, 1, 1.0, 1.0, 1.0) == -1
    assert b"NULL" in lib.ceres_hip_bal_last_error(None)
    gp.close()
