"""Inner iterations in the BAL front end (ceres_hip_bal_set_inner_iterations / ceres_hip_bal_inner_iterate, and ceres_hip_bal_minimize
with them set) against the numpy restatement of CoordinateDescentMinimizer and DoInnerIterationsIfNeeded (tests/inner_reference.py)."""
import numpy as np
import pytest

import inner_reference as IR
import robust_reference as R
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

LOSSES = [None, ("huber", 1.0, 1.0, 1.0), ("cauchy", 1.0, 1.0, 1.0)]


def scene(oracle, seed=11):
    """100 cameras, 120 points, 6000 observations (points of more than 64 observations: the wave form), then the first 8 points cut
    down to one observation each (a rank-deficient J^T J that LM's D regularises), 5 % of the pixels 5-30 px off."""
    op = oracle.BalProblem.generate(100, 120, 6000, seed=seed)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    keep = np.ones(cam.shape[0], bool)
    for q in range(8):
        idx = np.flatnonzero(pt == q)
        keep[idx[1:]] = False
    cam, pt, obs = cam[keep], pt[keep], obs[keep].copy()
    rng = np.random.default_rng(seed)
    out = rng.random(cam.shape[0]) < 0.05
    ang, mag = rng.uniform(0, 2 * np.pi, out.sum()), rng.uniform(5.0, 30.0, out.sum())
    obs[out, 0] += mag * np.cos(ang)
    obs[out, 1] += mag * np.sin(ang)
    counts = np.bincount(pt, minlength=op.num_points)
    assert counts.max() > 64 and np.sum(counts == 1) == 8
    return op.num_cameras, op.num_points, cam, pt, obs, op.state()


def problem(hip, nc, npts, cam, pt, obs, solver_type=5, pre=2, generic=False):
    o = hip.LinearSolverOptions(type=solver_type, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=500,
                                force_generic_path=generic)
    return hip.BalProblem(o, nc, npts, cam, pt, obs)


@pytest.fixture(scope="module")
def inner_scene(oracle):
    return scene(oracle)


@pytest.mark.parametrize("loss", LOSSES, ids=["squared", "huber", "cauchy"])
@pytest.mark.parametrize("blocks", IR.KINDS)
def test_one_pass_matches_the_restatement(hip, oracle, inner_scene, blocks, loss):
    nc, npts, cam, pt, obs, x0 = inner_scene
    gp = problem(hip, nc, npts, cam, pt, obs)
    if loss:
        gp.set_loss(loss[0], loss[1], loss[2], loss[3])
    gp.set_inner_iterations(blocks)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order(), loss=loss)
    group, ng = IR.ordering(nc, npts, cam, pt, blocks)
    xr, itr = IR.one_pass(ev, x0, group, ng)
    x, c0, c1, its = gp.inner_iterate(x0)
    assert c0 == pytest.approx(ev.cost(x0), rel=1e-12)
    assert c1 <= c0
    assert abs(c1 - ev.cost(xr)) <= 1e-10 * c1, (c1, ev.cost(xr))
    blk = [x[:3 * npts].reshape(-1, 3), x[3 * npts:].reshape(-1, 9)]
    ref = [xr[:3 * npts].reshape(-1, 3), xr[3 * npts:].reshape(-1, 9)]
    err = np.concatenate([np.abs(b - r).max(axis=1) / np.maximum(np.abs(r).max(axis=1), 1e-300) for b, r in zip(blk, ref)])
    assert err.max() <= 1e-9, err.max()
    assert np.array_equal(its < 0, itr < 0)
    differ = int(np.sum(its != itr))
    print(f"{blocks} {loss}: iterations differ on {differ} of {its.size} blocks; mean {its[its >= 0].mean():.2f}")
    assert differ <= max(3, its.size // 50)
    gp.close()


def test_pass_is_deterministic_and_forms_agree(hip, inner_scene, monkeypatch):
    nc, npts, cam, pt, obs, x0 = inner_scene
    gp = problem(hip, nc, npts, cam, pt, obs)
    gp.set_loss("huber", 1.0)
    gp.set_inner_iterations("automatic")
    a = gp.inner_iterate(x0)
    b = gp.inner_iterate(x0)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    for form in ("lane", "wave"):   # every point in one kernel form
        monkeypatch.setenv("CERES_HIP_INNER_FORM", form)
        f = gp.inner_iterate(x0)
        assert rel(f[0], a[0]) <= 1e-12, form
        assert f[2] == pytest.approx(a[2], rel=1e-12)
    gp.close()


@pytest.mark.parametrize("solver_type,pre", [(5, 2), (6, 1), (3, 0)])
def test_minimize_with_inner_iterations_follows_the_restatement(hip, oracle, solver_type, pre):
    """ITERATIVE_SCHUR + SCHUR_JACOBI, CGNR + JACOBI, DENSE_SCHUR (eta 1e-12) against the dense reference loop with the inner pass."""
    op = oracle.BalProblem.generate(10, 200, 1200, seed=5)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x0 = op.state()
    gp = problem(hip, op.num_cameras, op.num_points, cam, pt, obs, solver_type, pre)
    gp.set_loss("huber", 1.0)
    ev = R.Evaluator(oracle.snavely_batch, op.num_cameras, op.num_points, cam, pt, obs, gp.row_order(), loss=("huber", 1.0, 1.0, 1.0))
    group, ng = IR.ordering(op.num_cameras, op.num_points, cam, pt, "automatic")
    cost_tol = 1e-6 if solver_type == hip.CGNR else 1e-8
    for tol in (1e-3, 0.2):   # 0.2: the tolerance switches the pass off part-way
        gp.set_inner_iterations("automatic", tol)
        xr, Sr = IR.minimize(ev, x0, group, ng, inner_iteration_tolerance=tol, max_num_iterations=8)
        x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
        steps, secs, groups = gp.inner_iteration_stats()
        assert groups == ng == 2 and secs > 0.0
        assert steps == Sr["num_inner_iteration_steps"] >= 1, (steps, Sr["num_inner_iteration_steps"])
        its = Sr["iterations"]
        assert S.num_iterations_logged == len(its)
        for i, it in enumerate(its):
            d = S.iterations[i]
            assert (d.step_is_successful, d.step_is_valid) == (it["step_is_successful"], it["step_is_valid"]), i
            assert abs(d.cost - it["cost"]) <= cost_tol * abs(it["cost"]), (i, d.cost, it["cost"])
        assert S.termination_type == Sr["termination_type"]
        assert S.final_cost == pytest.approx(Sr["final_cost"], rel=cost_tol)
        assert rel(x, xr) <= 100.0 * cost_tol
        if tol == 0.2:
            assert not Sr["inner_enabled_at_end"] and steps < len(its) - 1
    gp.close()


def test_useful_inner_iterations_accept_a_poor_step(hip, oracle):
    """inner_iterations_were_useful accepts a step whose relative decrease is at most min_relative_decrease.  Constructed: a start
    further off (parameter noise 0.1) and min_relative_decrease = 0.999; the restatement's second step has a relative decrease of
    0.997 and is accepted because the inner pass was useful."""
    op = oracle.BalProblem.generate(10, 200, 1200, seed=6, param_noise=0.1)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x0 = op.state()
    gp = problem(hip, op.num_cameras, op.num_points, cam, pt, obs)
    gp.set_inner_iterations("automatic", 0.0)
    ev = R.Evaluator(oracle.snavely_batch, op.num_cameras, op.num_points, cam, pt, obs, gp.row_order())
    group, ng = IR.ordering(op.num_cameras, op.num_points, cam, pt, "automatic")
    xr, Sr = IR.minimize(ev, x0, group, ng, inner_iteration_tolerance=0.0, max_num_iterations=6, min_relative_decrease=0.999)
    poor = [it for it in Sr["iterations"][1:] if it.get("inner_useful") and it.get("relative_decrease", 1.0) <= 0.999 and it["step_is_successful"]]
    assert poor, "no step accepted only through the inner iterations"
    x, S = gp.minimize(x0, max_num_iterations=6, min_relative_decrease=0.999, eta=1e-12)
    assert S.num_iterations_logged == len(Sr["iterations"])
    for i, it in enumerate(Sr["iterations"]):
        assert S.iterations[i].step_is_successful == it["step_is_successful"], i
    assert S.final_cost == pytest.approx(Sr["final_cost"], rel=1e-8)
    gp.close()


def test_without_inner_iterations_nothing_changes(hip, oracle):
    op = oracle.BalProblem.generate(12, 800, 3600, seed=5)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x0 = op.state()
    runs = []
    for setting in ("never", "none", "automatic-then-none"):
        gp = problem(hip, op.num_cameras, op.num_points, cam, pt, obs)
        if setting == "none":
            gp.set_inner_iterations(None)
        elif setting == "automatic-then-none":
            gp.set_inner_iterations("automatic")
            gp.minimize(x0, max_num_iterations=2)
            gp.set_inner_iterations(None)
        runs.append(gp.minimize(x0, max_num_iterations=6) + (gp.inner_iteration_stats(),))
        gp.close()
    (xb, Sb, stb) = runs[0]
    assert stb == (0, 0.0, 0)
    for x, S, stats in runs[1:]:
        assert stats == (0, 0.0, 0)
        assert S.initial_cost == Sb.initial_cost and S.num_iterations_logged == Sb.num_iterations_logged
        for i in range(S.num_iterations_logged):
            a, b = S.iterations[i], Sb.iterations[i]
            assert (a.step_is_successful, a.step_is_valid, a.linear_solver_iterations) == (b.step_is_successful, b.step_is_valid, b.linear_solver_iterations)
            assert abs(a.cost - b.cost) <= 1e-12 * a.cost and a.step_norm == pytest.approx(b.step_norm, rel=1e-10)
        assert rel(x, xb) <= 1e-10 and S.termination_type == Sb.termination_type


def test_quality_and_both_paths(hip, inner_scene):
    """minimize with AUTOMATIC reaches no higher a cost than without, on the fused <2,3,9> path and the generic one (whose camera-major
    list the inner pass builds itself); both paths agree."""
    nc, npts, cam, pt, obs, x0 = inner_scene
    finals = {}
    for generic in (False, True):
        gp = problem(hip, nc, npts, cam, pt, obs, generic=generic)
        assert (gp.solver_info().kernel_path == hip.PATH_BAL) != generic
        _, S0 = gp.minimize(x0, max_num_iterations=5)
        gp.set_inner_iterations("automatic")
        x1, S1 = gp.minimize(x0, max_num_iterations=5)
        assert S1.final_cost <= S0.final_cost, (S1.final_cost, S0.final_cost)
        finals[generic] = (x1, S1.final_cost, gp.inner_iterate(x0)[0])
        gp.close()
    assert finals[False][1] == pytest.approx(finals[True][1], rel=1e-8)
    assert rel(finals[False][2], finals[True][2]) <= 1e-12


def test_argument_validation_on_a_live_handle(hip, inner_scene):
    nc, npts, cam, pt, obs, x0 = inner_scene
    gp = problem(hip, nc, npts, cam, pt, obs)
    with pytest.raises(hip.HipError, match="no inner iterations"):
        gp.inner_iterate(x0)
    for blocks, tol, name in ((6, 1e-3, "blocks"), (-1, 1e-3, "blocks"), (1, -1.0, "tolerance"), (1, float("nan"), "tolerance"),
                              (1, float("inf"), "tolerance")):
        with pytest.raises(hip.HipError, match=rf"\b{name}\b"):
            gp.set_inner_iterations(blocks, tol)
    with pytest.raises(ValueError):
        gp.set_inner_iterations("everything")
    gp.set_inner_iterations("points", 0.0)
    x, c0, c1, its = gp.inner_iterate(x0)
    assert np.all(its[npts:] == -1) and np.all(its[:npts] >= 0) and c1 <= c0
    assert np.array_equal(x[3 * npts:], x0[3 * npts:])   # cameras untouched
    lib = hip.load_library()
    assert lib.ceres_hip_bal_inner_iterate(gp._h, None, None, None, None) == -1
    gp.close()
