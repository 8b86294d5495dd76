"""The dogleg trust region of the BAL front end (ceres_hip_bal_set_trust_region_strategy, ceres_hip_op_jacobian_gram) against the numpy
restatement of DoglegStrategy inside TrustRegionMinimizer (tests/dogleg_reference.py)."""
import numpy as np
import pytest

import dogleg_reference as DR
import inner_reference as IR
import robust_reference as R
from test_gpu_inner_iterations import problem, scene
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

LOSSES = [None, ("huber", 1.0, 1.0, 1.0), ("cauchy", 1.0, 1.0, 1.0)]
DENSE_SCHUR = 3


@pytest.fixture(scope="module")
def outlier_scene(oracle):
    return scene(oracle)


def clean_scene(oracle, seed=5, **kw):
    op = oracle.BalProblem.generate(10, 200, 1200, seed=seed, **kw)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    return op.num_cameras, op.num_points, cam, pt, obs, op.state()


def dogleg_problem(hip, sc, kind, loss=None, generic=False):
    nc, npts, cam, pt, obs, _ = sc
    gp = problem(hip, nc, npts, cam, pt, obs, DENSE_SCHUR, 2, generic)
    if loss:
        gp.set_loss(*loss)
    gp.set_trust_region_strategy("dogleg", kind)
    return gp


def follows(S, Sr, cost_tol=1e-6):
    """Iteration by iteration: flags, cost, radius, and whether a linear solve ran; then the totals.  The Gauss-Newton solve at mu = 1e-8
    is ill-conditioned along the gauge of every BAL problem (the 7 directions of a similarity transform, where J^T J is singular): the
    last digits of the Schur solve come back amplified ~1e8 there, so two GPU runs, or the GPU and the dense restatement, agree in the
    first step's cost to ~1e-7 only.  Costs to cost_tol, radii (3 x the step norm after a good step) to 100 cost_tol."""
    its = Sr["iterations"]
    assert S.num_iterations_logged == len(its)
    for i, it in enumerate(its):
        d = S.iterations[i]
        assert (d.step_is_successful, d.step_is_valid) == (it["step_is_successful"], it["step_is_valid"]), (i, it.get("branch"))
        assert abs(d.cost - it["cost"]) <= cost_tol * abs(it["cost"]), (i, d.cost, it["cost"], it.get("branch"))
        assert d.trust_region_radius == pytest.approx(it["trust_region_radius"], rel=100 * cost_tol), (i, it.get("branch"))
        if i > 0:
            assert (d.linear_solver_iterations == 0) == (it["linear_solver_iterations"] == 0), (i, it.get("branch"))
    assert S.termination_type == Sr["termination_type"]
    assert S.num_linear_solves == Sr["num_linear_solves"]
    assert S.final_cost == pytest.approx(Sr["final_cost"], rel=cost_tol)


def test_jacobian_gram_matches_numpy(hip, oracle, outlier_scene):
    nc, npts, cam, pt, obs, x0 = outlier_scene
    rng = np.random.default_rng(3)
    for solver_type, generic in ((DENSE_SCHUR, False), (5, False), (DENSE_SCHUR, True)):
        gp = problem(hip, nc, npts, cam, pt, obs, solver_type, 2, generic)
        assert (gp.solver_info().kernel_path == hip.PATH_GENERIC) == generic
        gp.evaluate(x0, jacobian=True)   # leaves J and f loaded in the linear solver
        ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order())
        _, r, vals, _ = ev.evaluate(x0)
        J = ev.dense_jacobian(vals)
        a, b = rng.standard_normal(ev.n), rng.standard_normal(ev.n)
        out = np.full(5, np.nan)
        lib = hip.load_library()
        s = lib.ceres_hip_bal_linear_solver(gp._h)
        assert lib.ceres_hip_op_jacobian_gram(s, a.ctypes.data_as(hip._DP), b.ctypes.data_as(hip._DP), out.ctypes.data_as(hip._DP)) == 0
        ja, jb = J @ a, J @ b
        want = [ja @ ja, ja @ jb, jb @ jb, ja @ r, jb @ r]
        scales = [ja @ ja, np.linalg.norm(ja) * np.linalg.norm(jb), jb @ jb, np.linalg.norm(ja) * np.linalg.norm(r),
                  np.linalg.norm(jb) * np.linalg.norm(r)]
        for k in range(5):
            assert abs(out[k] - want[k]) <= 1e-13 * scales[k], (solver_type, generic, k, out[k], want[k])
        gp.close()


@pytest.mark.parametrize("loss", LOSSES, ids=["squared", "huber", "cauchy"])
@pytest.mark.parametrize("kind", ["traditional", "subspace"])
def test_minimize_follows_the_restatement(hip, oracle, outlier_scene, kind, loss):
    """The outlier scene's single-observation points add to the gauge's singular directions of J^T J (see follows)."""
    nc, npts, cam, pt, obs, x0 = outlier_scene
    gp = dogleg_problem(hip, outlier_scene, kind, loss)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order(), loss=loss)
    xr, Sr = DR.minimize(ev, x0, kind, max_num_iterations=8)
    x, S = gp.minimize(x0, max_num_iterations=8)
    follows(S, Sr, cost_tol=1e-5)
    assert rel(x, xr) <= 1e-3
    gp.close()


@pytest.mark.parametrize("kind", ["traditional", "subspace"])
def test_branches_and_reused_steps_on_a_clean_scene(hip, oracle, kind):
    """Initial radii chosen so that the traditional step's three branches all occur (asserted from the restatement's record), and
    rejected steps (a start further off and min_relative_decrease = 0.99999) whose successors reuse the Gauss-Newton step and the Cauchy
    point: no solve, 0 linear-solver iterations, num_linear_solves as the restatement counts them."""
    sc = clean_scene(oracle, seed=6, param_noise=0.3)
    nc, npts, cam, pt, obs, x0 = sc
    gp = dogleg_problem(hip, sc, kind)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order())
    branches, reused = set(), 0
    for radius, mrd in ((10.0, 1e-3), (1e2, 1e-3), (1e4, 1e-3), (1e4, 0.99999)):
        xr, Sr = DR.minimize(ev, x0, kind, max_num_iterations=10, initial_trust_region_radius=radius, min_relative_decrease=mrd)
        x, S = gp.minimize(x0, max_num_iterations=10, initial_trust_region_radius=radius, min_relative_decrease=mrd)
        follows(S, Sr)
        assert rel(x, xr) <= 1e-3
        for i, it in enumerate(Sr["iterations"][1:], 1):
            branches.add(it["branch"].split(":")[-1])
            if it["solves"] == 0 and it["step_is_valid"]:
                reused += 1
                assert S.iterations[i].linear_solver_iterations == 0
    assert reused >= 1, branches
    if kind == "traditional":
        assert {"gauss_newton", "cauchy"} <= branches and any(b.startswith("dogleg_c") for b in branches), branches
    else:
        assert "subspace_boundary" in branches, branches
    gp.close()


def test_dogleg_with_inner_iterations(hip, oracle):
    sc = clean_scene(oracle, seed=6)
    nc, npts, cam, pt, obs, x0 = sc
    gp = dogleg_problem(hip, sc, "subspace", ("huber", 1.0, 1.0, 1.0))
    gp.set_inner_iterations("automatic", 1e-3)
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, obs, gp.row_order(), loss=("huber", 1.0, 1.0, 1.0))
    group, ng = IR.ordering(nc, npts, cam, pt, "automatic")
    xr, Sr = DR.minimize(ev, x0, "subspace", inner=(group, ng), max_num_iterations=6)
    x, S = gp.minimize(x0, max_num_iterations=6)
    follows(S, Sr)
    assert gp.inner_iteration_stats()[0] >= 1
    gp.close()


def test_deterministic_and_fused_generic_agree(hip, oracle, outlier_scene):
    """The dogleg pass is bit-for-bit repeatable.  Whole minimize runs agree as far as the Gauss-Newton solve lets them (see follows):
    the DENSE_SCHUR solve inside is not bitwise repeatable (its camera sums), and the fused and generic paths form S differently."""
    nc, npts, cam, pt, obs, x0 = outlier_scene
    gp = problem(hip, nc, npts, cam, pt, obs, DENSE_SCHUR, 2)
    gp.evaluate(x0, jacobian=True)
    lib = hip.load_library()
    s = lib.ceres_hip_bal_linear_solver(gp._h)
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal(gp.num_parameters), rng.standard_normal(gp.num_parameters)
    outs = [np.full(5, np.nan) for _ in range(2)]
    for o in outs:
        assert lib.ceres_hip_op_jacobian_gram(s, a.ctypes.data_as(hip._DP), b.ctypes.data_as(hip._DP), o.ctypes.data_as(hip._DP)) == 0
    assert np.array_equal(outs[0], outs[1])
    gp.close()
    sc = clean_scene(oracle, seed=6, param_noise=0.3)
    runs = []
    for generic in (False, False, True):
        gp = dogleg_problem(hip, sc, "subspace", ("cauchy", 1.0, 1.0, 1.0), generic)
        x, S = gp.minimize(sc[-1], max_num_iterations=8)
        runs.append((x, S))
        gp.close()
    x1, S1 = runs[0]
    for x, S in runs[1:]:
        assert S.num_iterations_logged == S1.num_iterations_logged and S.num_linear_solves == S1.num_linear_solves
        for i in range(S1.num_iterations_logged):
            a_, b_ = S1.iterations[i], S.iterations[i]
            assert (a_.step_is_successful, a_.step_is_valid) == (b_.step_is_successful, b_.step_is_valid)
            assert abs(a_.cost - b_.cost) <= 1e-6 * a_.cost
        assert rel(x, x1) <= 1e-3


def test_levenberg_marquardt_is_unchanged(hip, oracle, outlier_scene):
    nc, npts, cam, pt, obs, x0 = outlier_scene
    out = []
    for how in ("never", "lm", "dogleg_then_lm"):
        gp = problem(hip, nc, npts, cam, pt, obs, DENSE_SCHUR, 2)
        if how == "lm":
            gp.set_trust_region_strategy("levenberg_marquardt")
        elif how == "dogleg_then_lm":
            gp.set_trust_region_strategy("dogleg", "subspace")
            gp.minimize(x0, max_num_iterations=2)
            gp.set_trust_region_strategy("levenberg_marquardt")
        x, S = gp.minimize(x0, max_num_iterations=6)
        out.append((x, S.num_linear_solves, [(S.iterations[i].cost, S.iterations[i].trust_region_radius) for i in range(S.num_iterations_logged)]))
        gp.close()
    # (the same launches: what remains is the DENSE_SCHUR solve's own run-to-run rounding)
    for x, n, its in out[1:]:
        assert n == out[0][1] and len(its) == len(out[0][2]) and rel(x, out[0][0]) <= 1e-12
        for (c, r), (c0, r0) in zip(its, out[0][2]):
            assert abs(c - c0) <= 1e-13 * c0 and r == pytest.approx(r0, rel=1e-12)


def test_argument_validation(hip, oracle):
    nc, npts, cam, pt, obs, _ = clean_scene(oracle)
    for solver_type, pre in ((5, 2), (6, 1)):   # ITERATIVE_SCHUR, CGNR: Ceres refuses DOGLEG (I/solver.cc:431-438)
        gp = problem(hip, nc, npts, cam, pt, obs, solver_type, pre)
        with pytest.raises(hip.HipError, match="DOGLEG only supports exact factorization based linear solvers"):
            gp.set_trust_region_strategy("dogleg", "traditional")
        gp.set_trust_region_strategy("levenberg_marquardt")
        gp.close()
    gp = problem(hip, nc, npts, cam, pt, obs, DENSE_SCHUR, 2)
    lib = hip.load_library()
    assert lib.ceres_hip_bal_set_trust_region_strategy(gp._h, 2, 0) == -1
    assert b"unknown strategy" in lib.ceres_hip_bal_last_error(gp._h)
    assert lib.ceres_hip_bal_set_trust_region_strategy(gp._h, 1, 2) == -1
    assert b"unknown dogleg_type" in lib.ceres_hip_bal_last_error(gp._h)
    with pytest.raises(ValueError):
        gp.set_trust_region_strategy("dogleg", "double")
    gp.close()


@pytest.mark.parametrize("kind", ["traditional", "subspace"])
def test_cpp_host_mirror_selects_dogleg(hip, oracle, tmp_path, kind):
    """HipBalProblem::SetTrustRegionStrategy through host_driver (BAL file -> DENSE_SCHUR + DOGLEG -> Minimize): the same run as the
    Python mirror over the same C ABI."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    op = oracle.BalProblem.generate(8, 250, 1200, seed=17)
    op.build_structure(True)
    f = str(tmp_path / "problem.txt")
    assert op.write(f) == 0
    exe = os.path.join(ROOT, "ceres-solver_amd", "host", "host_driver")
    r = subprocess.run([exe, f, "6", kind + "_dogleg"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(re.findall(r"(\w+)=([^ ]+)", [l for l in r.stdout.splitlines() if l.startswith("bal ")][0]))
    o = hip.LinearSolverOptions(type=DENSE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=500)
    gp, x0 = hip.BalProblem.from_file(o, f)
    gp.set_trust_region_strategy("dogleg", kind)
    x, S = gp.minimize(x0, max_num_iterations=6)
    gp.close()
    assert float(kv["initial_cost"]) == pytest.approx(S.initial_cost, rel=1e-13)
    assert float(kv["final_cost"]) == pytest.approx(S.final_cost, rel=1e-6)
    assert int(kv["successful"]) == S.num_successful_steps and int(kv["linear_solves"]) == S.num_linear_solves
    assert int(kv["termination"]) == S.termination_type
    assert S.final_cost < 0.5 * S.initial_cost
    r = subprocess.run([exe, f, "6", "double_dogleg"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "unknown dogleg type" in r.stdout


def test_gram_and_model_cost_probes(hip, oracle, outlier_scene):
    """ceres_hip_time_op's two passes over J that tools/dogleg_times.py compares run on the loaded Jacobian and take time."""
    nc, npts, cam, pt, obs, x0 = outlier_scene
    gp = problem(hip, nc, npts, cam, pt, obs, DENSE_SCHUR, 2)
    gp.evaluate(x0, jacobian=True)
    lib = hip.load_library()
    s = lib.ceres_hip_bal_linear_solver(gp._h)
    for op in (hip.TIMED_JACOBIAN_GRAM, hip.TIMED_MODEL_COST):
        ms = np.zeros(1)
        assert lib.ceres_hip_time_op(s, op, 5, ms.ctypes.data_as(hip._DP)) == 0
        assert 0.0 < ms[0] < 1e3
    gp.close()
