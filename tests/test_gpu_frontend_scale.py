"""The BAL front end beyond its kernels' grid caps (csrc/device.h: kMaxEvalGrid, kMaxLsCameraGrid, kMaxVecGrid), where every kernel takes a
second trip of its grid-stride loop: ceres_hip_bal_evaluate, ceres_hip_bal_evaluate_gradient, ceres_hip_bal_minimize and
ceres_hip_bal_minimize_line_search on the wide scene of tests/frontend_scale_cases.py (600 000 observations; tests/test_frontend_scale_cpu.py
holds it to exceed the caps and the compared line search runs to be non-degenerate), against references that need no dense Jacobian —
the oracle's evaluator and trust-region loop, constant_blocks_reference.Problem.evaluate and line_search_reference.minimize.

Quantities per element (residuals, Jacobian values, the gradient per block) keep the small tests' tolerances: nothing in them grows
with the size.  The cost is a sum over all rows, added on the device in another order than in a reference (per thread over the trips, a
butterfly across lanes, (0 + 1) + (2 + 3) across wavefronts, the workgroups' partial sums by the host in index order): its bound is the
larger of the small tests' 1e-13 and ten times the reference's own spread — its cost against math.fsum of the terms it added —, the factor
design/14_cluster_jacobi.md §14.3 allows another summation order; measured in the test, printed, recorded in design/18_frontend_scale.md."""
import math

import numpy as np
import pytest

import frontend_scale_cases as F
from test_gpu_bal_frontend import check_same_trajectory
from test_gpu_line_search import OP_TOL, block_deviation, check_gradient, device_problem, follow_the_restatement
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

COST_TOL = 1e-13   # test_evaluate_matches_oracle_dual_numbers
RESIDUAL_TOL = {"angle_axis": 1e-13, "quaternion": 1e-13, "quaternion_manifold": 1e-13}   # test_gpu_bal_frontend / test_gpu_quaternion_cameras
JACOBIAN_TOL = 1e-12
LOSS_NAME = {None: "none", F.HUBER: "huber", F.CAUCHY: "cauchy"}


@pytest.fixture(scope="module")
def handles(hip, oracle):
    """One device problem per (camera model, mask set, linear solver), opened when first asked for and shared by the module's tests."""
    opened = {}

    def get(camera, masks="none", solver=(5, 2)):
        key = (camera, masks, solver)
        if key not in opened:
            cc, cp = F.MASKS[masks]
            opened[key] = device_problem(hip, F.scene(oracle), camera, cc, cp, solver=solver)
        return opened[key]
    yield get
    for gp in opened.values():
        gp.close()


def set_loss(gp, loss):
    gp.set_loss(*(loss if loss else ("trivial", 1.0, 1.0, 1.0)))


def cost_bound(cost, terms):
    """(bound, the reference's own spread): its cost against the exactly rounded sum of the terms it added."""
    spread = abs(cost - math.fsum(terms)) / cost
    return max(COST_TOL, 10.0 * spread), spread


def by_trip(what, a, b, upper):
    """rel(a, b) over the entries of the first trip and over those of the later trips (upper: the mask of the latter), printed."""
    lo, hi = rel(a[~upper], b[~upper]), rel(a[upper], b[upper])
    print(f"  {what}: rows below the cap {lo:.3e}, rows at or above it {hi:.3e}")
    return lo, hi


def check_evaluation(gp, camera, reference, row_has_e, row_has_f, cw, terms, w=None):
    """ceres_hip_bal_evaluate against (x0, cost, residuals, values, gradient) of a reference, the deviations by trip."""
    x0, cost_r, res_r, vals_r, g_r = reference
    cap = F.caps()["rows"]
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    bound, spread = cost_bound(cost_r, terms)
    dc = abs(cost - cost_r) / cost_r
    print(f"  cost: deviation {dc:.3e}, bound {bound:.3e} (the reference's own spread {spread:.3e})")
    rows = res_r.shape[0] // 2
    assert rows > cap and res.shape == res_r.shape and vals.shape == vals_r.shape and grad.shape == g_r.shape
    upper_res = np.repeat(np.arange(rows) >= cap, 2)
    value_row = np.concatenate([np.repeat(np.flatnonzero(row_has_e), 6), np.repeat(np.flatnonzero(row_has_f), 2 * cw)])
    assert value_row.shape == vals.shape
    dr = by_trip("residuals", res, res_r, upper_res)
    dv = by_trip("Jacobian values", vals, vals_r, value_row >= cap)
    dg = rel(grad, g_r)
    print(f"  gradient: {dg:.3e}")
    assert dc <= bound
    assert max(dr) <= RESIDUAL_TOL[camera] and max(dv) <= JACOBIAN_TOL and dg <= 1e-12
    if w is not None:
        db = block_deviation(grad, g_r, w)
        print(f"  gradient, worst block: {db:.3e}")
        assert db <= OP_TOL
    c2, r2, g2, v2 = gp.evaluate(x0)   # cost only: another instantiation, the same sum
    assert c2 == cost and r2 is None and g2 is None and v2 is None
    return cost, grad


# ---- a. evaluate ----
def test_evaluate_matches_the_oracle_past_the_cap(hip, oracle, handles):
    """Angle-axis, no loss, against the oracle's dual numbers (as test_evaluate_matches_oracle_dual_numbers), row order included."""
    op = F.oracle_problem(oracle)
    gp = handles("angle_axis")
    set_loss(gp, None)
    x0 = F.initial_state(oracle, "angle_axis")
    cost_o, res_o, vals_o = op.evaluate(x0)
    cam, pt, _ = op.indices()
    order = gp.row_order()
    assert np.all(np.diff(pt[order]) >= 0) and np.all(np.diff(order)[np.diff(pt[order]) == 0] > 0)   # grouped by point, stable
    g_o = oracle.Matrix(op.bs, 0).left_multiply(vals_o, res_o)
    terms = 0.5 * (res_o[0::2] ** 2 + res_o[1::2] ** 2)
    every = np.ones(op.num_observations, bool)
    _, _, _, vals = gp.evaluate(x0, jacobian=True)
    # analytic Jacobian against forward-mode duals of the same formula, entry by entry
    assert np.max(np.abs(vals - vals_o) / (np.abs(vals_o) + 1e-9 * np.abs(vals_o).max())) <= 1e-9
    check_evaluation(gp, "angle_axis", (x0, cost_o, res_o, vals_o, g_o), every, every, 9, terms)


@pytest.mark.parametrize("camera,loss,masks", F.EVALUATE_CONFIGS,
                         ids=lambda v: LOSS_NAME.get(v, v) if not isinstance(v, str) else v)
def test_evaluate_matches_the_reference_evaluator_past_the_cap(hip, oracle, handles, camera, loss, masks):
    w, x0, cost_r, res_r, vals_r, g_r = F.reference_evaluation(oracle, camera, loss, masks)
    gp = handles(camera, masks)
    set_loss(gp, loss)
    assert np.array_equal(gp.row_order(), w.row_order)
    rows, rows_e, removed, nfc, nfp = gp.reduced_sizes()
    assert (rows, rows_e, removed) == (w.n_rows, w.n_rows_e, w.removed.size) and gp.num_effective_parameters == w.n
    check_evaluation(gp, camera, (x0, cost_r, res_r, vals_r, g_r), w.row_has_e, w.row_has_f, w.cw, F.row_cost_terms(w, x0), w=w)


# ---- b. evaluate_gradient ----
@pytest.mark.parametrize("camera,loss,masks", F.GRADIENT_CONFIGS,
                         ids=lambda v: LOSS_NAME.get(v, v) if not isinstance(v, str) else v)
def test_gradient_matches_the_reference_evaluator_past_both_caps(hip, oracle, handles, camera, loss, masks):
    """ls_point_pass_kernel beyond kMaxEvalGrid x 4 x 64 rows and ls_camera_pass_kernel beyond kMaxLsCameraGrid x 4 camera chunks:
    the same bits on a second call, every block within OP_TOL of the reference and of evaluate()."""
    w, x0, cost_r, _, _, g_r = F.reference_evaluation(oracle, camera, loss, masks)
    gp = handles(camera, masks)
    set_loss(gp, loss)
    assert gp.num_effective_parameters == g_r.shape[0]
    _, g = check_gradient(gp, w, x0, cost_r, g_r)
    # where the worst block lies: the points whose rows reach the second trip, the other points, the cameras
    nfp = int(np.count_nonzero(w.pcol >= 0))
    last_row = np.full(nfp, -1)
    last_row[w.pcol[w.pt[w.row_order[:w.n_rows_e]]]] = np.arange(w.n_rows_e)   # (ascending rows: the last one stays)
    dev = np.abs(g - g_r)
    pdev = dev[:3 * nfp].reshape(-1, 3).max(axis=1) / np.abs(g_r[:3 * nfp]).reshape(-1, 3).max(axis=1)
    cdev = dev[3 * nfp:].reshape(-1, w.cw).max(axis=1) / np.abs(g_r[3 * nfp:]).reshape(-1, w.cw).max(axis=1)
    upper = last_row >= F.caps()["rows"]
    print(f"  worst block: points below the cap {pdev[~upper].max():.3e}, points at or above it {pdev[upper].max():.3e}, cameras {cdev.max():.3e}")


# ---- c. minimize (Levenberg-Marquardt) against the oracle's own loop ----
LM_ITERATIONS = 4
# eta = 1e-12 on both sides (test_gpu_robust_loss.py): both linear solves converge, so a different CG stopping decision cannot part the
# trajectories.  The initial radius: with the default 1e4 the oracle's CG does not get there in its 500 iterations on this scene (408, 500,
# 500, 394 iterations, 148 s on 8 cores — measured on the oracle alone) and the comparison would be one of CG's rounding after 500
# iterations; from a radius of 1 it converges in 9, 14, 23, 40 iterations (SCHUR_JACOBI) and every step is accepted.
LM_OPTIONS = dict(max_num_iterations=LM_ITERATIONS, eta=1e-12)
LM_RADIUS = 1.0
TILE_FORMS = (None, "0", "2", "3")
_ORACLE_LM = {}


def oracle_lm(oracle, solver):
    """(summary, final state) of op.lm_solve from x0, once per linear solver."""
    if solver not in _ORACLE_LM:
        op = F.oracle_problem(oracle)
        op.set_state(F.initial_state(oracle, "angle_axis"))
        S = op.lm_solve(solver_type=solver[0], preconditioner=solver[1], max_it=500, initial_radius=LM_RADIUS, **LM_OPTIONS)
        _ORACLE_LM[solver] = (S, op.state())
        op.set_state(F.initial_state(oracle, "angle_axis"))
    return _ORACLE_LM[solver]


def check_against_the_oracle_loop(oracle, gp, run, solver, label, cg_tol=1):
    Sa, xa = oracle_lm(oracle, solver)
    x, Sb = run
    op = F.oracle_problem(oracle)
    x0 = F.initial_state(oracle, "angle_axis")
    cost_o, res_o, _ = op.evaluate(x0, jacobian=False)
    bound, spread = cost_bound(cost_o, 0.5 * (res_o[0::2] ** 2 + res_o[1::2] ** 2))
    d0 = abs(Sb.initial_cost - Sa.initial_cost) / Sa.initial_cost
    dg = abs(Sb.iterations[0].gradient_max_norm - Sa.iterations[0].gradient_max_norm) / Sa.iterations[0].gradient_max_norm
    worst = max(abs(Sa.iterations[i].cost - Sb.iterations[i].cost) / Sa.iterations[i].cost for i in range(Sa.num_iterations_logged))
    print(f"  {label}: initial cost {d0:.3e} (bound {bound:.3e}, the oracle's own spread {spread:.3e}), gradient_max_norm {dg:.3e}, "
          f"worst cost of the trajectory {worst:.3e}, state {rel(x, xa):.3e}, CG iterations "
          f"{[Sb.iterations[i].linear_solver_iterations for i in range(Sb.num_iterations_logged)]} / "
          f"{[Sa.iterations[i].linear_solver_iterations for i in range(Sa.num_iterations_logged)]}")
    assert abs(Sa.initial_cost - cost_o) <= bound * cost_o and d0 <= bound and dg <= OP_TOL   # (the oracle's threads add in no fixed order)
    assert Sa.num_iterations_logged == LM_ITERATIONS + 1 and Sa.num_successful_steps == LM_ITERATIONS
    check_same_trajectory(Sa, Sb, 1e-6, cg_tol)
    assert Sb.termination_type == Sa.termination and Sb.final_cost < 0.6 * Sb.initial_cost
    assert rel(x, xa) <= 1e-5
    assert gp.evaluate(x)[0] == pytest.approx(Sb.final_cost, rel=1e-12)   # the returned state is the one whose cost is reported


@pytest.fixture(scope="module")
def tile_form_runs(hip, oracle, handles):
    """ceres_hip_bal_minimize on ITERATIVE_SCHUR + SCHUR_JACOBI under every form of CERES_HIP_EVAL_TILES (unset: the evaluator writes the
    solver's tiles — bal_evaluate_tiles_kernel, here more than kMaxEvalGrid x 4 tiles; "0": the row-order evaluator and a re-layout)."""
    gp = handles("angle_axis")
    set_loss(gp, None)
    assert gp.solver_info().kernel_path == hip.PATH_BAL
    x0 = F.initial_state(oracle, "angle_axis")
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        for form in TILE_FORMS:
            if form is None:
                mp.delenv("CERES_HIP_EVAL_TILES", raising=False)
            else:
                mp.setenv("CERES_HIP_EVAL_TILES", form)
            runs[form] = gp.minimize(x0, initial_trust_region_radius=LM_RADIUS, **LM_OPTIONS)
    return runs


@pytest.mark.parametrize("form", TILE_FORMS, ids=lambda f: "unset" if f is None else f)
def test_minimize_follows_the_oracle_loop_past_the_tile_cap(hip, oracle, handles, tile_form_runs, form):
    check_against_the_oracle_loop(oracle, handles("angle_axis"), tile_form_runs[form], (5, 2), f"CERES_HIP_EVAL_TILES={form}")


def test_tile_forms_agree_past_the_tile_cap(tile_form_runs):
    """The tighter form-against-form checks of test_evaluator_writing_the_tiles_is_the_two_pass_form: the same numbers in the same
    tiles, whichever kernel wrote them."""
    xb, Sb = tile_form_runs["0"]
    for form in (None, "2", "3"):
        xa, Sa = tile_form_runs[form]
        assert Sa.num_iterations_logged == Sb.num_iterations_logged and Sa.num_iterations_logged >= 4
        for i in range(Sa.num_iterations_logged):
            a, b = Sa.iterations[i], Sb.iterations[i]
            assert (a.step_is_successful, a.step_is_valid) == (b.step_is_successful, b.step_is_valid), (form, i)
            assert a.linear_solver_iterations == b.linear_solver_iterations, (form, i)
            assert abs(a.cost - b.cost) <= 1e-9 * abs(a.cost) and abs(a.gradient_max_norm - b.gradient_max_norm) <= 1e-7 * abs(a.gradient_max_norm), (form, i)
        print("  form", form, "cost", max(abs(Sa.iterations[i].cost - Sb.iterations[i].cost) / Sb.iterations[i].cost for i in range(Sa.num_iterations_logged)),
              "state", rel(xa, xb))
        assert rel(xa, xb) <= 1e-7, form


# CG iteration counts of CGNR + JACOBI: at eta = 1e-12 and 45 to 77 iterations the stopping test compares a change of Q of 1e-14 of Q,
# the rounding of the sums that make Q.  The oracle's own counts on this run are 18, 27-28, 44-46, 75-77 depending on the order its
# threads add in (8, 4, 3 threads and repeated runs, measured on the oracle alone; its costs move by 1.0e-9 with them; multiplying
# the observations by 1 + 1e-15 N(0, 1), seeds 1 and 2, moves no count of CGNR and one count of ITERATIVE_SCHUR by 1): two counts
# that each spread over 2 may differ by 4.  Costs, radii and the state keep the small test's tolerances.
CGNR_CG_TOL = 4


def test_minimize_cgnr_follows_the_oracle_loop_past_the_cap(hip, oracle, handles):
    gp = handles("angle_axis", solver=(6, 1))
    set_loss(gp, None)
    run = gp.minimize(F.initial_state(oracle, "angle_axis"), initial_trust_region_radius=LM_RADIUS, **LM_OPTIONS)
    check_against_the_oracle_loop(oracle, gp, run, (6, 1), "CGNR + JACOBI", cg_tol=CGNR_CG_TOL)


# ---- d. the line search minimizer ----
@pytest.mark.parametrize("name", list(F.LINE_SEARCH_CASES))
def test_minimize_line_search_follows_the_restatement_past_the_caps(hip, oracle, handles, name):
    camera, loss, masks, opts = F.LINE_SEARCH_CASES[name]
    w, x0, reference = F.run_line_search_reference(oracle, name)
    gp = handles(camera, masks)
    set_loss(gp, loss)
    follow_the_restatement(gp, w, x0, reference, F.LINE_SEARCH_ITERATIONS, opts, masks != "none", name)
