"""Shared camera intrinsics of the BAL front end (ceres_hip_bal_create_with_shared_intrinsics: one [f, k1, k2] parameter block per group of
cameras beside a 6-wide pose block per camera) on the device, through the C ABI, against the restatement
(tests/shared_intrinsics_reference.py, held to the wrapped restatement by tests/test_shared_intrinsics_cpu.py).  Scenes, limits and
tolerances are those of tests/test_gpu_frontend_matrix.py as tests/test_gpu_fixed_intrinsics.py uses them; the table
(tests/shared_intrinsics_cases.py) gives every grouping layout every level of every other factor, and excuses no case."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_reference as F
import shared_intrinsics_cases as C
import shared_intrinsics_reference as SI
from test_gpu_frontend_matrix import NAMES, exceeded, tolerances, trajectory
from test_gpu_operators import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scenes(oracle):
    return C.scenes(oracle)


def device_problem(hip, sc, groups, constant=(), solver=(5, 2), generic=0):
    nc, npts, cam, pt, obs, _ = sc
    o = hip.LinearSolverOptions(type=solver[0], preconditioner_type=solver[1], min_num_iterations=0, max_num_iterations=10000,
                                force_generic_path=bool(generic))
    mask = np.zeros(nc, bool)
    mask[np.asarray(constant, dtype=np.int64)] = True
    return hip.BalProblem(o, nc, npts, cam, pt, obs, constant_cameras=mask if mask.any() else None, camera_groups=groups)


def evaluation_deviations(gp, w, x0, xc, sc):
    dev = {}
    nc, npts, cam, pt = sc[0], sc[1], sc[2], sc[3]
    assert np.array_equal(gp.row_order(), np.argsort(pt, kind="stable"))
    rows, rows_e, removed, nfc, nfp = gp.reduced_sizes()
    assert (rows, rows_e, removed, nfc, nfp) == (w.n_rows, w.n_rows, 0, w.nfc, npts)
    assert gp.num_parameters == x0.size == 3 * npts + 9 * nc and gp.num_effective_parameters == w.n == 3 * npts + 6 * nfc + 3 * w.ng
    assert gp.num_residuals == 2 * w.n_rows and gp.num_intrinsics_groups == w.ng and gp.camera_tangent_size == 6 and gp.camera_state_size == 9
    cost_r, res_r, vals_r, g_r = w.evaluate(xc)
    assert gp.num_jacobian_values == vals_r.size
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    dev["eval_cost"] = abs(cost - cost_r) / cost_r
    dev["eval_residuals"], dev["eval_jacobian"], dev["eval_gradient"] = rel(res, res_r), rel(vals, vals_r), rel(grad, g_r)
    assert gp.fixed_cost(x0) == 0.0   # (no row is removed)
    print("evaluate:", dev)
    return dev


def loop_deviations(gp, w, x0, xc, case, max_num_iterations=8):
    """test_gpu_constant_blocks.loop_deviations between an ambient device state and the restatement's compact one (no fixed cost, no
    inner iterations): flags and the solve pattern up to the iteration where the costs first part by more than the case's tolerance —
    which fails the cost check where costs are compared —, the solve count and termination only if they never part."""
    c = dict(zip(NAMES, case))
    cost_tol = tolerances(case)[0]
    dev = {}
    opts = dict(max_num_iterations=max_num_iterations, jacobi_scaling=c["jacobi"])
    xr, Sr = F.minimize(w, xc, c["strategy"], **opts)
    its = Sr["iterations"]
    x, S = gp.minimize(x0, eta=1e-12, **opts)
    dev["initial_cost"] = abs(S.initial_cost - Sr["initial_cost"]) / Sr["initial_cost"]
    dev["iterations"] = abs(S.num_iterations_logged - len(its))
    flags = costs = radii = solves = 0
    parted = False
    for i, it in enumerate(its[:S.num_iterations_logged]):
        d = S.iterations[i]
        if abs(d.cost - it["cost"]) > cost_tol * abs(it["cost"]):
            parted = True
        costs = max(costs, abs(d.cost - it["cost"]) / abs(it["cost"]))
        radii = max(radii, abs(d.trust_region_radius - it["trust_region_radius"]) / it["trust_region_radius"])
        if parted:
            continue
        flags += (d.step_is_successful, d.step_is_valid) != (it["step_is_successful"], it["step_is_valid"])
        solves += i > 0 and (d.linear_solver_iterations == 0) != (it["solves"] == 0)
    dev.update(flags=flags, cost=costs, radius=radii, solve_pattern=solves)
    dev["num_linear_solves"] = 0 if parted else abs(S.num_linear_solves - Sr["num_linear_solves"])
    dev["termination"] = 0 if parted else int(S.termination_type != Sr["termination_type"])
    dev["iterations"] = 0 if parted else dev["iterations"]
    dev["final_cost"] = abs(S.final_cost - Sr["final_cost"]) / Sr["final_cost"]
    dev["state"] = rel(w.compact(x), xr)
    dev["final_vs_evaluate"] = abs(gp.evaluate(x)[0] - S.final_cost) / S.final_cost   # the returned state is the one reported
    # constant poses: read, never written; every group: one set of bits
    dev["constant_poses_changed"] = int(np.count_nonzero(x[w.constant_state].view(np.int64) != x0[w.constant_state].view(np.int64)))
    dev["groups_differ"] = int(not w.groups_identical(x))
    dev["free_blocks_moved"] = int(np.count_nonzero(x != x0))
    return dev


def one_side(hip, oracle, sc, entry, loop):
    layout, constant, case = entry
    c = dict(zip(NAMES, case))
    loss = C.loss_of(case)
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, constant, loss)
    gp = device_problem(hip, w.scene, groups, const, c["solver"], c["generic"])
    try:
        if loss:
            gp.set_loss(*loss)
        if c["strategy"] != "lm":
            gp.set_trust_region_strategy("dogleg", c["strategy"])
        return loop_deviations(gp, w, x0, xc, case) if loop else evaluation_deviations(gp, w, x0, xc, w.scene)
    finally:
        gp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", C.TABLE, ids=C.si_id)
def test_case_follows_the_restatement(hip, oracle, scenes, entry):
    dev = one_side(hip, oracle, scenes["edge"], entry, loop=False)
    dev.update({"edge_" + k: v for k, v in one_side(hip, oracle, scenes["edge"], entry, loop=True).items()})
    dev.update(one_side(hip, oracle, scenes["clean"], entry, loop=True))
    lim = C.si_limits(entry)
    print(C.si_id(entry), dev)
    assert dev["free_blocks_moved"] > 0 and dev["edge_free_blocks_moved"] > 0
    assert not exceeded(dev, lim), (exceeded(dev, lim), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,constant,strategy", [("two", "camera0", "lm"), ("one", "none", "traditional")])
def test_pixels_as_generated_on_dense_schur(hip, oracle, scenes, layout, constant, strategy):
    """The scenes' own pixels under shared intrinsics — cameras of focal lengths 800 .. 1180 on one value: the large-residual problem
    on which Ceres' CG rule ends short of the exact step (shared_intrinsics_cases.shared_scene).  DENSE_SCHUR takes the exact step the
    restatement takes, so there that regime is held to the table's limits, on both scenes."""
    case = ("angle_axis", "none", 1.0, strategy, (3, 0), 0, None, 1, None, None)
    entry = (layout, constant, case)
    dev = {}
    for scene, pre in (("edge", "edge_"), ("clean", "")):
        w, x0, xc, groups, const = C.reference(oracle, scenes[scene], layout, constant, None, as_generated=True)
        assert not np.array_equal(w.scene[4], C.reference(oracle, scenes[scene], layout, constant, None)[0].scene[4])
        gp = device_problem(hip, w.scene, groups, const, (3, 0))
        try:
            if strategy != "lm":
                gp.set_trust_region_strategy("dogleg", strategy)
            if scene == "edge":
                dev.update(evaluation_deviations(gp, w, x0, xc, w.scene))
            dev.update({pre + k: v for k, v in loop_deviations(gp, w, x0, xc, case).items()})
        finally:
            gp.close()
    lim = C.si_limits(entry)
    print(layout, constant, strategy, dev)
    assert all(k in lim for k in ("edge_cost", "edge_state", "cost", "state"))   # (values compared on both scenes)
    assert not exceeded(dev, lim), (exceeded(dev, lim), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [(5, 2), (5, 1), (6, 1), (3, 0)])
def test_which_kernels_run(hip, scenes, solver):
    """ceres_hip_set_structure's decision, stated: the structure alone decides, whatever the solver.  One or two groups take the
    <2,3,6> tile plan with the shared strip — with and without constant cameras, whose rows are the strip shapes' rows without a camera
    cell; CGNR too, since the front end hands over the elimination order and a 3-wide group block is not read as a point.  Three groups
    (nine shared scalars, more than the strip takes), a group per camera, and a group of one camera (it ties with that camera's pose
    in the plan's choice of the shared block) run the generic kernels."""
    sc = scenes["clean"]
    for layout, path in (("one", hip.PATH_BAL), ("two", hip.PATH_BAL), ("two_single", hip.PATH_GENERIC), ("three", hip.PATH_GENERIC),
                         ("each", hip.PATH_GENERIC)):
        groups = SI.layout(layout, sc[0])
        for constant in SI.CONSTANT_SETS:
            gp = device_problem(hip, sc, groups, SI.constant_cameras(constant, groups), solver)
            try:
                info = gp.solver_info()
                assert info.kernel_path == path, (layout, constant, info.kernel_path)
                assert gp.camera_tangent_size == 6
                # the camera side: 6 per free pose and 3 per group — two widths, so the detected F block size is dynamic (-1), as
                # DetectStructure reports it; the fused kernels with a strip are compiled for poses 6 and 9 wide
                nfc, ng = gp.reduced_sizes()[3], gp.num_intrinsics_groups
                assert (info.num_f_blocks, info.num_cols_f, info.f_block_size, info.e_block_size) == (nfc + ng, 6 * nfc + 3 * ng, -1, 3)
            finally:
                gp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout,solver,generic", [("one", (5, 2), 0), ("two", (5, 1), 0), ("two_single", (3, 0), 0), ("three", (5, 2), 0),
                                                   ("each", (6, 1), 0), ("two", (5, 2), 1)])
def test_groups_stay_identical_and_constant_poses_untouched(hip, oracle, scenes, layout, solver, generic):
    """After minimize the members of every group hold one set of bits, the constant cameras' poses the caller's — a -0.0 among them —,
    and everything else has moved; the gradient's max norm runs over the tangent."""
    sc = scenes["clean"]
    nc, npts = sc[0], sc[1]
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, "two", None)
    x0 = x0.copy()
    x0[3 * npts + 9 * int(const[1]) + 1] = -0.0   # (a signed zero in a constant pose: x + 0.0 would lose it)
    gp = device_problem(hip, w.scene, groups, const, solver, generic)
    try:
        assert gp.num_effective_parameters == w.n and gp.num_intrinsics_groups == w.ng
        x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
        assert S.final_cost < S.initial_cost
        assert w.groups_identical(x)
        assert np.array_equal(x[w.constant_state].view(np.int64), x0[w.constant_state].view(np.int64))
        assert np.signbit(x[3 * npts + 9 * int(const[1]) + 1]) and x[3 * npts + 9 * int(const[1]) + 1] == 0.0
        moved = np.ones(x0.size, bool)
        moved[w.constant_state] = False
        assert np.all(x[moved] != x0[moved])
        _, _, grad, _ = gp.evaluate(x0, gradient=True)
        assert grad.size == w.n and S.iterations[0].gradient_max_norm == pytest.approx(np.max(np.abs(grad)), rel=1e-12)
    finally:
        gp.close()


@pytest.mark.gpu
def test_a_group_that_disagrees_in_one_bit_is_refused(hip, oracle, scenes):
    sc = scenes["clean"]
    nc, npts = sc[0], sc[1]
    w, x0, xc, groups, const = C.reference(oracle, sc, "two", "camera0", None)
    gp = device_problem(hip, w.scene, groups, const)
    try:
        c0 = gp.evaluate(x0)[0]
        bad = x0.copy()
        at = 3 * npts + 9 * 5 + 7
        bad[at] = np.nextafter(bad[at], np.inf)   # camera 5 (group 1, whose first camera is 1), k1: one bit
        for call, fn in ((lambda: gp.evaluate(bad), "ceres_hip_bal_evaluate"), (lambda: gp.minimize(bad, max_num_iterations=2), "ceres_hip_bal_minimize"),
                         (lambda: gp.fixed_cost(bad), "ceres_hip_bal_fixed_cost")):
            with pytest.raises(hip.HipError) as e:
                call()
            msg = str(e.value)
            assert f"error {hip.E_INVALID}" in msg and fn in msg and "camera 5 coordinate 7" in msg and "camera 1" in msg, msg
        zero = x0.copy()
        zero[3 * npts + 9 * np.flatnonzero(groups == 0) + 8] = 0.0
        zero[3 * npts + 9 * 4 + 8] = -0.0   # (group 0, k2: equal as a number, not as bits)
        with pytest.raises(hip.HipError, match="camera 4 coordinate 8"):
            gp.evaluate(zero)
        assert gp.evaluate(x0)[0] == c0   # the handle works on
    finally:
        gp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout,constant,solver", [("one", "two", (5, 2)), ("three", "camera0", (5, 2)), ("two", "none", (3, 0))])
def test_two_evaluations_give_the_same_bits(hip, oracle, scenes, layout, constant, solver):
    sc = scenes["edge"]
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, constant, None)
    gp = device_problem(hip, w.scene, groups, const, solver)
    try:
        for loss in (None, ("huber", 2.0)):
            if loss:
                gp.set_loss(*loss)
            a = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
            b = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])   # cost, residuals, Jacobian values
            assert gp.evaluate(x0)[0] == a[0]   # (the cost-only kernel: the same sum)
    finally:
        gp.close()


# ---- poison ---------------------------------------------------------------------------------------------------------------------------
POISON_CASES = [("one", "two", (5, 2)), ("two", "camera0", (5, 1)), ("three", "none", (5, 2)), ("two_single", "two", (3, 0)), ("each", "none", (6, 1))]


def poison_run(hip, oracle, layout, constant, solver):
    sc = C.scenes(oracle)["clean"]
    w, x0, xc, groups, const = C.reference(oracle, sc, layout, constant, None)
    gp = device_problem(hip, w.scene, groups, const, solver)
    try:
        gp.set_loss("huber", 2.0)
        ev = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
        x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
        return ev, x, S, x0, w
    finally:
        gp.close()


def child_main():
    """In the child interpreter (CERES_HIP_DEBUG_POISON=nan): every poison case on a fresh handle; one JSON line each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hip = pkg.hip_solver
    hip.load_library()
    for layout, constant, solver in POISON_CASES:
        ev, x, S, _, _ = poison_run(hip, oracle, layout, constant, solver)
        print(json.dumps(dict(cost=ev[0], res=ev[1].tolist(), grad=ev[2].tolist(), vals=ev[3].tolist(), x=x.tolist(),
                              traj=[list(t) for t in trajectory(S)], final=S.final_cost)), flush=True)
    return 0


@pytest.mark.gpu
def test_poisoned_allocations_change_nothing(hip, oracle):
    """CERES_HIP_DEBUG_POISON=nan (read once per process: a child interpreter) fills every new floating-point device buffer with NaN: a
    fresh handle's first evaluation has the same bits, its first minimize the same trajectory, the groups and constant poses hold."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_shared_intrinsics as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr
    got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(got) == len(POISON_CASES)
    for (layout, constant, solver), g in zip(POISON_CASES, got):
        ev, x, S, x0, w = poison_run(hip, oracle, layout, constant, solver)
        gx = np.array(g["x"])
        assert np.isfinite(g["cost"]) and all(np.all(np.isfinite(g[k])) for k in ("res", "grad", "vals", "x"))
        assert g["cost"] == ev[0] and np.array_equal(g["res"], ev[1]) and np.array_equal(g["vals"], ev[3]) and rel(np.array(g["grad"]), ev[2]) <= 1e-12
        case = ("angle_axis", "huber", 1.0, "lm", solver, 0, None, 1, None, None)
        cost_tol, radius_tol, x_tol = tolerances(case)
        ta, tb = trajectory(S), g["traj"]
        assert len(ta) == len(tb) and all(tuple(u[:2]) == tuple(v[:2]) for u, v in zip(ta, tb))
        assert all(np.isfinite(t[2]) and np.isfinite(t[3]) for t in tb)
        assert max(abs(u[2] - v[2]) / abs(u[2]) for u, v in zip(ta, tb)) <= cost_tol and rel(gx, x) <= x_tol
        assert g["final"] < tb[0][2]
        assert w.groups_identical(gx) and np.array_equal(gx[w.constant_state], x0[w.constant_state])


# ---- |x| of the parameter-tolerance test ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_parameter_tolerance_counts_a_group_once(hip, oracle):
    """The scene of test_shared_intrinsics_cpu.norm_scene: the restatement's run ends by the parameter-tolerance test at an iteration
    where |x| over the program's parameter blocks (a group once, no constant pose) decides it, and |x| over the ambient state would have
    ended it one iteration earlier — by a factor of sqrt 2 or more on either side.  The device ends at the same iteration."""
    from test_shared_intrinsics_cpu import norm_scene
    sc, tol, ends_at, ambient_ends_at = norm_scene(oracle)
    w, x0, xc, groups, const = C.reference(oracle, sc, "one", "camera0", None)
    opts = dict(max_num_iterations=12, parameter_tolerance=tol, function_tolerance=0.0, gradient_tolerance=0.0)
    _, Sr = F.minimize(w, xc, "lm", **opts)
    assert Sr["termination_type"] == F.CONVERGENCE and len(Sr["iterations"]) == ends_at + 1 == ambient_ends_at + 2
    for solver in ((3, 0), (5, 2)):
        gp = device_problem(hip, w.scene, groups, const, solver)
        try:
            x, S = gp.minimize(x0, eta=1e-12, **opts)
            print(solver, S.num_iterations_logged, S.message)
            assert S.termination_type == hip.CONVERGENCE and S.message.decode() == "Parameter tolerance reached."
            assert S.num_iterations_logged == ends_at + 1
            for i, it in enumerate(Sr["iterations"]):
                assert (S.iterations[i].step_is_successful, S.iterations[i].step_is_valid) == (it["step_is_successful"], it["step_is_valid"])
        finally:
            gp.close()


# ---- past the evaluator's grid cap ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_evaluate_past_the_grid_cap(hip, oracle):
    """One evaluation with two groups beyond the evaluator's grid cap (kMaxEvalGrid workgroups of kVecBlock rows: the grid-stride loop's
    second trip) on the scene of tests/frontend_scale_cases.py, against the reference evaluator regrouped by the restatement; the
    comparison of tests/test_gpu_frontend_scale.py."""
    import frontend_scale_cases as S
    from test_gpu_frontend_scale import check_evaluation
    nc, npts, cam, pt, obs, _ = S.scene(oracle)
    groups = SI.layout("two", nc)
    x0 = SI.share(S.initial_state(oracle, "angle_axis"), nc, npts, groups)
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=100)
    gp = hip.BalProblem(o, nc, npts, cam, pt, obs, camera_groups=groups)
    try:
        inner = S.reference_problem(oracle, "angle_axis", S.HUBER, "none")
        w = SI.Problem(inner, nc, npts, groups)
        assert gp.num_rows > S.caps()["rows"] and np.array_equal(gp.row_order(), inner.row_order) and gp.num_effective_parameters == w.n
        print("kernel path", gp.solver_info().kernel_path, "camera width", gp.solver_info().f_block_size)
        gp.set_loss(*S.HUBER)
        xc = w.compact(x0)
        cost_r, res_r, vals_r, g_r = w.evaluate(xc)
        every = np.ones(gp.num_rows, bool)
        # (18 values per row behind the E cells, pose cell then group cell: the rows of check_evaluation's trips as for a 9-wide cell)
        check_evaluation(gp, "angle_axis", (x0, cost_r, res_r, vals_r, g_r), every, every, 9, S.row_cost_terms(inner, x0))
    finally:
        gp.close()


# ---- the calls such a handle does not offer yet -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calls_not_offered_answer_unsupported_or_work(hip, oracle, scenes):
    """Inner iterations, the line search minimizer, evaluate_gradient, covariance, a finite bound and the tile timing probe: each call
    returns 0 or CERES_HIP_E_UNSUPPORTED with a message, nothing else, and ceres_hip_bal_evaluate afterwards returns the bits it
    returned before.  (Which of the two is not pinned: a later change that offers one of them keeps this test.)"""
    lib = hip.load_library()
    sc = scenes["clean"]
    w, x0, xc, groups, const = C.reference(oracle, sc, "two", "camera0", None)

    def fresh():
        return device_problem(hip, w.scene, groups, const, (3, 0))
    a, b = ctypes.c_double(), ctypes.c_double()
    calls = []
    for blocks in ("automatic", "cameras", "points", "cameras,points", "points,cameras"):
        calls.append(("set_inner_iterations " + blocks, lambda gp, blocks=blocks: lib.ceres_hip_bal_set_inner_iterations(gp._h, hip.INNER_BLOCKS[blocks], 1e-3)))
    calls.append(("inner_iterate", lambda gp: lib.ceres_hip_bal_inner_iterate(gp._h, hip._p(x0.copy()), ctypes.byref(a), ctypes.byref(b), None)))
    calls.append(("evaluate_gradient", lambda gp: lib.ceres_hip_bal_evaluate_gradient(gp._h, hip._p(x0), ctypes.byref(a),
                                                                                      hip._p(np.zeros(gp.num_parameters)))))

    def line_search(gp):
        o = hip.line_search_options(max_num_iterations=2)
        S = hip.CLineSearchSummary()
        return lib.ceres_hip_bal_minimize_line_search(gp._h, ctypes.byref(o), hip._p(x0.copy()), ctypes.byref(S))
    calls.append(("minimize_line_search", line_search))
    calls.append(("covariance", lambda gp: gp.covariance_raw(x0, [(0, 0)])[0]))

    def bounds(gp):
        lo = np.full(gp.num_parameters, -np.inf)
        lo[0] = x0[0] - 1.0
        return lib.ceres_hip_bal_set_bounds(gp._h, hip._p(lo), None, None)
    calls.append(("set_bounds", bounds))
    calls.append(("tile timing probe", lambda gp: lib.ceres_hip_debug_bal_evaluate_tiles_timing(gp._h, hip._p(x0), 0, 2, hip._p(np.zeros(1)))))
    for name, call in calls:
        gp = fresh()   # (a handle per call: one that is offered may leave its setting in force)
        try:
            before = gp.evaluate(x0, residuals=True, jacobian=True)
            rc = call(gp)
            msg = lib.ceres_hip_bal_last_error(gp._h).decode()
            print(name, rc, msg)
            assert rc in (0, hip.E_UNSUPPORTED), (name, rc, msg)
            if rc == hip.E_UNSUPPORTED:
                assert msg, name
            else:   # (offered: back to the plain loop's settings before the evaluation below)
                assert lib.ceres_hip_bal_set_inner_iterations(gp._h, hip.INNER_BLOCKS[None], 1e-3) == 0
                assert lib.ceres_hip_bal_set_bounds(gp._h, None, None, None) == 0
            after = gp.evaluate(x0, residuals=True, jacobian=True)
            assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[3], before[3])
        finally:
            gp.close()
    # bounds without a finite entry constrain nothing: accepted
    gp = fresh()
    try:
        gp.set_bounds(np.full(gp.num_parameters, -np.inf), np.full(gp.num_parameters, np.inf))
        x, S = gp.minimize(x0, max_num_iterations=3)
        assert S.final_cost < S.initial_cost and w.groups_identical(x)
    finally:
        gp.close()


@pytest.mark.gpu
def test_no_grouping_is_the_constant_blocks_entry_point(hip, scenes):
    """camera_group == NULL through the new creator: the handle of ceres_hip_bal_create_with_constant_blocks — on the generic path the
    same trajectory bit for bit."""
    nc, npts, cam, pt, obs, par = scenes["clean"]
    lib = hip.load_library()
    mask = np.zeros(nc, np.uint8)
    mask[0] = 1
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=10000,
                                force_generic_path=True)

    def run(new_entry):
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, constant_cameras=mask.astype(bool))
        try:
            if new_entry:
                lib.ceres_hip_bal_destroy(gp._h)
                c = hip.COptions(o.type, o.preconditioner_type, o.min_num_iterations, o.max_num_iterations, o.residual_reset_period, npts, o.device,
                                 int(o.force_generic_path), o.cg_check_interval, o.jacobian_storage, o.max_num_spse_iterations,
                                 int(o.use_spse_initialization), o.spse_tolerance, int(o.use_explicit_schur_complement), int(o.visibility_clustering_type))
                i32 = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
                gp._h = lib.ceres_hip_bal_create_with_shared_intrinsics(ctypes.byref(c), 0, nc, npts, cam.shape[0], i32(cam), i32(pt),
                                                                        hip._p(np.ascontiguousarray(obs).reshape(-1)),
                                                                        mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, 0)
                assert gp._h, lib.ceres_hip_bal_last_error(None).decode()
            x0 = gp.state_from_bal(par)
            ev = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
            x, S = gp.minimize(x0, max_num_iterations=6)
            return ev, x, trajectory(S), gp.reduced_sizes(), gp.num_effective_parameters
        finally:
            gp.close()
    old, new = run(False), run(True)
    assert old[0][0] == new[0][0] and all(np.array_equal(u, v) for u, v in zip(old[0][1:], new[0][1:]))
    assert np.array_equal(old[1], new[1]) and old[2] == new[2] and old[3:] == new[3:]
