"""Constant parameter blocks of the BAL front end (ceres_hip_bal_create_with_constant_blocks) on the device, through the C ABI, against
the restatement (tests/constant_blocks_reference.py, held to the unwrapped restatements by tests/test_constant_blocks_cpu.py).  Scenes,
limits, tolerances and the option table are those of tests/test_gpu_frontend_matrix.py; the table here gives every mask set every
level of every other factor."""
import numpy as np
import pytest

import constant_blocks_reference as CB
import frontend_reference as F
import inner_reference as IR
import line_search_reference as LR
from test_gpu_frontend_matrix import (CASES, EDGE_INEXACT_SOLVERS, FACTORS, LOSS_PARAMS, MODELS, NAMES, allowed, case_id, clean_scene, edge_scene,
                                      exceeded, limits, pairs, set_env, tolerances, trajectory)
from test_gpu_operators import rel

MASKS = CB.MASK_SETS


def build_table():
    """For every mask set, rows of test_gpu_frontend_matrix.CASES (each allowed, the table there covers every allowed pair of its
    factors) chosen greedily until the mask set has met every level of every factor: the constant-block factor paired with
    everything.  Deterministic: ties go to the earlier row; each mask set starts one row further down, so that the sets do not all
    take the same rows."""
    table = []
    for m, name in enumerate(MASKS):
        need = {(i, v) for i, (_, levels) in enumerate(FACTORS) for v in levels}
        rows = CASES[m * 7:] + CASES[:m * 7]
        while need:
            best = max(rows, key=lambda c: len(need & set(enumerate(c))))
            gain = need & set(enumerate(best))
            assert gain, need
            need -= gain
            table.append((name, best))
    return table


TABLE = build_table()


def cb_id(entry):
    return entry[0] + "-" + case_id(entry[1])


def test_table_pairs_every_mask_set_with_every_level():
    assert all(allowed(c) for _, c in TABLE) and len(set(TABLE)) == len(TABLE)
    have = {(m, i, v) for m, c in TABLE for i, v in enumerate(c)}
    need = {(m, i, v) for m in MASKS for i, (_, levels) in enumerate(FACTORS) for v in levels}
    assert not need - have, sorted(need - have, key=repr)[:10]
    # every pair of the matrix's own factors is still the matrix's business (its own test); here: the table is drawn from it
    assert all(c in CASES for _, c in TABLE)
    assert all(pairs(c) for _, c in TABLE)
    # the cases whose edge-scene values are not compared: all with inner iterations, and no more than a quarter of those
    ids = {cb_id(e): e for e in TABLE}
    with_inner = [e for e in TABLE if dict(zip(NAMES, e[1]))["inner"]]
    assert all(k in ids and dict(zip(NAMES, ids[k][1]))["inner"] for k in EDGE_ILL_CONDITIONED)
    assert 4 * len(EDGE_ILL_CONDITIONED) <= len(with_inner), (len(EDGE_ILL_CONDITIONED), len(with_inner))
    assert all(k in ids and edge_values_compared(ids[k]) for k in EDGE_DEVICE_UNREPEATABLE)


# Edge-scene cases whose costs, radii and state are NOT compared: the restatement's own 8-iteration trajectory moves by more than a
# hundredth of the case's cost tolerance when every Jacobian value is multiplied by 1 + 1e-14 N(0, 1) (seeds 1 and 2) — the rule and
# the method of test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED, measured on the restatement, on the CPU
# (tools/constant_blocks_conditioning.py prints this table); the largest relative cost deviation is the value.  Flags, solve pattern,
# solve count, inner steps and termination are still compared as far as the costs agree.
EDGE_ILL_CONDITIONED = {
    "point_of_constant_cameras-angle_axis-none-lm-s51-inner=cameras-unscaled-tiles=2-form=lane": 6.4e-02,
    "points_only-angle_axis-tolerant-lm-s51-inner=points,cameras-unscaled-tiles=2-form=wave": 5.1e-02,
    "both_constant-angle_axis-trivialx2.5-lm-s61-inner=cameras,points-unscaled-tiles=2-form=lane": 2.5e-02,
    "both_constant-angle_axis-tolerant-traditional-s30-inner=cameras-form=lane": 1.3e-03,
    "none-angle_axis-none-lm-s61-inner=automatic-unscaled-tiles=0": 1.1e-03,
    "points_only-angle_axis-trivial-lm-s52-inner=automatic-unscaled-tiles=3-form=wave": 6.6e-04,
    "none-angle_axis-trivialx2.5-lm-s61-inner=cameras,points-unscaled-tiles=2-form=lane": 7.9e-06,
    "point_of_constant_cameras-angle_axis-tolerantx2.5-subspace-s30-inner=automatic-form=wave": 3.3e-06,
    "camera_of_constant_points-angle_axis-none-lm-s61-inner=automatic-unscaled-tiles=0": 1.1e-06,
    "cameras01_points3-angle_axis-tolerantx2.5-lm-s51-inner=cameras,points-unscaled-tiles=3-form=lane": 3.7e-08,
}


# Edge-scene cases where the device does not repeat ITSELF to a tenth of the cost tolerance: the largest relative difference of any logged
# cost over three fresh handles (the rule and the method of test_gpu_frontend_matrix.EDGE_DEVICE_UNREPEATABLE — whose own table lists
# the same option sets; tools/constant_blocks_repeatability.py prints this one, on the GPU).  What differs are the costs of REJECTED
# candidates: a sample of the non-linear cost far from the linearisation point, at the end of a hundred CG iterations whose LDS sums
# are not bitwise repeatable (both_constant-…-s52-inner=points,cameras-tiles=3, four fresh handles: iterations 1-4 rejected, CG 109 /
# 110 / 109 / 109 iterations in the first, the four runs' candidate costs -2.9e-7 … -1.1e-6 from the restatement's in the second — a
# spread of 8.6e-7 among themselves — while every accepted iterate agrees with the restatement to 3.4e-9 and with the other runs to
# 4e-12).  For these cases the per-iteration cost check runs over the ACCEPTED iterations ("cost_accepted"); radii, the final cost, the
# state and everything else are compared as for any other case.
EDGE_DEVICE_UNREPEATABLE = {
    "none-quaternion-soft_l_onex2.5-traditional-s30-unscaled": 8.9e-06,
    "camera0-angle_axis-trivial-lm-s52-inner=automatic-unscaled-tiles=3-form=wave": 1.6e-07,
    "both_constant-angle_axis-none-lm-s52-inner=points,cameras-tiles=3": 1.4e-07,
}


def edge_values_compared(entry, conditioning=None):
    c = dict(zip(NAMES, entry[1]))
    if conditioning is None:
        conditioning = EDGE_ILL_CONDITIONED.get(cb_id(entry), 0.0)
    return 100.0 * conditioning <= tolerances(entry[1])[0] and not (c["strategy"] == "lm" and c["solver"] in EDGE_INEXACT_SOLVERS)


LOOP_VALUES = ("cost", "radius", "final_cost", "state")


@pytest.fixture(scope="module")
def edge(oracle):
    return edge_scene(oracle)


@pytest.fixture(scope="module")
def loop_scene(oracle):
    return clean_scene(oracle)


def device_problem(hip, sc, masks, camera="angle_axis", solver=(5, 2), generic=0, new_entry=True):
    """test_gpu_frontend_matrix.device_problem with the mask set; "none" goes through the new entry point too (all-zero masks)."""
    nc, npts, cam, pt, obs, _ = sc
    cc, cp = CB.mask_set(masks, nc, npts, cam, pt)
    o = hip.LinearSolverOptions(type=solver[0], preconditioner_type=solver[1], min_num_iterations=0, max_num_iterations=10000,
                                force_generic_path=bool(generic))
    if not new_entry:
        assert masks == "none"
        return hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=camera)
    return hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=camera, constant_cameras=CB.mask(cc, nc), constant_points=CB.mask(cp, npts))


def reference(oracle, sc, masks, camera, loss):
    nc, npts, cam, pt, obs, _ = sc
    cc, cp = CB.mask_set(masks, nc, npts, cam, pt)
    return CB.Problem(oracle.snavely_batch, MODELS[camera], nc, npts, cam, pt, obs, cc, cp, loss)


def loss_of(c):
    return None if c["loss"] == "none" else (c["loss"],) + LOSS_PARAMS[c["loss"]] + (c["scale"],)


def evaluation_deviations(gp, w, x0):
    dev = {}
    assert np.array_equal(gp.row_order(), w.row_order)
    rows, rows_e, removed, nfc, nfp = gp.reduced_sizes()
    assert (rows, rows_e, removed) == (w.n_rows, w.n_rows_e, w.removed.size)
    assert (nfc, nfp) == (int(np.count_nonzero(w.ccol >= 0)), int(np.count_nonzero(w.pcol >= 0)))
    assert gp.num_parameters == x0.size and gp.num_effective_parameters == w.n and gp.num_residuals == 2 * w.n_rows
    cost_r, res_r, vals_r, g_r = w.evaluate(x0)
    assert gp.num_jacobian_values == vals_r.size
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    dev["eval_cost"] = abs(cost - cost_r) / cost_r
    dev["eval_residuals"], dev["eval_jacobian"], dev["eval_gradient"] = rel(res, res_r), rel(vals, vals_r), rel(grad, g_r)
    fixed_r, fixed = w.fixed_cost(x0), gp.fixed_cost(x0)
    dev["fixed_cost"] = abs(fixed - fixed_r) / fixed_r if fixed_r else abs(fixed)
    print("evaluate:", dev)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("camera", ["angle_axis", "quaternion", "quaternion_manifold"])
def test_evaluate(hip, oracle, edge, masks, camera):
    """cost, residuals, Jacobian values in the reduced layout, gradient and the fixed cost at x0, with no loss, Huber and Tukey."""
    gp = device_problem(hip, edge, masks, camera)
    try:
        x0 = gp.state_from_bal(edge[-1])
        case = (camera, "none", 1.0, "lm", (5, 2), 0, None, 1, None, None)
        lim = {k: v for k, v in limits(case).items() if k.startswith("eval_")}
        lim["fixed_cost"] = lim["eval_cost"]
        for kind in ("none", "huber", "tukey"):
            loss = None if kind == "none" else (kind,) + LOSS_PARAMS[kind] + (1.0,)
            if loss:
                gp.set_loss(*loss)
            dev = evaluation_deviations(gp, reference(oracle, edge, masks, camera, loss), x0)
            assert not exceeded(dev, lim), (kind, exceeded(dev, lim), dev)
    finally:
        gp.close()


def loop_deviations(gp, w, x0, case, inner, max_num_iterations=8):
    """test_gpu_frontend_matrix.loop_deviations with the fixed cost: the restatement minimizes the reduced program; every cost the
    device reports (initial, final, per iteration) includes the removed rows' cost, as TrustRegionMinimizer's do."""
    c = dict(zip(NAMES, case))
    cost_tol = tolerances(case)[0]
    dev = {}
    opts = dict(max_num_iterations=max_num_iterations, jacobi_scaling=c["jacobi"])
    xr, Sr = F.minimize(w, x0, c["strategy"], inner=inner, **opts)
    fixed = w.fixed_cost(x0)
    its = Sr["iterations"]
    x, S = gp.minimize(x0, eta=1e-12, **opts)
    dev["initial_cost"] = abs(S.initial_cost - (Sr["initial_cost"] + fixed)) / (Sr["initial_cost"] + fixed)
    dev["iterations"] = abs(S.num_iterations_logged - len(its))
    flags = costs = costs_accepted = radii = solves = 0
    parted = False
    for i, it in enumerate(its[:S.num_iterations_logged]):
        d = S.iterations[i]
        ref_cost = it["cost"] + fixed
        if abs(d.cost - ref_cost) > cost_tol * abs(ref_cost):
            parted = True
        costs = max(costs, abs(d.cost - ref_cost) / abs(ref_cost))
        if d.step_is_successful and it["step_is_successful"]:
            costs_accepted = max(costs_accepted, abs(d.cost - ref_cost) / abs(ref_cost))
        radii = max(radii, abs(d.trust_region_radius - it["trust_region_radius"]) / it["trust_region_radius"])
        if parted:
            continue
        flags += (d.step_is_successful, d.step_is_valid) != (it["step_is_successful"], it["step_is_valid"])
        solves += i > 0 and (d.linear_solver_iterations == 0) != (it["solves"] == 0)
    dev.update(flags=flags, cost=costs, cost_accepted=costs_accepted, radius=radii, solve_pattern=solves)
    dev["num_linear_solves"] = 0 if parted else abs(S.num_linear_solves - Sr["num_linear_solves"])
    dev["inner_steps"] = 0 if parted else abs(gp.inner_iteration_stats()[0] - Sr["num_inner_iteration_steps"])
    dev["termination"] = 0 if parted else int(S.termination_type != Sr["termination_type"])
    dev["iterations"] = 0 if parted else dev["iterations"]
    dev["final_cost"] = abs(S.final_cost - (Sr["final_cost"] + fixed)) / (Sr["final_cost"] + fixed)
    dev["state"] = rel(x, xr)
    dev["final_vs_evaluate"] = abs(gp.evaluate(x)[0] + gp.fixed_cost(x) - S.final_cost) / S.final_cost
    # constant blocks: read, never written
    dev["constant_blocks_changed"] = int(np.count_nonzero(x[w.constant_state] != x0[w.constant_state]))
    dev["free_blocks_moved"] = int(np.count_nonzero(x != x0))
    if c["camera"] == "quaternion_manifold":
        qn = lambda v: np.linalg.norm(v[3 * w.np_:].reshape(-1, 10)[:, :4], axis=1)
        dev["qnorm"] = float(np.max(np.abs(qn(x) - qn(x0))))
    return dev


def one_side(hip, oracle, sc, entry, loop):
    masks, case = entry
    c = dict(zip(NAMES, case))
    gp = device_problem(hip, sc, masks, c["camera"], c["solver"], c["generic"])
    try:
        loss = loss_of(c)
        if loss:
            gp.set_loss(*loss)
        if c["strategy"] != "lm":
            gp.set_trust_region_strategy("dogleg", c["strategy"])
        w = reference(oracle, sc, masks, c["camera"], loss)
        inner = None
        if c["inner"]:
            gp.set_inner_iterations(c["inner"], 1e-3)
            inner = w.inner_ordering(c["inner"])
        x0 = gp.state_from_bal(sc[-1])
        if loop:
            return loop_deviations(gp, w, x0, case, inner)
        dev = evaluation_deviations(gp, w, x0)
        if inner is not None:   # one pass from x0 (test_gpu_inner_iterations' tolerances)
            npts = w.np_
            xr, _ = IR.one_pass(w.ev, x0, *inner)
            xi, _, c1, its = gp.inner_iterate(x0)
            dev["inner_pass_cost"] = abs(c1 - w.cost(xr)) / c1
            blk = [(xi[:3 * npts].reshape(-1, 3), xr[:3 * npts].reshape(-1, 3)), (xi[3 * npts:].reshape(-1, 9), xr[3 * npts:].reshape(-1, 9))]
            dev["inner_pass_blocks"] = float(max(np.max(np.abs(b - r).max(axis=1) / np.maximum(np.abs(r).max(axis=1), 1e-300)) for b, r in blk))
            dev["inner_constant_blocks_changed"] = int(np.count_nonzero(xi[w.constant_state] != x0[w.constant_state]))
            constant = np.concatenate([w.pcol < 0, w.ccol < 0])
            # -1 exactly on the blocks outside the ordering, the constant ones among them
            dev["inner_block_iterations"] = int(np.count_nonzero((its == -1) != (inner[0] < 0))) + int(np.count_nonzero(its[constant] != -1))
        return dev
    finally:
        gp.close()


def cb_limits(entry):
    lim = limits(entry[1])   # (the matrix's limits; its edge_* value checks are decided by ITS table of ill-conditioned cases: redone below)
    for k in LOOP_VALUES:
        lim.pop("edge_" + k, None)
    lim["cost_accepted"] = lim["cost"]
    if edge_values_compared(entry):
        for k in LOOP_VALUES + ("cost_accepted",):
            lim["edge_" + k] = lim[k]
        if cb_id(entry) in EDGE_DEVICE_UNREPEATABLE:
            del lim["edge_cost"]   # (rejected candidates' costs: see the table)
    lim.pop("tukey_rows", None)
    lim["fixed_cost"] = lim["eval_cost"]
    for pre in ("", "edge_"):
        lim[pre + "constant_blocks_changed"] = 0
    if dict(zip(NAMES, entry[1]))["inner"]:
        lim["inner_constant_blocks_changed"] = lim["inner_block_iterations"] = 0
    return lim


@pytest.mark.gpu
@pytest.mark.parametrize("entry", TABLE, ids=cb_id)
def test_case_follows_the_restatement(hip, oracle, edge, loop_scene, monkeypatch, entry):
    c = dict(zip(NAMES, entry[1]))
    set_env(monkeypatch, "CERES_HIP_EVAL_TILES", c["tiles"])
    set_env(monkeypatch, "CERES_HIP_INNER_FORM", c["inner_form"])
    dev = one_side(hip, oracle, edge, entry, loop=False)
    dev.update({"edge_" + k: v for k, v in one_side(hip, oracle, edge, entry, loop=True).items()})
    dev.update(one_side(hip, oracle, loop_scene, entry, loop=True))
    lim = cb_limits(entry)
    print(cb_id(entry), dev)
    assert dev["free_blocks_moved"] > 0 and dev["edge_free_blocks_moved"] > 0
    assert not exceeded(dev, lim), (exceeded(dev, lim), dev)


def run(gp, x0, n=8):
    cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    x, S = gp.minimize(x0, max_num_iterations=n, eta=1e-12)
    return dict(cost=cost, res=res, grad=grad, vals=vals, x=x, traj=trajectory(S), order=gp.row_order())


def spread(a, b):
    """The largest relative difference of two runs: evaluation, trajectory costs and radii, final state; inf if the flags differ."""
    if len(a["traj"]) != len(b["traj"]) or any(u[:2] != v[:2] for u, v in zip(a["traj"], b["traj"])):
        return np.inf
    d = [abs(a["cost"] - b["cost"]) / b["cost"], rel(a["res"], b["res"]), rel(a["grad"], b["grad"]), rel(a["vals"], b["vals"]), rel(a["x"], b["x"])]
    d += [abs(u[2] - v[2]) / abs(v[2]) for u, v in zip(a["traj"], b["traj"])] + [abs(u[3] - v[3]) / v[3] for u, v in zip(a["traj"], b["traj"])]
    return float(max(d))


@pytest.mark.gpu
@pytest.mark.parametrize("camera,solver,generic,inner", [("angle_axis", (5, 2), 0, None), ("angle_axis", (5, 2), 1, None), ("angle_axis", (6, 1), 0, None),
                                                         ("angle_axis", (3, 0), 0, None), ("angle_axis", (5, 2), 1, "automatic"),
                                                         ("quaternion_manifold", (5, 2), 0, None), ("quaternion", (6, 1), 1, None)])
def test_zero_masks_are_the_old_entry_point(hip, loop_scene, camera, solver, generic, inner):
    """All-zero masks through ceres_hip_bal_create_with_constant_blocks: the handle ceres_hip_bal_create_with_camera builds — same row
    order, same sizes, and the same numbers as far as the old entry point repeats ITSELF on this device.  Cost, residuals and Jacobian
    values come from one thread per observation and a fixed-order sum: equal, always.  The gradient and the loop go through the LDS
    sums and the dense factorisation, which are not bitwise repeatable, and eight iterations amplify that: four fresh old-entry handles
    say how far (their largest mutual difference), and the nearest of two new-entry handles to any of them must be no further — a
    systematic difference of the new entry point would move ALL its pairs.  (First version of this test: the new handle against the
    first old one within twice the largest difference of three — a single draw against a maximum of three, which the amplified noise
    exceeds by chance: 5.6e-7 against 6.6e-8 on quaternion_manifold, ITERATIVE_SCHUR.)  Where the old entry point repeats itself
    exactly — the generic path, inner passes — equality is required."""
    def fresh(new_entry):
        gp = device_problem(hip, loop_scene, "none", camera, solver, generic, new_entry=new_entry)
        try:
            if inner:
                gp.set_inner_iterations(inner, 1e-3)
            out = run(gp, gp.state_from_bal(loop_scene[-1]))
            out["sizes"] = gp.reduced_sizes()
            return out
        finally:
            gp.close()
    old = [fresh(False) for _ in range(4)]
    new = [fresh(True) for _ in range(2)]
    noise = max(spread(old[i], old[j]) for i in range(4) for j in range(i))
    got = min(spread(n, o) for n in new for o in old)
    print("old entry repeats itself to", noise, "; nearest new-entry run differs by", got, "; all:", [spread(n, o) for n in new for o in old])
    assert np.isfinite(noise)
    for n in new:
        assert np.array_equal(n["order"], old[0]["order"]) and n["sizes"] == old[0]["sizes"] and n["sizes"][2] == 0
        assert n["cost"] == old[0]["cost"] and np.array_equal(n["res"], old[0]["res"]) and np.array_equal(n["vals"], old[0]["vals"])
    assert got <= noise, (got, noise)
    if noise == 0.0:
        assert max(spread(n, o) for n in new for o in old) == 0.0
    if generic:
        assert noise == 0.0, noise   # (the premise of requiring equality there)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [(5, 2), (5, 1)], ids=["schur_jacobi", "jacobi"])
@pytest.mark.parametrize("masks", ["camera0", "point_of_constant_cameras"])
def test_constant_cameras_keep_the_tile_order_evaluator(hip, oracle, loop_scene, monkeypatch, masks, solver):
    """Constant cameras alone leave every row its E cell: the fused path keeps the evaluator that writes the tiles, and the loop's
    four evaluator forms (CERES_HIP_EVAL_TILES unset / 0 / 2 / 3) follow one trajectory at the matrix's limits."""
    case = ("angle_axis", "huber", 1.0, "lm", solver, 0, None, 1, None, None)
    cost_tol, radius_tol, x_tol = tolerances(case)
    runs = {}
    for form in (None, "0", "2", "3"):
        set_env(monkeypatch, "CERES_HIP_EVAL_TILES", form)
        gp = device_problem(hip, loop_scene, masks, "angle_axis", solver)
        try:
            x0 = gp.state_from_bal(loop_scene[-1])
            assert gp.solver_info().kernel_path == hip.PATH_BAL
            if form != "0":
                assert gp.evaluate_tiles_timing(x0, 0, 2) > 0.0   # (E_UNSUPPORTED raises: the evaluator writes this structure's tiles)
                gp.close()
                gp = device_problem(hip, loop_scene, masks, "angle_axis", solver)
            else:
                with pytest.raises(hip.HipError):
                    gp.evaluate_tiles_timing(x0, 0, 2)
                gp.close()
                gp = device_problem(hip, loop_scene, masks, "angle_axis", solver)
            gp.set_loss("huber", 2.0)
            x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
            runs[form] = (x, trajectory(S))
        finally:
            gp.close()
    for form in ("0", "2", "3"):
        a, b = runs[form][1], runs[None][1]
        assert len(a) == len(b) >= 2 and all(u[:2] == v[:2] for u, v in zip(a, b))
        dc = max(abs(u[2] - v[2]) / abs(v[2]) for u, v in zip(a, b))
        dr = max(abs(u[3] - v[3]) / v[3] for u, v in zip(a, b))
        print(form, "cost", dc, "radius", dr, "state", rel(runs[form][0], runs[None][0]))
        assert dc <= cost_tol and dr <= radius_tol and rel(runs[form][0], runs[None][0]) <= x_tol


@pytest.mark.gpu
@pytest.mark.parametrize("masks,solver,tiles", [("camera0", (5, 2), None), ("camera0", (3, 0), None), ("points_only", (5, 2), None),
                                                ("both_constant", (6, 1), None)])
def test_poisoned_allocations_do_not_reach_the_results(hip, oracle, loop_scene, monkeypatch, masks, solver, tiles):
    """CERES_HIP_DEBUG_POISON=nan fills every device allocation with NaN: a cell that is not written must not be read."""
    monkeypatch.setenv("CERES_HIP_DEBUG_POISON", "nan")
    set_env(monkeypatch, "CERES_HIP_EVAL_TILES", tiles)
    gp = device_problem(hip, loop_scene, masks, "angle_axis", solver)
    try:
        x0 = gp.state_from_bal(loop_scene[-1])
        gp.set_loss("huber", 2.0)
        w = reference(oracle, loop_scene, masks, "angle_axis", ("huber", 2.0, 1.0, 1.0))
        cost, res, grad, vals = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
        assert all(np.all(np.isfinite(v)) for v in (res, grad, vals)) and np.isfinite(cost) and np.isfinite(gp.fixed_cost(x0))
        x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
        assert np.all(np.isfinite(x)) and all(np.isfinite(t[2]) and np.isfinite(t[3]) for t in trajectory(S))
        assert S.final_cost < S.initial_cost and np.array_equal(x[w.constant_state], x0[w.constant_state])
        xr, Sr = F.minimize(w, x0, "lm", max_num_iterations=8)
        assert abs(S.final_cost - (Sr["final_cost"] + w.fixed_cost(x0))) <= tolerances(("angle_axis", "huber", 1.0, "lm", solver, 0, None, 1, None, None))[0] * S.final_cost
        # Two further inputs, whose every read-back comes through the same stage of partial sums as the loop's (csrc/partial_sums.h) and
        # which no other poisoned test reaches: the line search minimizer (handles with bounds or fixed intrinsics refuse it) on every
        # handle, and the dogleg strategy on the DENSE_SCHUR one (it needs an exact factorisation).  The same bound as the LM run above.
        cost_tol = tolerances(("angle_axis", "huber", 1.0, "lm", solver, 0, None, 1, None, None))[0]
        xl, Sl = gp.minimize_line_search(x0, max_num_iterations=8)
        xlr, Slr = LR.minimize(w, x0, max_num_iterations=8)
        assert np.all(np.isfinite(xl)) and all(np.isfinite(Sl.iterations[k].cost) and np.isfinite(Sl.iterations[k].gradient_max_norm) and
                                               np.isfinite(Sl.iterations[k].step_norm) for k in range(Sl.num_iterations_logged))
        assert Sl.final_cost < Sl.initial_cost and np.array_equal(xl[w.constant_state], x0[w.constant_state])
        print("line search: final cost against the restatement", abs(Sl.final_cost - Slr["final_cost"]) / Sl.final_cost, "bound", cost_tol)
        assert abs(Sl.final_cost - Slr["final_cost"]) <= cost_tol * Sl.final_cost
        if solver == (3, 0):
            gp.set_trust_region_strategy("dogleg", "traditional")
            xd, Sd = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
            assert np.all(np.isfinite(xd)) and all(np.isfinite(t[2]) and np.isfinite(t[3]) for t in trajectory(Sd))
            assert Sd.final_cost < Sd.initial_cost and np.array_equal(xd[w.constant_state], x0[w.constant_state])
            xdr, Sdr = F.minimize(w, x0, "traditional", max_num_iterations=8)
            print("dogleg: final cost against the restatement", abs(Sd.final_cost - (Sdr["final_cost"] + w.fixed_cost(x0))) / Sd.final_cost, "bound", cost_tol)
            assert abs(Sd.final_cost - (Sdr["final_cost"] + w.fixed_cost(x0))) <= cost_tol * Sd.final_cost
    finally:
        gp.close()


@pytest.mark.gpu
def test_reduced_sizes_arguments_are_null_able(hip, loop_scene):
    gp = device_problem(hip, loop_scene, "both_constant")
    try:
        lib = hip.load_library()
        assert lib.ceres_hip_bal_reduced_sizes(gp._h, None, None, None, None, None) == 0
        assert lib.ceres_hip_bal_reduced_sizes(None, None, None, None, None, None) == hip.E_INVALID
        assert gp.reduced_sizes()[2] >= 1 and gp.row_order().size == gp.num_rows < loop_scene[2].shape[0]
    finally:
        gp.close()
