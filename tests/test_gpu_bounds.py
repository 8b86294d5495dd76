"""Bound constraints of the BAL front end on the device (ceres_hip_bal_set_bounds, csrc/bounds.inc, csrc/kernels_bounds.hip): the cases of
tests/bounds_cases.py against the numpy restatement tests/bounds_reference.py (tests/test_bounds_cpu.py holds those runs to be decided
nowhere by rounding), the three kernels alone against numpy, handles that no bound constrains against fresh handles bit for bit, bounds
that never bind, every refusal, and poisoned allocations."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bounds_cases as BC
import bounds_reference as B
import line_search_cases as LC
from conftest import ROOT
from test_gpu_frontend_matrix import tolerances
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu
DBL_MAX = np.finfo(np.float64).max


def device_problem(hip, sc, camera="angle_axis", solver=(5, 2), generic=0, cc=None, cp=None):
    nc, npts, cam, pt, obs, _ = sc
    o = hip.LinearSolverOptions(type=solver[0], preconditioner_type=solver[1], min_num_iterations=0, max_num_iterations=10000,
                                force_generic_path=bool(generic))
    return hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=camera, constant_cameras=cc, constant_points=cp)


def case_problem(hip, ref, name, bounds=True):
    camera, loss, cc, cp, strategy, lso, iters, solver, generic = BC.CASES[name]
    gp = device_problem(hip, ref["sc"], camera, solver, generic, cc, cp)
    if loss:
        gp.set_loss(*loss)
    if strategy != "lm":
        gp.set_trust_region_strategy("dogleg", strategy)
    if bounds:
        gp.set_bounds(ref["lower"], ref["upper"], **lso)
    return gp


def logged(S):
    return [bytes(S.iterations[i]) for i in range(S.num_iterations_logged)]


def run_case(hip, ref, name):
    """What a fresh handle returns for a table case: (x, the summary's numbers, bounds_stats, the cost of evaluate at x — with constant
    blocks plus the fixed cost of the removed rows, which every cost the loop reports includes)."""
    gp = case_problem(hip, ref, name)
    try:
        x, S = gp.minimize(ref["x0"], eta=1e-12, max_num_iterations=BC.CASES[name][6], jacobi_scaling=1)
        st = gp.bounds_stats()
        return x, S, st, gp.evaluate(x)[0] + (gp.fixed_cost(x) if BC.CASES[name][2] or BC.CASES[name][3] else 0.0)
    finally:
        gp.close()


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_follows_the_restatement(hip, oracle, name):
    ref = BC.reference(oracle, name)
    xr, Sr = ref["x"], ref["S"]
    its = Sr["iterations"]
    x, S, st, cost_at_x = run_case(hip, ref, name)
    cost_tol = tolerances(BC.matrix_case(name))[0]
    fixed = ref["pr"].fixed_cost(ref["x0"])   # (the restatement's costs are the reduced program's; 0.0 without constant blocks)
    n = S.num_iterations_logged
    dev = [S.iterations[i] for i in range(n)]
    figures = dict(
        cost=max(abs(d.cost - (r["cost"] + fixed)) / abs(r["cost"] + fixed) for d, r in zip(dev, its)),
        radius=max(abs(d.trust_region_radius - r["trust_region_radius"]) / r["trust_region_radius"] for d, r in zip(dev, its)),
        step_size=max(abs(st["step_size"][i] - r["step_size"]) / r["step_size"] for i, r in enumerate(its[:n])),
        state=rel(x, xr), gradient_max_norm_0=abs(dev[0].gradient_max_norm - its[0]["gradient_max_norm"]) / its[0]["gradient_max_norm"],
        final_vs_evaluate=abs(cost_at_x - S.final_cost) / S.final_cost)
    print(name, {k: f"{v:.2e}" for k, v in figures.items()})
    # exact
    assert n == len(its) and S.termination_type == Sr["termination_type"]
    assert [(d.step_is_valid, d.step_is_successful) for d in dev] == [(r["step_is_valid"], r["step_is_successful"]) for r in its]
    assert S.num_linear_solves == Sr["num_linear_solves"]
    assert st["is_constrained"] == 1 and st["num_projected"] == Sr["num_projected"]
    assert list(st["line_search_iterations"][:n]) == [r["line_search_iterations"] for r in its]
    assert list(st["line_search_success"][:n]) == [r["line_search_success"] for r in its]
    assert np.all(st["line_search_iterations"][n:] == -1) and np.all(st["step_size"][n:] == 1.0)
    assert (st["num_function_evaluations"], st["num_gradient_evaluations"]) == (Sr["counts"]["function"], Sr["counts"]["gradient"])
    assert st["num_line_search_steps"] == Sr["num_line_search_steps"] and st["line_search_seconds"] > 0.0
    # to the tolerances of test_gpu_frontend_matrix
    assert figures["cost"] <= cost_tol and abs(S.final_cost - (Sr["final_cost"] + fixed)) <= cost_tol * Sr["final_cost"]
    assert figures["radius"] <= 100.0 * cost_tol and figures["state"] <= 100.0 * cost_tol and figures["step_size"] <= 100.0 * cost_tol
    assert figures["gradient_max_norm_0"] <= 1e-12
    assert figures["final_vs_evaluate"] <= 1e-12
    # the box holds exactly; constant blocks come back bit-identical
    assert np.all(x >= ref["lower"]) and np.all(x <= ref["upper"])
    const = getattr(ref["pr"], "constant_state", np.zeros(0, dtype=np.int64))
    assert np.array_equal(x[const], ref["x0"][const])
    f = B.free_coordinates(ref["pr"])
    at = (x[f] == ref["lower"][f]) | (x[f] == ref["upper"][f])
    assert at.any() and np.array_equal(at, (xr[f] == ref["lower"][f]) | (xr[f] == ref["upper"][f]))


# ---- the kernels alone ---------------------------------------------------------------------------------------------------------------
def big_scene():
    """100 cameras, 90 000 points of two observations each (cameras q % 100 and (q + 37) % 100), random pixels: 270 900 state doubles,
    more than 2 x 512 x 256 — every thread of the plain kernels takes a second trip.  numpy only."""
    rng = np.random.default_rng(7)
    nc, npts = 100, 90000
    q = np.arange(npts)
    pt = np.repeat(q, 2).astype(np.int32)
    cam = np.stack([q % nc, (q + 37) % nc], axis=1).reshape(-1).astype(np.int32)
    obs = rng.uniform(-300.0, 300.0, (2 * npts, 2))
    state = np.concatenate([rng.normal(0.0, 1.0, 3 * npts) + np.tile([0.0, 0.0, -8.0], npts),
                            np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 500.0, 0.0, 0.0], nc) + rng.normal(0.0, 0.01, 9 * nc)])
    return nc, npts, cam, pt, obs, state


def kernel_handle(hip, oracle, which):
    """(handle, state, free state coordinates in tangent order)"""
    from test_gpu_line_search import tiny_scene
    if which in ("tiny", "tiny_constant"):
        sc = tiny_scene(oracle)
        cc, cp = ([1], [0, 5]) if which == "tiny_constant" else (None, None)
        camera = "angle_axis"
    elif which == "clean_quaternion":
        sc, cc, cp, camera = BC.scene(oracle), None, None, "quaternion"
    elif which == "clean_quaternion_constant":
        sc, cc, cp, camera = BC.scene(oracle), [0, 9], [0, 1, 199], "quaternion"
    else:
        sc, cc, cp, camera = big_scene(), None, None, "angle_axis"
    nc, npts = sc[0], sc[1]
    state = LC.initial_state(sc, camera)
    cs = 9 if camera == "angle_axis" else 10
    free = np.ones(state.size, bool)
    for c in cc or []:
        free[3 * npts + cs * c:3 * npts + cs * (c + 1)] = False
    for q in cp or []:
        free[3 * q:3 * q + 3] = False
    return device_problem(hip, sc, camera, cc=cc, cp=cp), state, np.flatnonzero(free)


@pytest.mark.parametrize("which", ["tiny", "tiny_constant", "clean_quaternion", "clean_quaternion_constant", "big"])
def test_kernels_against_numpy(hip, oracle, which):
    gp, x, f = kernel_handle(hip, oracle, which)
    try:
        rng = np.random.default_rng(11)
        n = x.size
        assert gp.num_effective_parameters == f.size
        v = rng.normal(0.0, 1.0, f.size) * (1.0 + np.abs(x[f]))
        # bounds: active in the first and the last 256 coordinates and at random elsewhere (a third below, a third above, the rest none
        # or far); the state itself partly outside (the projection moves it)
        kind = rng.integers(0, 4, n)
        kind[:256] = rng.integers(0, 2, min(256, n))
        kind[-256:] = rng.integers(0, 2, min(256, n))
        w = 0.2 * (1.0 + np.abs(x))
        lower = np.where(kind == 0, x + 0.5 * w * rng.uniform(-1.0, 1.0, n), np.where(kind == 2, -np.inf, x - 50.0 * w))
        upper = np.where(kind == 1, x + 0.5 * w * rng.uniform(-1.0, 1.0, n), np.where(kind == 2, np.inf, x + 50.0 * w))
        upper = np.maximum(upper, lower + 1e-3 * w)
        upper[kind == 3] = DBL_MAX   # (the other spelling of "none")
        gp.set_bounds(lower, upper)
        lo, hi = lower[f], np.where(upper[f] >= DBL_MAX, np.inf, upper[f])
        clamp = lambda a: np.minimum(np.maximum(a, lo), hi)   # noqa: E731
        # the projection
        want = x.copy()
        want[f] = clamp(x[f])
        moved = int(np.count_nonzero(want != x))
        assert moved > 0
        for _ in range(2):
            y, m = gp.project(x)
            assert np.array_equal(y, want) and m == moved
        close = lambda a, b: np.all(np.abs(a - b) <= 1e-14 * np.abs(b))   # noqa: E731
        pm_want = float(np.max(np.abs(x[f] - clamp(x[f] - v))))
        for t in (1.0, 0.3, 0.0):
            trial = x[f] + t * v
            out_want = x.copy()
            out_want[f] = clamp(trial)
            clamped = np.zeros(n, bool)
            clamped[f] = out_want[f] != trial
            runs = [gp.bounded_step(x, v, t) for _ in range(2)]
            out, xn, sn, pm = runs[0]
            assert np.array_equal(out, runs[1][0]) and runs[0][1:] == runs[1][1:]          # the same bits twice
            assert clamped[f].any() or t == 0.0
            assert np.array_equal(out[clamped], out_want[clamped])                        # clamped coordinates exactly
            assert close(out[~clamped], out_want[~clamped])
            rest = np.setdiff1d(np.arange(n), f)
            assert np.array_equal(out[rest], x[rest])                                     # constant blocks copied
            assert abs(xn - np.linalg.norm(x[f])) <= 1e-14 * np.linalg.norm(x[f])
            sn_want = float(np.linalg.norm(out_want[f] - x[f]))
            assert abs(sn - sn_want) <= 1e-14 * sn_want
            assert abs(pm - pm_want) <= 1e-14 * pm_want
    finally:
        gp.close()


# ---- handles no bound constrains ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,generic", [((5, 2), 1), ((3, 0), 1)], ids=["generic_path", "dense_schur"])
def test_an_unconstrained_handle_is_untouched(hip, oracle, solver, generic):
    """Bounds that constrain no free coordinate leave minimize the bits of a fresh handle.  Checked where two fresh handles give the same
    bits at all: force_generic_path, with ITERATIVE_SCHUR and with DENSE_SCHUR (test_gpu_fixed_intrinsics'
    test_zero_mask_is_the_constant_blocks_entry_point holds both to that).  On the fused path the sums in LDS differ in the last bits from
    one fresh handle to the next, bounds or none (test_gpu_frontend_matrix.EDGE_DEVICE_UNREPEATABLE; seen here too: DENSE_SCHUR on the
    fused path, the states of two handles equal to the eight digits printed and not to the bit)."""
    sc = BC.scene(oracle)
    cc, cp = [0], [0, 1, 2]
    x0 = LC.initial_state(sc, "angle_axis")
    n = x0.size
    const = np.concatenate([np.arange(9), 3 * sc[1] + np.arange(9)])
    inf = np.full(n, np.inf)
    on_constants_lo, on_constants_hi = -inf.copy(), inf.copy()
    on_constants_lo[const], on_constants_hi[const] = 1e3, 2e3   # (the values lie outside: never applied, never judged)
    box = (np.where(np.arange(n) % 2 == 0, x0 - 1.0, -np.inf), x0 + 1.0)

    def run(setup):
        gp = device_problem(hip, sc, "angle_axis", solver, generic, cc, cp)
        try:
            setup(gp)
            x, S = gp.minimize(x0, eta=1e-12, max_num_iterations=4)
            return x, S, gp.bounds_stats(), gp.project(x0)
        finally:
            gp.close()
    xa, Sa, _, _ = run(lambda gp: None)
    setups = {
        "infinite": lambda gp: gp.set_bounds(-inf, inf),
        "dbl_max": lambda gp: gp.set_bounds(np.full(n, -DBL_MAX), np.full(n, DBL_MAX)),
        "constant_blocks_only": lambda gp: gp.set_bounds(on_constants_lo, on_constants_hi),
        "set_then_cleared": lambda gp: (gp.set_bounds(*box), gp.set_bounds(None, None)),
        "one_side_none": lambda gp: gp.set_bounds(None, inf),
    }
    assert Sa.num_iterations_logged == 5
    for name, setup in setups.items():
        x, S, st, (xp, moved) = run(setup)
        assert np.array_equal(x, xa), name
        assert logged(S) == logged(Sa) and (S.initial_cost, S.final_cost, S.termination_type) == (Sa.initial_cost, Sa.final_cost, Sa.termination_type), name
        assert st["is_constrained"] == 0 and np.all(st["line_search_iterations"] == -1) and np.all(st["step_size"] == 1.0), name
        assert st["num_projected"] == 0 and st["num_function_evaluations"] == 0, name
        assert np.array_equal(xp, x0) and moved == 0, name


def test_bounds_that_never_bind(hip, oracle):
    name = "cubic_default"
    ref = BC.reference(oracle, name)
    x0 = ref["x0"]
    gp = case_problem(hip, ref, name, bounds=False)
    try:
        xa, Sa = gp.minimize(x0, eta=1e-12, max_num_iterations=8, jacobi_scaling=1)
        w = 1e3 * (1.0 + np.abs(x0))
        gp.set_bounds(x0 - w, x0 + w)
        x, S = gp.minimize(x0, eta=1e-12, max_num_iterations=8, jacobi_scaling=1)
        st = gp.bounds_stats()
    finally:
        gp.close()
    n = S.num_iterations_logged
    assert n == Sa.num_iterations_logged >= 3 and S.termination_type == Sa.termination_type   # (the run may converge before its eighth iteration)
    assert st["is_constrained"] == 1 and st["num_projected"] == 0
    valid = np.array([S.iterations[i].step_is_valid for i in range(1, n)], bool)
    assert valid.all()
    assert np.all(st["line_search_iterations"][1:n] == 0) and np.all(st["line_search_success"][1:n] == 1) and np.all(st["step_size"][:n] == 1.0)
    assert st["num_function_evaluations"] == st["num_gradient_evaluations"] == n - 1
    cost_tol = tolerances(BC.matrix_case(name))[0]
    for i in range(n):
        a, b = S.iterations[i], Sa.iterations[i]
        assert (a.step_is_valid, a.step_is_successful) == (b.step_is_valid, b.step_is_successful)
        assert abs(a.cost - b.cost) <= cost_tol * b.cost
    assert rel(x, xa) <= 100.0 * cost_tol


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def refused(hip, gp, call, code, *words):
    rc = call()
    msg = gp._lib.ceres_hip_bal_last_error(gp._h).decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_refusals_of_set_bounds(hip, oracle):
    ref = BC.reference(oracle, "quaternion_constant")   # cameras [0], points [0, 1, 2] constant; 10 doubles per camera
    sc, x0, lower, upper = ref["sc"], ref["x0"], ref["lower"], ref["upper"]
    npts = sc[1]
    gp = case_problem(hip, ref, "quaternion_constant", bounds=False)
    try:
        lib, n = gp._lib, x0.size
        p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(hip._DP)   # noqa: E731
        set_bounds = lambda lo, hi, o=None: lib.ceres_hip_bal_set_bounds(gp._h, p(lo), p(hi), None if o is None else hip.byref(o))   # noqa: E731
        c0 = gp.evaluate(x0)[0]
        bad = lower.copy()
        bad[3 * 7 + 1] = np.nan
        refused(hip, gp, lambda: set_bounds(bad, upper), hip.E_INVALID, "ceres_hip_bal_set_bounds", "NaN")
        # lower >= upper on a free block: refused, with the block, the index and both values (note the >=)
        k = 3 * npts + 10 * 4 + 7
        eq_lo, eq_hi = lower.copy(), upper.copy()
        eq_lo[k] = eq_hi[k] = 1.5
        refused(hip, gp, lambda: set_bounds(eq_lo, eq_hi), hip.E_INVALID, "ceres_hip_bal_set_bounds", "camera 4", "index: 7", "infeasible bound", "1.5")
        eq_lo[k], eq_hi[k] = lower[k], upper[k]
        eq_lo[3 * 5 + 2], eq_hi[3 * 5 + 2] = 2.0, -3.0
        refused(hip, gp, lambda: set_bounds(eq_lo, eq_hi), hip.E_INVALID, "point 5", "index: 2", "Lower bound: 2", "upper bound: -3")
        # ... on a constant block it is kept, never judged
        ok_lo, ok_hi = lower.copy(), upper.copy()
        ok_lo[0] = ok_hi[0] = x0[0]
        assert set_bounds(ok_lo, ok_hi) == 0 and set_bounds(None, None) == 0
        # a line-search field out of range, in ls_validate's words; the fields the search does not read are ignored
        for field, value, words in (("min_line_search_step_size", 0.0, ("min_line_search_step_size", "> 0.0")),
                                    ("max_line_search_step_contraction", 1.0, ("max_line_search_step_contraction", "< 1.0")),
                                    ("max_num_line_search_step_size_iterations", 0, ("max_num_line_search_step_size_iterations",)),
                                    ("line_search_interpolation_type", 7, ("line_search_interpolation_type",)),
                                    ("line_search_sufficient_function_decrease", 0.0, ("line_search_sufficient_function_decrease", "> 0.0"))):
            refused(hip, gp, lambda: set_bounds(lower, upper, hip.line_search_options(**{field: value})), hip.E_INVALID,
                    "ceres_hip_bal_set_bounds", "Invalid configuration", *words)
        ignored = hip.line_search_options(max_lbfgs_rank=-4, line_search_direction_type=hip.BFGS, max_num_iterations=-1,
                                          line_search_sufficient_curvature_decrease=7.0, max_line_search_step_expansion=0.0)
        assert set_bounds(lower, upper, ignored) == 0
        assert gp.bounds_stats()["is_constrained"] == 0   # (of the last minimize: none yet)
        # on a constrained handle
        refused(hip, gp, lambda: lib.ceres_hip_bal_minimize_line_search(gp._h, hip.byref(hip.line_search_options()), p(x0.copy()),
                                                                       hip.byref(hip.CLineSearchSummary())),
                hip.E_INVALID, "LINE_SEARCH Minimizer does not support bounds.")
        # evaluate, evaluate_gradient ignore bounds
        assert gp.evaluate(x0)[0] == c0 and gp.evaluate_gradient(x0)[0] == pytest.approx(c0, rel=1e-12)
        # a constant block infeasible at minimize: refused before any device call, the state untouched
        bad_lo, bad_hi = lower.copy(), upper.copy()
        kc = 3 * npts + 3   # camera 0 (constant), coordinate 3
        bad_lo[kc], bad_hi[kc] = x0[kc] + 1.0, x0[kc] + 2.0
        assert set_bounds(bad_lo, bad_hi) == 0
        xs = x0.copy()
        S = hip.CMinimizerSummary()
        o = hip.CMinimizerOptions()
        lib.ceres_hip_minimizer_default_options(hip.byref(o))
        refused(hip, gp, lambda: lib.ceres_hip_bal_minimize(gp._h, hip.byref(o), p(xs), hip.byref(S)), hip.E_INVALID, "ceres_hip_bal_minimize",
                "camera 0", "index: 3", "infeasible")
        msg = lib.ceres_hip_bal_last_error(gp._h).decode()
        numbers = [float(v) for v in re.findall(r"(?:Lower bound|value|upper bound): ([-+0-9.einfa]+?)(?:,|$)", msg)]
        assert numbers == [bad_lo[kc], x0[kc], bad_hi[kc]], msg
        assert np.array_equal(xs, x0)
        # the handle works on: the case's run, as a fresh handle gives it
        gp.set_bounds(lower, upper)
        x, S = gp.minimize(x0, eta=1e-12, max_num_iterations=2, jacobi_scaling=1)
        assert gp.bounds_stats()["is_constrained"] == 1 and S.final_cost < S.initial_cost
        its, fixed = ref["S"]["iterations"], ref["pr"].fixed_cost(x0)
        assert all(abs(S.iterations[i].cost - (its[i]["cost"] + fixed)) <= 1e-6 * its[i]["cost"] for i in range(3))
    finally:
        gp.close()


@pytest.mark.parametrize("kind", ["quaternion_manifold", "fixed_intrinsics"])
def test_handles_that_take_no_bounds(hip, oracle, kind):
    sc = BC.scene(oracle)
    nc, npts, cam, pt, obs, _ = sc
    o = hip.LinearSolverOptions(type=5, preconditioner_type=2, min_num_iterations=0, max_num_iterations=10000)
    if kind == "quaternion_manifold":
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model="quaternion_manifold")
        x0 = LC.initial_state(sc, "quaternion_manifold")
    else:
        gp = hip.BalProblem(o, nc, npts, cam, pt, obs, constant_intrinsics=["k1"])
        x0 = LC.initial_state(sc, "angle_axis")
    try:
        lo = x0 - 1.0
        p = lambda a: None if a is None else a.ctypes.data_as(hip._DP)   # noqa: E731
        for a, b in ((lo, None), (None, x0 + 1.0), (lo, x0 + 1.0)):
            refused(hip, gp, lambda: gp._lib.ceres_hip_bal_set_bounds(gp._h, p(a), p(b), None), hip.E_UNSUPPORTED, "ceres_hip_bal_set_bounds",
                    "not supported")
        assert gp._lib.ceres_hip_bal_set_bounds(gp._h, None, None, None) == 0   # clearing is no request
        x, S = gp.minimize(x0, max_num_iterations=2)
        assert S.final_cost < S.initial_cost and gp.bounds_stats()["is_constrained"] == 0
    finally:
        gp.close()


def test_inner_iterations_on_a_constrained_handle_are_refused(hip, oracle):
    ref = BC.reference(oracle, "cubic_default")
    gp = case_problem(hip, ref, "cubic_default")
    try:
        x0 = ref["x0"]
        gp.set_inner_iterations("automatic", 1e-3)
        xs = x0.copy()
        S, o = hip.CMinimizerSummary(), hip.CMinimizerOptions()
        gp._lib.ceres_hip_minimizer_default_options(hip.byref(o))
        refused(hip, gp, lambda: gp._lib.ceres_hip_bal_minimize(gp._h, hip.byref(o), xs.ctypes.data_as(hip._DP), hip.byref(S)), hip.E_UNSUPPORTED,
                "ceres_hip_bal_minimize", "inner iterations")
        c0, c1 = np.zeros(1), np.zeros(1)
        refused(hip, gp, lambda: gp._lib.ceres_hip_bal_inner_iterate(gp._h, xs.ctypes.data_as(hip._DP), c0.ctypes.data_as(hip._DP),
                                                                     c1.ctypes.data_as(hip._DP), None), hip.E_UNSUPPORTED,
                "ceres_hip_bal_inner_iterate", "bounds")
        assert np.array_equal(xs, x0)
        gp.set_inner_iterations(None, 1e-3)
        x, S = gp.minimize(x0, eta=1e-12, max_num_iterations=2, jacobi_scaling=1)
        its = ref["S"]["iterations"]
        assert all(abs(S.iterations[i].cost - its[i]["cost"]) <= 1e-6 * its[i]["cost"] for i in range(3))
        # cleared: inner iterations run again
        gp.set_bounds(None, None)
        gp.set_inner_iterations("automatic", 1e-3)
        x, S = gp.minimize(x0, max_num_iterations=2)
        assert gp.inner_iteration_stats()[0] >= 1 and gp.bounds_stats()["is_constrained"] == 0
    finally:
        gp.close()


# ---- poison ---------------------------------------------------------------------------------------------------------------------------
def child_main():
    """In the child interpreter (CERES_HIP_DEBUG_POISON=nan): cubic_default on a fresh handle; one JSON line."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hip = pkg.hip_solver
    hip.load_library()
    name = "cubic_default"
    sc, pr, x0, lower, upper = BC.setup(oracle, name)
    ref = dict(sc=sc, pr=pr, x0=x0, lower=lower, upper=upper)
    x, S, st, c = run_case(hip, ref, name)
    print(json.dumps(dict(x=x.tolist(), costs=[S.iterations[i].cost for i in range(S.num_iterations_logged)], final=S.final_cost, evaluate=c,
                          searches=[int(v) for v in st["line_search_iterations"][:S.num_iterations_logged]],
                          steps=[float(v) for v in st["step_size"][:S.num_iterations_logged]], projected=st["num_projected"])), flush=True)
    return 0


def test_poisoned_allocations_change_nothing(hip, oracle):
    name = "cubic_default"
    ref = BC.reference(oracle, name)
    x, S, st, c = run_case(hip, ref, name)
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_bounds as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr
    g = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    n = S.num_iterations_logged
    cost_tol = tolerances(BC.matrix_case(name))[0]
    assert np.all(np.isfinite(g["x"])) and np.all(np.isfinite(g["costs"]))
    assert g["searches"] == [int(v) for v in st["line_search_iterations"][:n]] and g["projected"] == st["num_projected"]
    assert len(g["costs"]) == n and max(abs(a - S.iterations[i].cost) / S.iterations[i].cost for i, a in enumerate(g["costs"])) <= cost_tol
    assert rel(np.array(g["x"]), x) <= 100.0 * cost_tol and abs(g["evaluate"] - g["final"]) <= 1e-12 * g["final"]
