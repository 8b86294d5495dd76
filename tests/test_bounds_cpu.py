"""tests/bounds_reference.py, the numpy restatement of ceres_hip_bal_minimize with bound constraints, held to things that do not depend
on it — frontend_reference.minimize where no bound constrains, the clamp and the projected gradient norm written out — and its runs on
the cases the device is compared on (tests/bounds_cases.py) held to be decided nowhere by rounding.  No device.

Measured on the table (the smallest recorded margin; the largest relative cost deviation under jacobian_noise = (1e-14, 1 and 2); the
searches): cubic_default 3.1e-5, 1.2e-14, searches of 1-2 iterations, one rejected step, 36 coordinates projected;
huber_first_sample 9.0e-4, 7.3e-14, every first sample accepted; quadratic 4.3e-5, 2.9e-14, up to 4 iterations, two rejected steps;
one_iteration 1.2e-2, 1.6e-13, five failed searches each followed by the rejected full clamped step; quaternion_constant 5.9e-6,
8.3e-15; quaternion_quadratic 4.3e-5, 2.4e-14; dogleg (4 iterations) 8.4e-4, 1.2e-10."""
import ctypes

import numpy as np
import pytest

import bounds_cases as BC
import bounds_reference as B
import frontend_reference as F
import line_search_cases as LC
from conftest import pkg
from test_gpu_frontend_matrix import tolerances

DBL_MAX = np.finfo(np.float64).max
ITERATION_NUMBERS = ("cost", "gradient_max_norm", "trust_region_radius", "relative_decrease")
ITERATION_FLAGS = ("step_is_valid", "step_is_successful", "branch", "solves", "linear_solver_iterations", "inner_step")


@pytest.fixture(scope="module")
def scene(oracle):
    return BC.scene(oracle)


# (the other spellings of "no bound" on one combination)
@pytest.mark.parametrize("strategy,camera,no_bound", [("lm", "angle_axis", "inf"), ("traditional", "angle_axis", "inf"),
                                                      ("lm", "quaternion", "inf"), ("traditional", "quaternion", "inf"),
                                                      ("lm", "angle_axis", "dbl_max"), ("lm", "angle_axis", "none")])
def test_without_a_constraining_bound_it_is_the_frontend_reference(oracle, scene, strategy, camera, no_bound):
    cc, cp = ([0], [0, 1, 2]) if camera == "quaternion" else (None, None)
    pr = LC.reference_problem(oracle, scene, camera, None, cc, cp)
    x0 = LC.initial_state(scene, camera)
    lower = {"inf": np.full(x0.size, -np.inf), "dbl_max": np.full(x0.size, -DBL_MAX), "none": None}[no_bound]
    upper = {"inf": np.full(x0.size, np.inf), "dbl_max": np.full(x0.size, DBL_MAX), "none": None}[no_bound]
    if cc:   # finite bounds on constant blocks alone constrain nothing (and are never applied, even where the value lies outside)
        lower, upper = lower.copy(), upper.copy()
        lower[pr.constant_state], upper[pr.constant_state] = 1e3, 2e3
    xr, Sr = F.minimize(pr, x0, strategy, max_num_iterations=3)
    x, S = B.minimize(pr, x0, lower, upper, strategy=strategy, max_num_iterations=3)
    assert S["is_constrained"] == 0 and S["num_projected"] == 0 and S["num_line_search_steps"] == 0
    assert np.array_equal(x, xr)
    assert (S["initial_cost"], S["final_cost"], S["termination_type"], S["num_linear_solves"]) == \
           (Sr["initial_cost"], Sr["final_cost"], Sr["termination_type"], Sr["num_linear_solves"])
    assert len(S["iterations"]) == len(Sr["iterations"]) == 4
    for a, b in zip(S["iterations"], Sr["iterations"]):
        assert [a.get(k) for k in ITERATION_NUMBERS + ITERATION_FLAGS] == [b.get(k) for k in ITERATION_NUMBERS + ITERATION_FLAGS]
        assert (a["line_search_iterations"], a["line_search_success"], a["step_size"]) == (-1, 0, 1.0)


def test_projection_and_projected_gradient_norm(oracle, scene):
    pr = LC.reference_problem(oracle, scene, "angle_axis", None, [0], [0, 1, 2])
    x = LC.initial_state(scene, "angle_axis")
    f = B.free_coordinates(pr)
    assert f.size == pr.n and np.intersect1d(f, pr.constant_state).size == 0
    rng = np.random.default_rng(3)
    lo, hi = x - rng.uniform(0.0, 1.0, x.size), x + rng.uniform(0.0, 1.0, x.size)
    inside = B.clamp(pr, x, lo, hi)
    assert np.array_equal(inside, x)
    moved = rng.choice(f, 40, replace=False)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[moved[:20]] = x[moved[:20]] + 0.5    # below the lower bound
    hi2[moved[:20]] = x[moved[:20]] + 1.0
    hi2[moved[20:]] = x[moved[20:]] - 0.5    # above the upper bound
    lo2[moved[20:]] = x[moved[20:]] - 1.0
    lo2[pr.constant_state], hi2[pr.constant_state] = 1e6, 2e6   # bounds on constant blocks: never applied
    y = B.clamp(pr, x, lo2, hi2)
    want = x.copy()
    want[moved[:20]] = lo2[moved[:20]]
    want[moved[20:]] = hi2[moved[20:]]
    assert np.array_equal(y, want) and np.array_equal(y[pr.constant_state], x[pr.constant_state])
    # the projected norm: |g|_inf where no bound is active (up to the rounding of x - (x - g)), smaller where a bound blocks -g
    _, _, _, g = pr.evaluate(x)
    none = np.full(x.size, np.inf)
    gmax = float(np.max(np.abs(g)))
    assert B.projected_gradient_max_norm(pr, x, g, -none, none) == pytest.approx(gmax, rel=1e-12)
    assert pr.gradient_max_norm(x, g) == gmax
    k = int(np.argmax(np.abs(g)))
    lo3, hi3 = -none.copy(), none.copy()
    if g[k] > 0:
        lo3[f[k]] = x[f[k]] - 0.25 * abs(g[k])   # x - g stops a quarter of the way
    else:
        hi3[f[k]] = x[f[k]] + 0.25 * abs(g[k])
    blocked = B.projected_gradient_max_norm(pr, x, g, lo3, hi3)
    second = float(np.sort(np.abs(g))[-2])
    assert blocked < gmax and blocked == pytest.approx(max(0.25 * gmax, second), rel=1e-12)
    assert B.is_constrained(pr, lo3, hi3, x.size) and not B.is_constrained(pr, -none, none, x.size)
    only_constants = (np.where(np.isin(np.arange(x.size), pr.constant_state), 0.0, -np.inf),
                      np.where(np.isin(np.arange(x.size), pr.constant_state), 1.0, np.inf))
    assert not B.is_constrained(pr, *only_constants, x.size)


def first_step(pr, x0, lower, upper):
    """The first iteration's pieces from the parts, not from bounds_reference.minimize: (projected x, cost, gradient, delta)."""
    lo, hi = B.normalized(pr, lower, upper, x0.size)
    x = B.clamp(pr, x0, lo, hi)
    cost, r, vals, g = pr.evaluate(x)
    J = pr.dense_jacobian(vals)
    scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
    o = F.DEFAULTS
    lm = F.LevenbergMarquardt(o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"], o["max_trust_region_radius"])
    _, step, _, _ = lm.compute_step(J * scale[None, :], r)
    return x, lo, hi, cost, g, step * scale


def test_the_search_gets_the_unprojected_derivative(oracle):
    ref = BC.reference(oracle, "cubic_default")
    x, lo, hi, cost, g, delta = first_step(ref["pr"], ref["x0"], ref["lower"], ref["upper"])
    it = ref["S"]["iterations"][1]
    assert it["line_search_derivative"] == float(g @ delta) and it["line_search_derivative"] < 0.0
    assert it["line_search_success"] == 1 and 0.0 < it["step_size"] < 1.0
    cand = B.clamp(ref["pr"], x + it["step_size"] * delta, lo, hi)
    assert it["step_norm"] == float(np.linalg.norm(x - cand)) and it["step_norm"] <= float(np.linalg.norm(it["step_size"] * delta))


def test_a_failed_search_leaves_delta_whole(oracle):
    ref = BC.reference(oracle, "one_iteration")
    x, lo, hi, cost, g, delta = first_step(ref["pr"], ref["x0"], ref["lower"], ref["upper"])
    it = ref["S"]["iterations"][1]
    assert (it["line_search_iterations"], it["line_search_success"], it["step_size"], it["step_is_successful"]) == (1, 0, 1.0, 0)
    cand = B.clamp(ref["pr"], x + delta, lo, hi)
    assert it["step_norm"] == float(np.linalg.norm(x - cand))
    assert it["cost"] == ref["pr"].cost(cand) > cost   # (a rejected step logs the candidate's cost)


def search_pattern(S):
    return [(i["step_is_valid"], i["step_is_successful"], i["line_search_iterations"], i["line_search_success"]) for i in S["iterations"]]


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_is_decided_nowhere_by_rounding(oracle, name):
    ref = BC.reference(oracle, name)
    S = ref["S"]
    margin = S["trace"].min_margin()
    assert {"armijo", "function_tolerance", "step_acceptance"} <= {n for n, _ in S["trace"].margins}
    deviation = 0.0
    for seed in BC.NOISE_SEEDS:
        _, Sn = BC.run_reference(ref["pr"], ref["x0"], ref["lower"], ref["upper"], name, jacobian_noise=(1e-14, seed))
        assert search_pattern(Sn) == search_pattern(S) and Sn["termination_type"] == S["termination_type"]
        assert (Sn["counts"], Sn["num_projected"], Sn["num_linear_solves"]) == (S["counts"], S["num_projected"], S["num_linear_solves"])
        deviation = max([deviation] + [abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(Sn["iterations"], S["iterations"])])
    print(f"{name}: smallest margin {margin:.2e}, largest cost deviation {deviation:.2e}, searches "
          f"{[(i['line_search_iterations'], i['line_search_success']) for i in S['iterations'][1:]]}")
    assert margin >= 1e-6                                               # test_line_search_cpu's rule
    assert 100.0 * deviation <= tolerances(BC.matrix_case(name))[0]     # test_gpu_frontend_matrix's rule
    assert S["is_constrained"] == 1 and len(S["iterations"]) == BC.CASES[name][6] + 1


def test_the_table_offers_every_pattern(oracle):
    runs = {name: BC.reference(oracle, name) for name in BC.CASES}
    its = [i for r in runs.values() for i in r["S"]["iterations"][1:]]
    assert any(i["line_search_iterations"] >= 2 for i in its)
    assert any(i["line_search_iterations"] == 0 and i["line_search_success"] for i in its)
    assert any(i["line_search_iterations"] >= 1 and not i["line_search_success"] for i in its)
    assert any(i["step_is_valid"] and not i["step_is_successful"] for i in its)
    assert all(r["S"]["num_projected"] > 0 for r in runs.values())
    for r in runs.values():
        x, lo, hi, npts = r["x"], r["lower"], r["upper"], r["sc"][1]
        at = (x == lo) | (x == hi)
        assert at[:3 * npts].any() and at[3 * npts:].any()
        f = B.free_coordinates(r["pr"])
        assert np.all(x[f] >= lo[f]) and np.all(x[f] <= hi[f])


def test_null_handle_calls_leave_a_message():
    hs = pkg.hip_solver
    lib = hs.load_library()
    one = np.zeros(4)
    n = ctypes.c_int64()
    p = one.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    calls = {
        "ceres_hip_bal_set_bounds": lambda: lib.ceres_hip_bal_set_bounds(None, p, p, None),
        "ceres_hip_bal_project": lambda: lib.ceres_hip_bal_project(None, p, ctypes.byref(n)),
        "ceres_hip_bal_bounds_stats": lambda: lib.ceres_hip_bal_bounds_stats(None, None, None, None, None, None, None, None, None, None),
        "ceres_hip_debug_bal_bounded_step": lambda: lib.ceres_hip_debug_bal_bounded_step(None, p, p, 1.0, p, p, p, p),
    }
    for name, call in calls.items():
        assert call() == hs.E_INVALID
        assert lib.ceres_hip_bal_last_error(None).decode() == f"{name}: NULL problem handle"
