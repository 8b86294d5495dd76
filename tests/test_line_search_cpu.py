"""The line search minimizer's host logic (csrc/line_search.inc) without a device: the numpy restatement (tests/line_search_reference.py)
against the reference's own unit-test answers (tests/golden/line_search_known_answers.json), the two host-only debug entries against
the restatement, the options' defaults and validation, and — on the restatement alone — the conditions that keep the GPU comparison
(tests/test_gpu_line_search.py) from passing on a degenerate run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import line_search_cases as C
import line_search_reference as LS

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = json.load(open(os.path.join(HERE, "golden", "line_search_known_answers.json")))


@pytest.fixture(scope="module")
def hs():
    from conftest import pkg
    pkg.hip_solver.load_library()
    return pkg.hip_solver


def samples_of(entry):
    return [LS.Sample(s["x"], s["value"] or 0.0, s["gradient"] or 0.0, s["value"] is not None, s["gradient"] is not None) for s in entry["samples"]]


# ---- 1. the restatement against the reference's unit tests ----
@pytest.mark.parametrize("entry", KNOWN["minimize_polynomial"], ids=lambda e: e["name"])
def test_restatement_minimize_polynomial_known_answers(entry):
    x, v = LS.minimize_polynomial(np.array(entry["polynomial"]), entry["x_min"], entry["x_max"])
    assert abs(v - entry["optimal_value"]) <= entry["tolerance"]
    if entry["optimal_x"] is None:
        assert entry["x_min"] <= x <= entry["x_max"]
    else:
        assert abs(x - entry["optimal_x"]) <= entry["tolerance"]


@pytest.mark.parametrize("entry", KNOWN["interpolating_polynomial"], ids=lambda e: e["name"])
def test_restatement_interpolating_polynomial_known_answers(entry):
    poly = LS.find_interpolating_polynomial(samples_of(entry))
    assert np.linalg.norm(poly - np.array(entry["polynomial"])) <= entry["tolerance"]


def test_restatement_line_search_minimizer_known_answer():
    """line_search_minimizer_test.cc FinalCostIsZero: f(x) = x^2 from x = 2 with the default options."""
    e = KNOWN["line_search_minimizer"][0]

    class Quadratic:
        def evaluate(self, x):
            return float(x[0] * x[0]), None, None, np.array([2.0 * x[0]])

        def cost(self, x):
            return float(x[0] * x[0])

        def plus(self, x, d):
            return x + d
    _, S = LS.minimize(Quadratic(), [e["initial_x"]])
    assert abs(S["final_cost"] - e["final_cost"]) <= e["tolerance"]


# ---- 2. ceres_hip_debug_minimize_interpolating_polynomial == restatement ----
def device_minimum(hs, samples, x_min, x_max):
    return hs.debug_minimize_interpolating_polynomial([s.x for s in samples], [s.value for s in samples], [s.value_is_valid for s in samples],
                                                      [s.gradient for s in samples], [s.gradient_is_valid for s in samples], x_min, x_max)


@pytest.mark.parametrize("entry", KNOWN["interpolating_polynomial"], ids=lambda e: e["name"])
def test_debug_interpolating_polynomial_known_answers(hs, entry):
    _, _, coef = device_minimum(hs, samples_of(entry), -4.0, 4.0)
    assert np.linalg.norm(coef - np.array(entry["polynomial"])) <= entry["tolerance"]


@pytest.mark.parametrize("entry", KNOWN["minimize_polynomial"], ids=lambda e: e["name"])
def test_debug_minimize_polynomial_known_answers(hs, entry):
    """MinimizePolynomial through the entry: samples on the polynomial that determine it (degree + 1 values)."""
    poly = np.array(entry["polynomial"])
    xs = np.linspace(-3.0, 5.0, poly.size)
    samples = [LS.Sample(x, LS.evaluate_polynomial(poly, x), 0.0, True, False) for x in xs]
    x, v, coef = device_minimum(hs, samples, entry["x_min"], entry["x_max"])
    assert np.max(np.abs(coef - poly)) <= 1e-12 * np.max(np.abs(poly))
    assert abs(v - entry["optimal_value"]) <= 1e-12
    if entry["optimal_x"] is not None:
        assert abs(x - entry["optimal_x"]) <= 1e-12


def random_sample_sets():
    """200 sets of 2-3 samples in the validity patterns the three interpolation types produce: QUADRATIC (gradient at the lower bound
    only), CUBIC (gradients everywhere), CUBIC with one sample whose value is valid and whose gradient is not (what the Armijo search
    passes on when d . g of a trial point is not finite), and the deficient case (a cubic fit to data of a quadratic)."""
    rng = np.random.default_rng(2024)
    sets = []
    patterns = ("quadratic", "cubic", "deficient", "cubic_missing_gradient")
    for k in range(200):
        pattern = patterns[k % 4 if k % 7 else 2]
        n = 3 if pattern == "cubic_missing_gradient" else 2 + (k // 4) % 2
        xs = np.sort(rng.uniform(0.0, 4.0, n))
        xs[0] = 0.0 if k % 3 else xs[0]
        if pattern == "deficient":
            a, b, c = rng.uniform(0.5, 2.0), rng.uniform(-4.0, -0.5), rng.uniform(0.0, 3.0)   # exact in binary: integers scaled
            a, b, c = float(np.round(a * 4) / 4), float(np.round(b * 4) / 4), float(np.round(c * 4) / 4)
            xs = np.array([0.0, 1.0, 2.0][:n])
            samples = [LS.Sample(x, a * x * x + b * x + c, 2 * a * x + b, True, True) for x in xs]
        else:
            vals = rng.uniform(-1.0, 1.0, n) + (xs - 1.5) ** 2
            grads = 2 * (xs - 1.5) + rng.uniform(-0.5, 0.5, n)
            missing = 1 + (k // 4) % 2 if pattern == "cubic_missing_gradient" else -1   # (the current or the previous sample)
            samples = [LS.Sample(xs[i], vals[i], grads[i], True, i == 0 if pattern == "quadratic" else i != missing) for i in range(n)]
        lo, hi = sorted(rng.uniform(0.0, 4.0, 2))
        sets.append((pattern, samples, float(lo), float(hi) + 0.1))
    return sets


def test_debug_interpolating_polynomial_random_sets(hs):
    decided = 0
    sets = random_sample_sets()
    for pattern, samples, lo, hi in sets:
        xr, vr, poly, margin = LS.minimize_interpolating_polynomial(samples, lo, hi, with_margin=True)
        x, v, coef = device_minimum(hs, samples, lo, hi)
        assert np.max(np.abs(coef - poly)) <= 1e-10 * np.max(np.abs(poly)), (pattern, coef, poly)
        if margin >= 1e-9:
            # (the same candidate wins on both sides, but not to the bit: the restatement finds the derivative's roots with np.roots — the
            # companion matrix's eigenvalues — and the library with the closed forms and the Aberth-Ehrlich iteration of dogleg.inc, so a
            # root candidate agrees to the root finders' accuracy, 1e-9 of the interval at the most for these quartics at most)
            decided += 1
            assert abs(x - xr) <= 1e-9 * max(abs(xr), hi - lo), (pattern, x, xr, margin)
    assert decided >= 0.9 * len(sets), decided


# ---- 3. ceres_hip_debug_line_search == restatement ----
def f_quadratic(x):
    return (x - 3.0) ** 2 + 1.0, 2.0 * (x - 3.0)


def f_nocedal_wright(x):
    return -x / (x * x + 2.0), (x * x - 2.0) / (x * x + 2.0) ** 2


def f_far_minimum(x):   # the minimum lies at 50 x the initial step of 1
    return (x - 50.0) ** 2 / 50.0, 2.0 * (x - 50.0) / 50.0


def f_needs_zoom(x):   # steep walls: the first sample overshoots into the far wall
    return (x - 0.3) ** 4 * 40.0 + (x - 0.3) ** 2, 160.0 * (x - 0.3) ** 3 + 2.0 * (x - 0.3)


def f_invalid_beyond(x):   # not defined beyond 0.7: the step is halved
    if x > 0.7:
        return None
    return (x - 0.5) ** 2, 2.0 * (x - 0.5)


def f_flat_descent(x):   # concave, ever descending and ever steeper: no Wolfe point, bracketing runs out of iterations
    return -x - 0.01 * x * x, -1.0 - 0.02 * x


def f_wall(x):   # rises at once from every positive step although f'(0) < 0 says otherwise: no step survives
    return (abs(x) ** 0.5) - 1e-3 * x if x > 0 else 0.0, -1.0


FUNCTIONS = {"quadratic": (f_quadratic, 1.0), "nocedal_wright": (f_nocedal_wright, 1.0), "far_minimum": (f_far_minimum, 1.0),
             "needs_zoom": (f_needs_zoom, 1.0), "invalid_beyond": (f_invalid_beyond, 1.0), "flat_descent": (f_flat_descent, 1.0),
             "wall": (f_wall, 1.0)}
SEARCHES = [(t, i) for t in (LS.ARMIJO, LS.WOLFE) for i in (LS.BISECTION, LS.QUADRATIC, LS.CUBIC)]


def search_options(kind, interpolation, name):
    o = dict(line_search_type=kind, line_search_interpolation_type=interpolation)
    if interpolation == LS.BISECTION:   # the contraction factors BISECTION needs: 0.5 must lie between them
        o.update(max_line_search_step_contraction=1e-3, min_line_search_step_contraction=0.5)
    if name == "flat_descent":
        o.update(max_num_line_search_step_size_iterations=4)
    return o


def both(hs, name, kind, interpolation):
    f, step = FUNCTIONS[name]
    o = search_options(kind, interpolation, name)
    f0, g0 = f(0.0)
    S, trace = LS.search(LS.univariate(f), o, f0, g0, step)

    def fn(x, want_gradient):
        return f(x)
    D = hs.debug_line_search(fn, step, f0, g0, **o)
    return S, trace, D


@pytest.mark.parametrize("name", list(FUNCTIONS))
@pytest.mark.parametrize("kind,interpolation", SEARCHES, ids=lambda v: str(v))
def test_debug_line_search_follows_the_restatement(hs, name, kind, interpolation):
    S, trace, D = both(hs, name, kind, interpolation)
    assert trace.min_margin() >= 1e-6, sorted(trace.margins, key=lambda m: m[1])[:3]
    assert bool(D.success) == S.success, D.error
    assert (D.num_function_evaluations, D.num_gradient_evaluations, D.num_iterations) == \
        (S.num_function_evaluations, S.num_gradient_evaluations, S.num_iterations)
    if S.success:
        assert abs(D.optimal_step_size - S.optimal_point.x) <= 1e-12 * abs(S.optimal_point.x)
    else:
        assert D.error


def test_the_line_search_cases_cover_every_path():
    """On the restatement alone: the set above contains an accept at the first sample, a bracket followed by zoom, an expansion over at
    least two bracketing iterations, the Armijo-only fallback with the iterations exhausted, and a failure by min_step_size."""
    seen = set()
    for name in FUNCTIONS:
        for kind, interpolation in SEARCHES:
            f, step = FUNCTIONS[name]
            f0, g0 = f(0.0)
            S, trace = LS.search(LS.univariate(f), search_options(kind, interpolation, name), f0, g0, step)
            ph = trace.phases[-1]
            if ph["first_sample_accepted"]:
                seen.add("first_sample")
            if ph["kind"] == "wolfe" and ph["zoom_iterations"] > 0 and S.success:
                seen.add("bracket_then_zoom")
            if ph["kind"] == "wolfe" and ph["bracket_iterations"] >= 2 and name == "far_minimum":   # expanded, over two bracketing iterations
                seen.add("expansion")
            if ph["outcome"] == "armijo_only_iterations" and S.success:
                seen.add("armijo_only_fallback")
            if ph["outcome"] == "failure_min_step_size" and not S.success:
                seen.add("min_step_size")
    assert seen == {"first_sample", "bracket_then_zoom", "expansion", "armijo_only_fallback", "min_step_size"}, seen


# ---- 4. options ----
def test_default_options(hs):
    o = hs.line_search_options()
    for k, v in LS.DEFAULTS.items():
        assert getattr(o, k) == v, k


INVALID = {
    "lbfgs_with_armijo": dict(line_search_type=LS.ARMIJO),
    "rank_zero": dict(max_lbfgs_rank=0),
    "min_step_size_zero": dict(min_line_search_step_size=0.0),
    "max_contraction_zero": dict(max_line_search_step_contraction=0.0),
    "max_contraction_one": dict(max_line_search_step_contraction=1.0, min_line_search_step_contraction=1.0),
    "contraction_bounds_out_of_order": dict(max_line_search_step_contraction=0.7, min_line_search_step_contraction=0.6),
    "min_contraction_above_one": dict(min_line_search_step_contraction=1.5),
    "no_step_size_iterations": dict(max_num_line_search_step_size_iterations=0),
    "decrease_zero": dict(line_search_sufficient_function_decrease=0.0),
    "curvature_not_above_decrease": dict(line_search_sufficient_curvature_decrease=1e-4),
    "curvature_one": dict(line_search_sufficient_curvature_decrease=1.0),
    "expansion_one": dict(max_line_search_step_expansion=1.0),
    "bisection_min_contraction": dict(line_search_interpolation_type=LS.BISECTION, min_line_search_step_contraction=0.4),
    "bisection_max_contraction": dict(line_search_interpolation_type=LS.BISECTION, max_line_search_step_contraction=0.55,
                                      min_line_search_step_contraction=0.6),
}

CHILD = r"""
import ctypes, sys
sys.path.insert(0, %(root)r)
import __graft_entry__ as entry
hs = entry.load_package().hip_solver
lib = hs.load_library()
import json
cases = json.loads(%(cases)r)
out = {}
S = hs.CLineSearchSummary()
x = (ctypes.c_double * 4)()
# (a NULL handle throughout: the options are validated before the handle is looked at, and no device is touched)
for name, fields in cases.items():
    o = hs.line_search_options(**fields)
    rc = lib.ceres_hip_bal_minimize_line_search(None, ctypes.byref(o), x, ctypes.byref(S))
    out[name] = [rc, lib.ceres_hip_bal_last_error(None).decode()]
o = hs.line_search_options()
out["null_handle"] = [lib.ceres_hip_bal_minimize_line_search(None, ctypes.byref(o), x, ctypes.byref(S)), lib.ceres_hip_bal_last_error(None).decode()]
# (options, state and summary NULL in turn; the options are read first of all, so each NULL must be caught before that)
out["null_options"] = [lib.ceres_hip_bal_minimize_line_search(None, None, x, ctypes.byref(S)), lib.ceres_hip_bal_last_error(None).decode()]
out["null_state"] = [lib.ceres_hip_bal_minimize_line_search(None, ctypes.byref(o), None, ctypes.byref(S)), lib.ceres_hip_bal_last_error(None).decode()]
out["null_summary"] = [lib.ceres_hip_bal_minimize_line_search(None, ctypes.byref(o), x, None), lib.ceres_hip_bal_last_error(None).decode()]
cost = ctypes.c_double()
out["null_handle_gradient"] = [lib.ceres_hip_bal_evaluate_gradient(None, x, ctypes.byref(cost), None), lib.ceres_hip_bal_last_error(None).decode()]
out["null_state_gradient"] = [lib.ceres_hip_bal_evaluate_gradient(None, None, ctypes.byref(cost), None), lib.ceres_hip_bal_last_error(None).decode()]
out["null_cost_gradient"] = [lib.ceres_hip_bal_evaluate_gradient(None, x, None, None), lib.ceres_hip_bal_last_error(None).decode()]
R = hs.CLineSearchResult()
out["null_function"] = [lib.ceres_hip_debug_line_search(ctypes.byref(o), None, None, 1.0, 1.0, -1.0, ctypes.byref(R)),
                        lib.ceres_hip_bal_last_error(None).decode()]
out["null_samples"] = [lib.ceres_hip_debug_minimize_interpolating_polynomial(2, None, None, None, None, None, 0.0, 1.0, None, None, None),
                       lib.ceres_hip_bal_last_error(None).decode()]
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def refusals():
    """Every refusal that needs no live handle, collected in ONE child process (a NULL pointer handled wrongly would take the process
    down, as in tests/test_abi_cpu.py)."""
    cases = dict(INVALID)
    cases["bfgs"] = dict(line_search_direction_type=LS.BFGS)
    code = CHILD % dict(root=os.path.dirname(HERE), cases=json.dumps(cases))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_null_arguments_are_refused_with_a_message(refusals):
    """Every pointer of the two problem entries NULL in turn (without a device the handle is NULL throughout; the same calls on a live
    handle: tests/test_gpu_line_search.py), and the debug entries' function and sample arrays.  The message names what was NULL."""
    named = {"null_handle": "NULL problem handle", "null_options": "NULL options", "null_state": "NULL state", "null_summary": "NULL summary",
             "null_handle_gradient": "NULL problem handle", "null_state_gradient": "NULL state", "null_cost_gradient": "NULL cost",
             "null_function": "NULL", "null_samples": "NULL"}
    for name, what in named.items():
        rc, msg = refusals[name]
        assert rc == -1 and what in msg, (name, rc, msg)


@pytest.mark.parametrize("name", list(INVALID))
def test_invalid_options_are_refused_before_any_device_call(refusals, name):
    """LineSearchOptionsAreValid's rules on ceres_hip_bal_minimize_line_search itself: CERES_HIP_E_INVALID, Ceres' wording."""
    rc, msg = refusals[name]
    assert rc == -1, (rc, msg)
    if name == "lbfgs_with_armijo":
        assert "When using (L)BFGS, Solver::Options::line_search_type must be set to WOLFE." in msg
    elif name.startswith("bisection"):
        assert "BISECTION" in msg and "prevent bisection (0.5) scaling" in msg
    else:
        assert "Invalid configuration. Solver::Options::" in msg and "Violated constraint: Solver::Options::" in msg, msg


def test_bfgs_is_unsupported_and_names_lbfgs(refusals):
    rc, msg = refusals["bfgs"]
    assert rc == -2 and "L-BFGS" in msg, (rc, msg)


# ---- 5. the GPU comparison's scenes are not degenerate (the restatement alone) ----
@pytest.fixture(scope="module")
def reference_runs(oracle):
    return {name: C.run_reference(oracle, name) for name in C.CASES}


@pytest.mark.parametrize("name", list(C.CASES))
def test_compared_runs_are_decided_with_a_margin_and_take_every_phase(reference_runs, name):
    offers = C.CASES[name][-1]
    _, _, _, (_, S) = reference_runs[name]
    trace = S["trace"]
    assert S["num_iterations"] == C.COMPARED_ITERATIONS
    assert trace.min_margin() >= 1e-6, sorted(trace.margins, key=lambda m: m[1])[:3]
    assert S["final_cost"] <= 0.9 * S["initial_cost"]
    if offers == "armijo":   # no bracketing and no zoom in an Armijo search: a contraction and a first-sample accept instead
        assert any(not p["first_sample_accepted"] for p in trace.phases) and any(p["first_sample_accepted"] for p in trace.phases)
        return
    assert any(p["zoom_iterations"] > 0 for p in trace.phases)
    if offers == "expansion":
        assert any(p["bracket_iterations"] > 1 for p in trace.phases)
    else:
        assert any(p["first_sample_accepted"] for p in trace.phases)


def test_rank_3_run_overwrites_the_circular_buffer(reference_runs):
    assert reference_runs["lbfgs_rank3_scaling"][3][1]["trace"].overwrites >= 1


def test_zero_step_run_hands_the_initial_position_back(oracle):
    """The run of line_search_cases.ZERO_STEP_CASES on the restatement alone: its only line search brackets at the first sample, has no
    zoom iteration left and returns the initial position — a step of zero, one more evaluation, the parameter tolerance."""
    _, _, x0, (x, S) = C.run_reference(oracle, "lbfgs_zero_step")
    ph = S["trace"].phases[-1]
    assert S["num_iterations"] == 1 and S["termination_type"] == LS.CONVERGENCE and S["message"].startswith("Parameter tolerance")
    assert (ph["bracket_iterations"], ph["zoom_iterations"], ph["outcome"]) == (1, 0, "zoom_armijo_only")
    assert S["iterations"][-1]["step_size"] == 0.0 and S["iterations"][-1]["step_norm"] == 0.0 and np.array_equal(x, x0)
    assert S["counts"] == dict(function=3, gradient=3)
    assert S["trace"].min_margin() >= 1e-6
