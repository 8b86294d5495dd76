"""A numpy restatement of ceres_hip_bal_minimize on a handle with bound constraints (csrc/bounds.inc; Problem::SetParameterLowerBound /
SetParameterUpperBound): TrustRegionMinimizer's loop with

  the projection         ParameterBlock::Plus clamps x_plus_delta to [lower, upper] (internal/ceres/parameter_block.h:227-255), on the
                         free blocks only; iteration zero projects the initial point (trust_region_minimizer.cc:210-220)
  the gradient norm      max |x - clamp(x - g)| (trust_region_minimizer.cc:281-302)
  the projected search   DoLineSearch (trust_region_minimizer.cc:596-641): ARMIJO on phi(a) = cost(clamp(x + a delta)), phi'(0) = g . delta
  the step norm          |x - candidate| in the ambient space (trust_region_minimizer.cc:726-748)

It works over the `Problem` interface of frontend_reference / constant_blocks_reference and composes frontend_reference.LevenbergMarquardt,
dogleg_reference.Strategy and line_search_reference.search (always with line_search_type = ARMIJO); it copies none of them.  Bounds that
constrain no free coordinate leave frontend_reference.minimize's loop, bit for bit (tests/test_bounds_cpu.py).  The decisions it adds
— the trust-region acceptance, the function tolerance, the parameter tolerance — record their relative margin in the line search's
`Trace`, beside the search's own (the Armijo test, the minimum step size)."""
import numpy as np

import dogleg_reference as DR
import frontend_reference as F
import line_search_reference as LS

DBL_MAX = np.finfo(np.float64).max
SEARCH_FIELDS = ("line_search_interpolation_type", "min_line_search_step_size", "line_search_sufficient_function_decrease",
                 "max_line_search_step_contraction", "min_line_search_step_contraction", "max_num_line_search_step_size_iterations")


def free_coordinates(pr):
    """The state coordinates of the free blocks, in the order of the tangent vector (bounds are only taken where Plus is x + delta:
    ambient and tangent offsets inside a block coincide)."""
    return np.asarray(pr.free_cols) if hasattr(pr, "free_cols") else np.arange(pr.n)


def normalized(pr, lower, upper, n):
    lo = np.full(n, -np.inf) if lower is None else np.where(np.asarray(lower, dtype=np.float64) <= -DBL_MAX, -np.inf, lower)
    hi = np.full(n, np.inf) if upper is None else np.where(np.asarray(upper, dtype=np.float64) >= DBL_MAX, np.inf, upper)
    return lo, hi


def is_constrained(pr, lower, upper, n):
    """Program::IsBoundsConstrained: a finite bound on a coordinate of a free block."""
    lo, hi = normalized(pr, lower, upper, n)
    f = free_coordinates(pr)
    return bool(np.any(np.isfinite(lo[f])) or np.any(np.isfinite(hi[f])))


def clamp(pr, x, lo, hi):
    """Plus(x, 0): std::max(x, lower) then std::min(., upper) on the free blocks; constant blocks untouched."""
    f = free_coordinates(pr)
    out = np.array(x, dtype=np.float64)
    out[f] = np.minimum(np.maximum(out[f], lo[f]), hi[f])
    return out


def projected_gradient_max_norm(pr, x, g, lo, hi):
    """max |x - clamp(x - g)| over the free blocks; g: the tangent gradient."""
    f = free_coordinates(pr)
    return float(np.max(np.abs(x[f] - np.minimum(np.maximum(x[f] - g, lo[f]), hi[f]))))


def line_search(pr, x, cost, g, delta, lo, hi, options, trace, counts=None):
    """DoLineSearch: returns (line_search_reference.SearchSummary, the derivative handed to the search)."""
    o = {k: v for k, v in options.items() if k in SEARCH_FIELDS}
    o["line_search_type"] = LS.ARMIJO
    counts = counts if counts is not None else dict(function=0, gradient=0)

    def fn(a, want_gradient):
        s = LS.Sample(a)
        s.vector_x = clamp(pr, pr.plus(x, a * delta), lo, hi)
        counts["function"] += 1
        if want_gradient:
            counts["gradient"] += 1
            c, _, _, gg = pr.evaluate(s.vector_x)
        else:
            c, gg = pr.cost(s.vector_x), None
        c = float(c)
        if not np.isfinite(c):
            return s
        s.value, s.value_is_valid = c, True
        if want_gradient:
            s.gradient = float(delta @ gg)
            if np.isfinite(s.gradient):
                s.gradient_is_valid = s.vector_gradient_is_valid = True
        return s
    derivative = float(g @ delta)
    summary, _ = LS.search(fn, o, cost, derivative, 1.0, float(np.max(np.abs(delta))), trace)
    return summary, derivative


def minimize(pr, x0, lower=None, upper=None, strategy="lm", jacobian_noise=None, line_search_options=None, **opts):
    """ceres_hip_bal_minimize with bounds lower / upper (state layout; None, -inf / +inf or -+DBL_MAX: none).  Returns (x, summary):
    frontend_reference.minimize's summary and iteration dicts, plus is_constrained, num_projected, num_line_search_steps, counts
    (function / gradient evaluations of the searches), trace, and per iteration step_norm, line_search_iterations (-1: no search ran),
    line_search_success, step_size (1 where the search failed or did not run), line_search_derivative."""
    o = dict(F.DEFAULTS)
    o.update(opts)
    lso = dict(line_search_options or {})
    noise_rng = np.random.default_rng(jacobian_noise[1]) if jacobian_noise else None
    assert strategy in F.STRATEGIES, strategy
    x = np.array(x0, dtype=np.float64)
    lo, hi = normalized(pr, lower, upper, x.size)
    constrained = is_constrained(pr, lower, upper, x.size)
    trace = LS.Trace()
    counts = dict(function=0, gradient=0)
    if strategy == "lm":
        strat = F.LevenbergMarquardt(o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"], o["max_trust_region_radius"])
    else:
        strat = DR.Strategy(strategy, o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"])
    one_success, invalid_run, iteration, num_solves = False, 0, 0, 0
    scale = np.ones(pr.n)
    its, st = [], {}
    num_projected = 0
    if constrained:   # iteration zero: x = Plus(x, 0)
        xp = clamp(pr, x, lo, hi)
        num_projected = int(np.count_nonzero(xp != x))
        x = xp

    def eval_jacobian():
        cost, r, vals, g = pr.evaluate(x)
        if noise_rng is not None:
            vals = vals * (1.0 + jacobian_noise[0] * noise_rng.standard_normal(vals.shape))
        J = pr.dense_jacobian(vals)
        if o["jacobi_scaling"] and iteration == 0:
            scale[:] = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        gm = projected_gradient_max_norm(pr, x, g, lo, hi) if constrained else pr.gradient_max_norm(x, g)
        st.update(cost=cost, r=r, g=g, Js=J * scale[None, :] if o["jacobi_scaling"] else J, grad_max=gm)

    eval_jacobian()
    S = dict(initial_cost=st["cost"], termination_type=F.NO_CONVERGENCE, is_constrained=int(constrained), num_projected=num_projected,
             num_line_search_steps=0, counts=counts, trace=trace)
    none = dict(line_search_iterations=-1, line_search_success=0, step_size=1.0)
    its.append(dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius, step_is_valid=1,
                    step_is_successful=1, branch="initial", solves=0, linear_solver_iterations=0, inner_step=False, **none))
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = F.NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"] or strat.radius <= o["min_trust_region_radius"]:
            S["termination_type"] = F.CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0, inner_step=False, **none)
        Js, r = st["Js"], st["r"]
        status, step, solves, lsi = strat.compute_step(Js, r)
        num_solves += solves
        it.update(branch=strat.branch, solves=solves, linear_solver_iterations=lsi)
        mcc = np.nan
        if status == "ok":
            model = Js @ step
            mcc = -float(np.sum(model * (r + model / 2.0)))
        valid = status == "ok" and bool(np.all(np.isfinite(step))) and mcc > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            invalid_run += 1
            if invalid_run >= o["max_consecutive_invalid_steps"]:
                S["termination_type"] = F.FAILURE
                break
            strat.invalid()
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius)
            its.append(it)
            continue
        invalid_run = 0
        delta = step * scale if o["jacobi_scaling"] else step
        if constrained:
            # the projected search scales delta on success and leaves it whole on failure; the model cost change stays the full step's
            ls, derivative = line_search(pr, x, st["cost"], st["g"], delta, lo, hi, lso, trace, counts)
            S["num_line_search_steps"] += ls.num_iterations
            it.update(line_search_iterations=ls.num_iterations, line_search_success=int(ls.success), line_search_derivative=derivative,
                      line_search_function_evaluations=ls.num_function_evaluations, line_search_gradient_evaluations=ls.num_gradient_evaluations)
            if ls.success:
                it["step_size"] = ls.optimal_point.x
                delta = delta * ls.optimal_point.x
            cand = clamp(pr, pr.plus(x, delta), lo, hi)
            step_norm = float(np.linalg.norm(x - cand))
        else:
            cand = pr.plus(x, delta)
            step_norm = float(np.linalg.norm(delta))
        cand_cost = pr.cost(cand)
        it["step_norm"] = step_norm
        ptol = o["parameter_tolerance"] * (float(np.linalg.norm(x[free_coordinates(pr)] if constrained else x)) + o["parameter_tolerance"])
        if one_success and trace.test("parameter_tolerance", step_norm, ptol, step_norm <= ptol):
            S["termination_type"] = F.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        ftol = o["function_tolerance"] * st["cost"]
        if trace.test("function_tolerance", abs(st["cost"] - cand_cost), ftol, abs(st["cost"] - cand_cost) <= ftol):
            S["termination_type"] = F.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        it["relative_decrease"] = rel_dec
        if trace.test("step_acceptance", rel_dec, o["min_relative_decrease"], rel_dec > o["min_relative_decrease"]):
            x = cand
            one_success = True
            eval_jacobian()
            strat.accepted(rel_dec)
            it["step_is_successful"] = 1
        else:
            strat.rejected()
        it.update(cost=st["cost"] if it["step_is_successful"] else cand_cost, gradient_max_norm=st["grad_max"],
                  trust_region_radius=strat.radius)
        its.append(it)
    S["final_cost"] = st["cost"]
    S["iterations"] = its
    S["num_linear_solves"] = num_solves
    return x, S
