"""numpy restatement of the line search minimizer (csrc/line_search.inc): the interpolating polynomial and its minimiser, the Armijo and
Wolfe line searches, the three search directions and LineSearchMinimizer's loop — after internal/ceres/polynomial.cc, line_search.cc,
line_search_direction.cc, low_rank_inverse_hessian.cc and line_search_minimizer.cc.

Every comparison that decides a branch records its RELATIVE MARGIN |a - b| / max(|a|, |b|) in a `Trace` (Armijo, both Wolfe tests,
f_k >= f_{k-1}, the sign of f', the secant test, d.g < 0, each termination test), and every line search records the phases it went
through, so that a test can assert that a run it compares with the device is decided nowhere by rounding.

The evaluators are the other front-end references' (robust_reference / quaternion_reference behind constant_blocks_reference.Problem:
cost, gradient = J^T r of their Jacobian, Plus)."""
import numpy as np

STEEPEST_DESCENT, NONLINEAR_CONJUGATE_GRADIENT, LBFGS, BFGS = 0, 1, 2, 3
FLETCHER_REEVES, POLAK_RIBIERE, HESTENES_STIEFEL = 0, 1, 2
ARMIJO, WOLFE = 0, 1
BISECTION, QUADRATIC, CUBIC = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2

DEFAULTS = dict(max_num_iterations=50, line_search_direction_type=LBFGS, nonlinear_conjugate_gradient_type=FLETCHER_REEVES,
                max_lbfgs_rank=20, use_approximate_eigenvalue_bfgs_scaling=0, line_search_type=WOLFE,
                line_search_interpolation_type=CUBIC, min_line_search_step_size=1e-9, line_search_sufficient_function_decrease=1e-4,
                max_line_search_step_contraction=1e-3, min_line_search_step_contraction=0.6,
                max_num_line_search_step_size_iterations=20, max_num_line_search_direction_restarts=5,
                line_search_sufficient_curvature_decrease=0.9, max_line_search_step_expansion=10.0, function_tolerance=1e-6,
                gradient_tolerance=1e-10, parameter_tolerance=1e-8)


class Trace:
    """The decisions of a run: (name, relative margin) of every comparison, and the phases of every line search."""

    def __init__(self):
        self.margins = []
        self.phases = []        # per line search: dict(bracket_iterations, zoom_iterations, first_sample_accepted, outcome)
        self.overwrites = 0     # L-BFGS: updates that replaced the oldest pair

    def test(self, name, a, b, result):
        m = abs(a - b) / max(abs(a), abs(b), 1e-300)
        self.margins.append((name, m))
        return result

    def min_margin(self):
        return min((m for _, m in self.margins), default=np.inf)


class Sample:
    def __init__(self, x=0.0, value=0.0, gradient=0.0, value_is_valid=False, gradient_is_valid=False):
        self.x, self.value, self.gradient = x, value, gradient
        self.value_is_valid, self.gradient_is_valid = value_is_valid, gradient_is_valid
        self.vector_x = None
        self.vector_gradient = None
        self.vector_gradient_is_valid = False


def evaluate_polynomial(poly, x):
    v = 0.0
    for c in poly:
        v = v * x + c
    return v


def find_interpolating_polynomial(samples):
    """Coefficients, highest power first: one equation per valid value / gradient; LU with full pivoting, threshold 0 — an exactly zero
    pivot ends the elimination, the unknowns left are 0."""
    nc = sum(int(s.value_is_valid) + int(s.gradient_is_valid) for s in samples)
    degree = nc - 1
    A, b = np.zeros((nc, nc)), np.zeros(nc)
    row = 0
    for s in samples:
        if s.value_is_valid:
            A[row, :] = [s.x ** (degree - j) for j in range(degree + 1)]
            b[row] = s.value
            row += 1
        if s.gradient_is_valid:
            A[row, :degree] = [(degree - j) * s.x ** (degree - j - 1) for j in range(degree)]
            b[row] = s.gradient
            row += 1
    col = list(range(nc))
    rank = 0
    for k in range(nc):
        sub = np.abs(A[k:, k:])
        i, j = np.unravel_index(np.argmax(sub), sub.shape)   # (first maximum in row-major order)
        if sub[i, j] == 0.0:
            break
        i, j = i + k, j + k
        if i != k:
            A[[k, i]] = A[[i, k]]
            b[[k, i]] = b[[i, k]]
        if j != k:
            A[:, [k, j]] = A[:, [j, k]]
            col[k], col[j] = col[j], col[k]
        for r in range(k + 1, nc):
            f = A[r, k] / A[k, k]
            A[r, k] = 0.0
            A[r, k + 1:] -= f * A[k, k + 1:]
            b[r] -= f * b[k]
        rank += 1
    y = np.zeros(nc)
    for i in range(rank - 1, -1, -1):
        y[i] = (b[i] - A[i, i + 1:rank] @ y[i + 1:rank]) / A[i, i]
    poly = np.zeros(nc)
    for i in range(rank):
        poly[col[i]] = y[i]
    return poly


def polynomial_roots_real_parts(poly):
    """The real parts of all roots (companion-matrix eigenvalues, as FindPolynomialRoots), leading zeros dropped."""
    p = np.trim_zeros(np.asarray(poly, dtype=np.float64), "f")
    if p.size <= 1:
        return np.zeros(0)
    return np.real(np.roots(p))


def _candidates_polynomial(poly, x_min, x_max):
    cands = [((x_min + x_max) / 2.0, None), (x_min, None), (x_max, None)]
    if len(poly) > 2:
        degree = len(poly) - 1
        der = [(degree - i) * poly[i] for i in range(degree)]
        if np.all(np.isfinite(der)):
            for r in polynomial_roots_real_parts(der):
                if x_min <= r <= x_max:
                    cands.append((float(r), None))
    return cands


def _pick(poly, cands):
    """The first strictly smallest value, in candidate order; also the margin to the best candidate at another x."""
    best_x, best_v = None, None
    vals = []
    for x, _ in cands:
        v = evaluate_polynomial(poly, x)
        vals.append((x, v))
        if best_v is None or v < best_v:
            best_x, best_v = x, v
    span = max(abs(c[0]) for c in cands) or 1.0
    others = [v for x, v in vals if abs(x - best_x) > 1e-9 * span]
    margin = min(((v - best_v) / max(abs(v), abs(best_v), 1e-300) for v in others), default=np.inf)
    return best_x, best_v, margin


def minimize_polynomial(poly, x_min, x_max):
    """(optimal_x, optimal_value): the midpoint, both ends, the real parts of ALL roots of the derivative inside the interval."""
    x, v, _ = _pick(poly, _candidates_polynomial(poly, x_min, x_max))
    return x, v


def minimize_interpolating_polynomial(samples, x_min, x_max, with_margin=False):
    poly = find_interpolating_polynomial(samples)
    cands = _candidates_polynomial(poly, x_min, x_max)
    cands += [(s.x, None) for s in samples if x_min <= s.x <= x_max]
    x, v, margin = _pick(poly, cands)
    return (x, v, poly, margin) if with_margin else (x, v)


def interpolating_step_size(kind, lowerbound, previous, current, min_step_size, max_step_size):
    if not current.value_is_valid or (kind == BISECTION and max_step_size <= current.x):
        return min(max(current.x * 0.5, min_step_size), max_step_size)
    if kind == BISECTION:
        return max_step_size
    samples = [lowerbound]
    if kind == QUADRATIC:
        samples.append(Sample(current.x, current.value, 0.0, True, False))
        if previous.value_is_valid:
            samples.append(Sample(previous.x, previous.value, 0.0, True, False))
    else:
        samples.append(current)
        if previous.value_is_valid:
            samples.append(previous)
    return minimize_interpolating_polynomial(samples, min_step_size, max_step_size)[0]


class SearchSummary:
    def __init__(self):
        self.success = False
        self.optimal_point = None
        self.num_function_evaluations = self.num_gradient_evaluations = self.num_iterations = 0
        self.error = ""


def _opt(o, k):
    return o.get(k, DEFAULTS[k])


def armijo(fn, o, initial, step_size_estimate, dmax, trace):
    """ArmijoLineSearch::DoSearch.  fn(x, want_gradient) -> Sample."""
    S = SearchSummary()
    kind = _opt(o, "line_search_interpolation_type")
    c1 = _opt(o, "line_search_sufficient_function_decrease")
    want = kind == CUBIC
    previous, ph = Sample(), dict(kind="armijo", bracket_iterations=0, zoom_iterations=0, first_sample_accepted=False, outcome="")
    trace.phases.append(ph)

    def ev(x):
        S.num_function_evaluations += 1
        S.num_gradient_evaluations += int(want)
        return fn(x, want)
    current = ev(step_size_estimate)
    while True:
        if current.value_is_valid:
            bound = initial.value + c1 * initial.gradient * current.x
            if not trace.test("armijo", current.value, bound, current.value > bound):
                break
        S.num_iterations += 1
        if S.num_iterations >= _opt(o, "max_num_line_search_step_size_iterations"):
            S.error, ph["outcome"] = "max_num_iterations", "failure_iterations"
            return S
        step = interpolating_step_size(kind, initial, previous, current, _opt(o, "max_line_search_step_contraction") * current.x,
                                       _opt(o, "min_line_search_step_contraction") * current.x)
        if trace.test("min_step_size", step * dmax, _opt(o, "min_line_search_step_size"), step * dmax < _opt(o, "min_line_search_step_size")):
            S.error, ph["outcome"] = "step_size too small", "failure_min_step_size"
            return S
        previous = current
        current = ev(step)
    ph["first_sample_accepted"] = S.num_iterations == 0
    ph["outcome"] = "accepted"
    S.optimal_point, S.success = current, True
    return S


def wolfe(fn, o, initial, step_size_estimate, dmax, trace):
    """WolfeLineSearch::DoSearch: the bracketing phase, then zoom."""
    S = SearchSummary()
    kind = _opt(o, "line_search_interpolation_type")
    c1, c2 = _opt(o, "line_search_sufficient_function_decrease"), _opt(o, "line_search_sufficient_curvature_decrease")
    max_it, min_step = _opt(o, "max_num_line_search_step_size_iterations"), _opt(o, "min_line_search_step_size")
    ph = dict(kind="wolfe", bracket_iterations=0, zoom_iterations=0, first_sample_accepted=False, outcome="")
    trace.phases.append(ph)

    def ev(x):
        S.num_function_evaluations += 1
        S.num_gradient_evaluations += 1
        return fn(x, True)
    # bracketing
    previous, current = initial, ev(step_size_estimate)
    bracket_low, bracket_high, do_zoom = initial, None, False
    while True:
        S.num_iterations += 1
        ph["bracket_iterations"] = S.num_iterations
        if current.value_is_valid:
            bound = initial.value + c1 * initial.gradient * current.x
            violated = trace.test("armijo", current.value, bound, current.value > bound)
            if not violated and previous.value_is_valid:
                violated = trace.test("f_k>f_k-1", current.value, previous.value, current.value > previous.value)
            if violated:
                do_zoom, bracket_low, bracket_high = True, previous, current
                break
            if trace.test("wolfe_curvature", abs(current.gradient), -c2 * initial.gradient, abs(current.gradient) <= -c2 * initial.gradient):
                bracket_low = bracket_high = current
                ph["first_sample_accepted"] = S.num_iterations == 1
                break
            if trace.test("sign_f'", current.gradient, 0.0, current.gradient >= 0):
                do_zoom, bracket_low, bracket_high = True, current, previous
                break
            if trace.test("bracket_width", abs(current.x - previous.x) * dmax, min_step, abs(current.x - previous.x) * dmax < min_step):
                bracket_low = current
                break
        if S.num_iterations >= max_it:   # (tested after the criteria above, valid sample or not)
            S.error = "bracketing: max_num_iterations"
            if current.value_is_valid and current.value < bracket_low.value:
                bracket_low = current
            ph["outcome"] = "armijo_only_iterations"
            break
        lo = current.x if current.value_is_valid else previous.x
        hi = current.x * _opt(o, "max_line_search_step_expansion") if current.value_is_valid else current.x
        step = interpolating_step_size(kind, previous, Sample(), current, lo, hi)
        if trace.test("min_step_size", step * dmax, min_step, step * dmax < min_step):
            S.error, ph["outcome"] = "step_size too small", "failure_min_step_size"
            return S
        if current.value_is_valid:
            previous = current
        current = ev(step)
    if do_zoom and abs(bracket_high.x - bracket_low.x) * dmax < min_step:
        do_zoom = False
    if not do_zoom:
        S.optimal_point, S.success = bracket_low, True
        ph["outcome"] = ph["outcome"] or "bracket_accepted"
        return S
    # zoom
    solution = Sample()
    nb = S.num_iterations
    ok = False
    if bracket_low.gradient * (bracket_high.x - bracket_low.x) >= 0:
        S.error, ph["outcome"] = "zoom: inconsistent bracket", "failure_bracket"
        return S
    while True:
        solution = bracket_low
        if S.num_iterations >= max_it:
            S.error = "zoom: max_num_iterations"
            break
        if abs(bracket_high.x - bracket_low.x) * dmax < min_step:
            S.error = "zoom: bracket width too small"
            break
        S.num_iterations += 1
        ph["zoom_iterations"] = S.num_iterations - nb
        lower, upper = (bracket_low, bracket_high) if bracket_low.x < bracket_high.x else (bracket_high, bracket_low)
        step = interpolating_step_size(kind, lower, Sample(), upper, lower.x, upper.x)
        solution = ev(step)
        if not solution.value_is_valid or not solution.gradient_is_valid:
            S.error = "zoom: invalid function"
            break
        bound = initial.value + c1 * initial.gradient * solution.x
        high = trace.test("armijo", solution.value, bound, solution.value > bound)
        if not high:
            high = trace.test("f>=f_low", solution.value, bracket_low.value, solution.value >= bracket_low.value)
        if high:
            bracket_high = solution
            continue
        if trace.test("wolfe_curvature", abs(solution.gradient), -c2 * initial.gradient, abs(solution.gradient) <= -c2 * initial.gradient):
            ok = True
            break
        v = solution.gradient * (bracket_high.x - bracket_low.x)
        if trace.test("sign_f'", v, 0.0, v >= 0):
            bracket_high = bracket_low
        bracket_low = solution
    if not ok and not solution.value_is_valid:
        ph["outcome"] = "failure_zoom"
        return S
    S.optimal_point = bracket_low if (not solution.value_is_valid or solution.value > bracket_low.value) else solution
    S.success = True
    ph["outcome"] = "zoom_accepted" if ok else "zoom_armijo_only"
    return S


def search(fn, o, initial_cost, initial_gradient, step_size_estimate, dmax=1.0, trace=None, initial=None):
    """LineSearch::Search on fn(x, want_gradient) -> Sample."""
    trace = trace if trace is not None else Trace()
    if initial is None:
        initial = Sample(0.0, initial_cost, initial_gradient, True, True)
    f = armijo if _opt(o, "line_search_type") == ARMIJO else wolfe
    return f(fn, o, initial, step_size_estimate, dmax, trace), trace


def univariate(f):
    """fn for `search` from f(x) -> (value, gradient) or None (invalid)."""
    def fn(x, want_gradient):
        s = Sample(x)
        r = f(x)
        if r is None or not np.isfinite(r[0]):
            return s
        s.value, s.value_is_valid = float(r[0]), True
        if want_gradient and np.isfinite(r[1]):
            s.gradient, s.gradient_is_valid, s.vector_gradient_is_valid = float(r[1]), True, True
        return s
    return fn


class LowRankInverseHessian:
    """L-BFGS: the secant test, the circular buffer, the two-loop recursion in the reference's order."""

    def __init__(self, rank, use_scaling, trace=None):
        self.rank, self.use_scaling, self.trace = rank, use_scaling, trace
        self.hist = []   # (delta_x, delta_gradient, s.y), oldest first
        self.scale = 1.0

    def update(self, dx, dg):
        sy = float(dx @ dg)
        skip = sy <= 1e-10
        if self.trace is not None:
            self.trace.test("secant", sy, 1e-10, skip)
        if skip:
            return False
        if len(self.hist) == self.rank:
            self.hist.pop(0)
            if self.trace is not None:
                self.trace.overwrites += 1
        self.hist.append((dx.copy(), dg.copy(), sy))
        self.scale = sy / float(dg @ dg)
        return True

    def direction(self, g):
        """-H g"""
        d = np.array(g, dtype=np.float64)
        alpha = []
        for s, y, sy in reversed(self.hist):
            a = float(s @ d) / sy
            d -= a * y
            alpha.append(a)
        if self.use_scaling:
            d *= self.scale
        for (s, y, sy), a in zip(self.hist, reversed(alpha)):
            b = float(y @ d) / sy
            d += s * (a - b)
        return -d


def minimize(pr, x0, **opts):
    """LineSearchMinimizer::Minimize on a problem with evaluate(x) -> (cost, residuals, values, gradient), cost(x), plus(x, delta),
    fixed_cost(x) (optional).  Returns (x, summary dict: iterations [dict], trace, counts, termination_type, message)."""
    o = dict(DEFAULTS)
    o.update(opts)
    trace = Trace()
    x = np.array(x0, dtype=np.float64)
    fixed = pr.fixed_cost(x) if hasattr(pr, "fixed_cost") else 0.0
    counts = dict(function=0, gradient=0)

    def evaluate(v):
        counts["function"] += 1
        counts["gradient"] += 1
        c, _, _, g = pr.evaluate(v)
        return float(c), np.asarray(g, dtype=np.float64)

    def norms(v, g):
        d = v - pr.plus(v, -g)
        return float(d @ d), float(np.max(np.abs(d)))
    cost, g = evaluate(x)
    g2, gmax = norms(x, g)
    S = dict(initial_cost=cost + fixed, termination_type=NO_CONVERGENCE, message="", trace=trace, counts=counts, num_line_search_steps=0,
             num_restarts=0, num_successful_steps=0)
    its = [dict(cost=cost + fixed, cost_change=0.0, gradient_max_norm=gmax, gradient_norm=np.sqrt(g2), step_norm=0.0, step_size=0.0)]
    S["iterations"] = its
    if trace.test("gradient_tolerance", gmax, o["gradient_tolerance"], gmax <= o["gradient_tolerance"]):
        S.update(termination_type=CONVERGENCE, message="Gradient tolerance reached.", final_cost=cost + fixed)
        return x, S
    kind = o["line_search_direction_type"]
    lb = LowRankInverseHessian(o["max_lbfgs_rank"], o["use_approximate_eigenvalue_bfgs_scaling"], trace)
    iteration, restarts = 0, 0
    prev = None   # dict(cost, g, g2, d, step_size)
    d = None
    while True:
        if iteration >= o["max_num_iterations"]:
            S["message"] = "Maximum number of iterations reached."
            break
        iteration += 1
        status = True
        if iteration == 1 or kind == STEEPEST_DESCENT:
            d = -g
        elif kind == LBFGS:
            lb.update(prev["d"] * prev["step_size"], g - prev["g"])
            d = lb.direction(g)
            dg = float(d @ g)
            if not trace.test("d.g<0", dg, 0.0, dg < 0.0):
                status = False
        else:
            t = o["nonlinear_conjugate_gradient_type"]
            if t == FLETCHER_REEVES:
                beta = g2 / prev["g2"]
            elif t == POLAK_RIBIERE:
                beta = float(g @ (g - prev["g"])) / prev["g2"]
            else:
                beta = float(g @ (g - prev["g"])) / float(prev["d"] @ (g - prev["g"]))
            d = -g + beta * prev["d"]
            dd = float(g @ d)
            if trace.test("ncg_restart", dd, -o["function_tolerance"], dd > -o["function_tolerance"]):
                d = -g
        if not status and restarts >= o["max_num_line_search_direction_restarts"]:
            S.update(termination_type=FAILURE, message="Line search direction failure")
            iteration -= 1
            break
        elif not status:
            restarts += 1
            lb = LowRankInverseHessian(o["max_lbfgs_rank"], o["use_approximate_eigenvalue_bfgs_scaling"], trace)
            d = -g
        dirderiv = float(g @ d)
        step0 = min(1.0, 1.0 / gmax) if (iteration == 1 or not status) else min(1.0, 2.0 * (cost - prev["cost"]) / dirderiv)
        if step0 < 0.0:
            S.update(termination_type=FAILURE, message="Numerical failure in line search, initial_step_size is negative")
            iteration -= 1
            break
        position, direction = x, d

        def fn(t, want_gradient):
            s = Sample(t)
            s.vector_x = pr.plus(position, t * direction)
            if want_gradient:
                c, gg = evaluate(s.vector_x)
            else:
                counts["function"] += 1
                c, gg = float(pr.cost(s.vector_x)), None
            if not np.isfinite(c):
                return s
            s.value, s.value_is_valid = c, True
            if want_gradient:
                s.gradient = float(direction @ gg)
                if np.isfinite(s.gradient):
                    s.gradient_is_valid = s.vector_gradient_is_valid = True
                    s.vector_gradient = gg
            return s
        initial = Sample(0.0, cost, dirderiv, True, True)
        initial.vector_x = x
        ls, _ = search(fn, o, cost, dirderiv, step0, float(np.max(np.abs(d))), trace, initial)
        trace.phases[-1]["iteration"] = iteration
        if not ls.success:
            S.update(termination_type=FAILURE, message="Numerical failure in line search, failed to find a valid step size")
            iteration -= 1
            break
        opt = ls.optimal_point
        prev = dict(cost=cost, g=g, g2=g2, d=d, step_size=opt.x)
        if opt.vector_gradient_is_valid:
            cost, g = opt.value, opt.vector_gradient
        else:
            cost, g = evaluate(opt.vector_x)
        g2, gmax = norms(opt.vector_x, g)
        step_norm = float(np.linalg.norm(opt.vector_x - x))
        free = np.setdiff1d(np.arange(x.size), pr.constant_state) if hasattr(pr, "constant_state") else slice(None)
        x_norm = float(np.linalg.norm(x[free]))
        x = opt.vector_x
        it = dict(cost=cost + fixed, cost_change=prev["cost"] - cost, gradient_max_norm=gmax, gradient_norm=np.sqrt(g2), step_norm=step_norm,
                  step_size=opt.x, line_search_function_evaluations=ls.num_function_evaluations,
                  line_search_gradient_evaluations=ls.num_gradient_evaluations, line_search_iterations=ls.num_iterations)
        its.append(it)
        S["num_line_search_steps"] += ls.num_iterations
        S["num_successful_steps"] += 1
        tol = o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"])
        if trace.test("parameter_tolerance", step_norm, tol, step_norm <= tol):
            S.update(termination_type=CONVERGENCE, message="Parameter tolerance reached.")
            break
        if trace.test("gradient_tolerance", gmax, o["gradient_tolerance"], gmax <= o["gradient_tolerance"]):
            S.update(termination_type=CONVERGENCE, message="Gradient tolerance reached.")
            break
        ftol = o["function_tolerance"] * abs(prev["cost"])
        if trace.test("function_tolerance", abs(it["cost_change"]), ftol, abs(it["cost_change"]) <= ftol):
            S.update(termination_type=CONVERGENCE, message="Function tolerance reached.")
            break
    S.update(final_cost=cost + fixed, num_iterations=iteration, num_restarts=restarts)
    return x, S
