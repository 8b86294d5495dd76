"""Numpy restatement of DoglegStrategy (internal/ceres/dogleg_strategy.cc) inside TrustRegionMinimizer::Minimize, statement by statement
as ceres_hip_bal_minimize runs it with ceres_hip_bal_set_trust_region_strategy(DOGLEG, ...): the Gauss-Newton solve dense (Cholesky of
J^T J + mu diag, a failed factorisation or a non-finite step raising mu), the quartic's roots from np.roots (companion-matrix
eigenvalues, real parts kept), and the subspace basis from a column-pivoting Householder QR.  Every iteration records which branch the
step took and how many linear solves it ran."""
import numpy as np

import inner_reference as IR
import robust_reference as R

MIN_MU, MAX_MU, MU_INCREASE = 1e-8, 1.0, 10.0


def poly_real_parts(poly):
    """FindPolynomialRoots' real parts (leading zeros dropped; np.roots drops them as well)."""
    p = np.asarray(poly, dtype=np.float64)
    if not np.all(np.isfinite(p)):
        return None
    return np.real(np.roots(p))


def boundary_minimum(B, g, radius):
    """FindMinimumOnTrustRegionBoundary + the cosine check: (code, x) with code 0, 1 (no valid root) or 2 (cosine < 0.99)."""
    B = np.asarray(B, dtype=np.float64).reshape(2, 2)
    g = np.asarray(g, dtype=np.float64)
    detB = B[0, 0] * B[1, 1] - B[1, 0] * B[0, 1]
    trB = B[0, 0] + B[1, 1]
    r2 = radius * radius
    adj = np.array([[B[1, 1], -B[0, 1]], [-B[1, 0], B[0, 0]]])
    poly = [r2, 2.0 * r2 * trB, r2 * (trB * trB + 2.0 * detB) - g @ g, -2.0 * (g @ adj @ g - r2 * detB * trB),
            r2 * detB * detB - (adj @ g) @ (adj @ g)]
    roots = poly_real_parts(poly)
    x = np.zeros(2)
    if roots is None:
        return 1, x
    best, valid = np.finfo(float).max, False
    for y in roots:
        with np.errstate(all="ignore"):
            try:
                xi = -np.linalg.solve(B + y * np.eye(2), g)
            except np.linalg.LinAlgError:
                continue
            nx = np.linalg.norm(xi)
            if nx > 0:
                xs = (radius / nx) * xi
                f = 0.5 * xs @ B @ xs + g @ xs
                valid = True
                if f < best:
                    best, x = f, xi
    if not valid:
        return 1, np.zeros(2)
    gm = B @ x + g
    cosine = -(x @ gm) / (np.linalg.norm(x) * np.linalg.norm(gm))
    if cosine < 0.99:
        return 2, x
    return 0, x


GRAM_FLOOR = 4.0 * np.sqrt(np.finfo(float).eps)


def pivoted_basis(gr, gn):
    """ColPivHouseholderQR of [gr, gn]: (rank, Q with 2 orthonormal columns).  Rank rule: |R_ii| > 2 eps max |R_jj|, with |R_22| taken
    as 0 at or below GRAM_FLOOR |second column| (columns within ~6e-8 rad of parallel: csrc/dogleg.inc forms R from the Gram matrix,
    where R_22 is rounding noise there)."""
    M = np.stack([gr, gn], axis=1)
    order = [1, 0] if gn @ gn > gr @ gr else [0, 1]
    Q, Rm = np.linalg.qr(M[:, order])
    d = np.abs(np.diag(Rm))
    if d[1] <= GRAM_FLOOR * np.linalg.norm(M[:, order[1]]):
        d[1] = 0.0
    rank = int(np.sum(d > 2.0 * np.finfo(float).eps * d.max())) if d.max() > 0 else 0
    return rank, Q


class Strategy:
    """DoglegStrategy's state and ComputeStep on a dense scaled Jacobian Js and residuals r (step in the minimizer's space)."""

    def __init__(self, kind, radius, min_diagonal, max_diagonal):
        self.kind, self.radius = kind, float(radius)
        self.min_d, self.max_d = min_diagonal, max_diagonal
        self.mu, self.reuse, self.step_norm = MIN_MU, False, 0.0

    def gauss_newton(self, Js, r):
        """ComputeGaussNewtonStep: (ok, solves)."""
        solves = 0
        ok = False
        while self.mu < MAX_MU:
            solves += 1
            A = Js.T @ Js + np.diag(self.diagonal ** 2 * self.mu)
            try:
                L = np.linalg.cholesky(A)
                y = np.linalg.solve(L.T, np.linalg.solve(L, Js.T @ r))
            except np.linalg.LinAlgError:
                y = None
            if y is None or not np.all(np.isfinite(y)):
                self.mu *= MU_INCREASE
                continue
            self.gn = -self.diagonal * y
            ok = True
            break
        return ok, solves

    def traditional(self):
        g, gn, r = self.gradient, self.gn, self.radius
        gnorm, gn_norm = np.linalg.norm(g), np.linalg.norm(gn)
        if gn_norm <= r:
            self.branch, self.step_norm = "gauss_newton", gn_norm
            return gn.copy()
        if gnorm * self.alpha >= r:
            self.branch, self.step_norm = "cauchy", r
            return -(r / gnorm) * g
        b_dot_a = -self.alpha * (g @ gn)
        a_sq = (self.alpha * gnorm) ** 2
        bma = a_sq - 2 * b_dot_a + gn_norm ** 2
        c = b_dot_a - a_sq
        d = np.sqrt(c * c + bma * (r ** 2 - a_sq))
        beta = (d - c) / bma if c <= 0 else (r * r - a_sq) / (d + c)
        step = (-self.alpha * (1.0 - beta)) * g + beta * gn
        self.branch = "dogleg_c_nonpositive" if c <= 0 else "dogleg_c_positive"
        self.step_norm = np.linalg.norm(step)
        return step

    def subspace(self):
        gn, r = self.gn, self.radius
        gn_norm = np.linalg.norm(gn)
        if gn_norm <= r:
            self.branch, self.step_norm = "gauss_newton", gn_norm
            return gn.copy()
        if self.one_dim:
            self.branch, self.step_norm = "subspace_1d", r
            return -(r / np.linalg.norm(self.gradient)) * self.gradient
        code, x = boundary_minimum(self.sB, self.sg, r)
        if code != 0:
            step = self.traditional()
            self.branch = "fallback_" + ("no_root" if code == 1 else "cosine") + ":" + self.branch
            return step
        self.branch, self.step_norm = "subspace_boundary", r
        return self.Q @ x

    def compute_step(self, Js, r):
        """(status, step in the minimizer's space, solves, linear_solver_iterations); status 'ok' or 'failure'."""
        if self.reuse:
            s = self.traditional() if self.kind == "traditional" else self.subspace()
            return "ok", s / self.diagonal, 0, 0
        self.reuse = True
        self.diagonal = np.sqrt(np.clip(np.sum(Js * Js, axis=0), self.min_d, self.max_d))
        self.gradient = (Js.T @ r) / self.diagonal
        Jg = Js @ (self.gradient / self.diagonal)
        self.alpha = (self.gradient @ self.gradient) / (Jg @ Jg)
        ok, solves = self.gauss_newton(Js, r)
        if not ok:
            self.branch = "failure"
            return "failure", None, solves, 0 if solves == 0 else 1
        if self.kind == "subspace":
            rank, Q = pivoted_basis(self.gradient, self.gn)
            if rank == 0:
                self.branch = "rank0"
                return "failure", None, solves, 1
            self.one_dim = rank == 1
            if not self.one_dim:
                self.Q = Q
                self.sg = Q.T @ self.gradient
                Jb = Js @ (Q / self.diagonal[:, None])
                self.sB = Jb.T @ Jb
        s = self.traditional() if self.kind == "traditional" else self.subspace()
        return "ok", s / self.diagonal, solves, 1

    def accepted(self, q):
        if q < 0.25:
            self.radius *= 0.5
        if q > 0.75:
            self.radius = max(self.radius, 3.0 * self.step_norm)
        self.mu = max(MIN_MU, 2.0 * self.mu / MU_INCREASE)
        self.reuse = False

    def rejected(self):
        self.radius *= 0.5
        self.reuse = True

    def invalid(self):
        self.mu *= MU_INCREASE
        self.reuse = False


def minimize(ev, x0, kind="traditional", inner=None, inner_iteration_tolerance=1e-3, **opts):
    """robust_reference.minimize with DoglegStrategy (and, with inner = (group, num_groups), inner_reference's
    DoInnerIterationsIfNeeded).  Per iteration also: branch, linear_solver_iterations, solves, mu; the summary has num_linear_solves."""
    o = dict(R.DEFAULTS)
    o.update(opts)
    x = np.array(x0, dtype=np.float64)
    n = ev.n
    strat = Strategy(kind, o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"])
    one_success, invalid_run, iteration, num_solves = False, 0, 0, 0
    inner_enabled = inner is not None
    scale = np.ones(n)
    its = []
    st = {}

    def eval_jacobian():
        cost, r, vals, gr = ev.evaluate(x)
        J = ev.dense_jacobian(vals)
        if o["jacobi_scaling"] and iteration == 0:
            scale[:] = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        st.update(cost=cost, r=r, Js=J * scale[None, :] if o["jacobi_scaling"] else J, grad_max=float(np.max(np.abs(gr))))

    eval_jacobian()
    S = dict(initial_cost=st["cost"], termination_type=R.NO_CONVERGENCE, iterations=[])
    its.append(dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius, step_is_valid=1,
                    step_is_successful=1, branch="initial", linear_solver_iterations=0, solves=0))
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = R.NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"]:
            S["termination_type"] = R.CONVERGENCE
            break
        if strat.radius <= o["min_trust_region_radius"]:
            S["termination_type"] = R.CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0)
        Js, r = st["Js"], st["r"]
        status, step, solves, lsi = strat.compute_step(Js, r)
        num_solves += solves
        it.update(branch=strat.branch, solves=solves, linear_solver_iterations=lsi, mu=strat.mu)
        mcc = np.nan
        if status == "ok":
            model = Js @ step
            mcc = -float(np.sum(model * (r + model / 2.0)))
        valid = status == "ok" and mcc > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            invalid_run += 1
            if invalid_run >= o["max_consecutive_invalid_steps"]:
                S["termination_type"] = R.FAILURE
                break
            strat.invalid()
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius)
            its.append(it)
            continue
        invalid_run = 0
        cand = x + step * scale if o["jacobi_scaling"] else x + step
        cand_cost = ev.cost(cand)
        inner_useful = False
        if inner_enabled and np.isfinite(cand_cost):
            xi, _ = IR.one_pass(ev, cand, inner[0], inner[1])
            ic = ev.cost(xi)
            if np.isfinite(ic):
                cand = xi
                mcc += cand_cost - ic
                inner_useful = ic < min(st["cost"], cand_cost)
                inner_enabled = (1.0 - ic / cand_cost) > inner_iteration_tolerance
                cand_cost = ic
        step_norm = float(np.linalg.norm(x - cand))
        if one_success and step_norm <= o["parameter_tolerance"] * (float(np.linalg.norm(x)) + o["parameter_tolerance"]):
            S["termination_type"] = R.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        if abs(st["cost"] - cand_cost) <= o["function_tolerance"] * st["cost"]:
            S["termination_type"] = R.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        if inner_useful or rel_dec > o["min_relative_decrease"]:
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
