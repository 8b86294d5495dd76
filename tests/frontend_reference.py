"""One numpy restatement of ceres_hip_bal_minimize (csrc/bal_frontend.inc) with every option of the BAL front end at once: the camera
model, the loss, the trust-region strategy (Levenberg-Marquardt, traditional or subspace dogleg), inner iterations and Jacobi scaling.
It composes the per-feature restatements and copies none of them:

  the evaluators       robust_reference.Evaluator (angle-axis; Jacobian from oracle.snavely_batch) and quaternion_reference.Evaluator
                       (both quaternion models; complex-step Jacobian), behind `Problem`, which gives both one interface
  the LM step          robust_reference.minimize's, as `LevenbergMarquardt` with the interface of dogleg_reference.Strategy
  the dogleg step      dogleg_reference.Strategy
  inner iterations     inner_reference.one_pass / ordering, with the outer loop's bookkeeping of inner_reference.minimize

tests/test_frontend_reference_cpu.py holds it to each of those restatements within its own domain."""
import numpy as np

import dogleg_reference as DR
import inner_reference as IR
import quaternion_reference as Q
import robust_reference as R

STRATEGIES = ("lm", "traditional", "subspace")
DEFAULTS = R.DEFAULTS
CONVERGENCE, NO_CONVERGENCE, FAILURE = R.CONVERGENCE, R.NO_CONVERGENCE, R.FAILURE


class Problem:
    """robust_reference.Evaluator or quaternion_reference.Evaluator with one interface: evaluate, cost, dense_jacobian, plus(x, delta),
    gradient_max_norm(x, g) and n (the tangent size).  Angle-axis: Euclidean Plus, |g|_inf; quaternion models: the Evaluator's own
    Plus (QuaternionPlus on the manifold) and |x - Plus(x, -g)|_inf."""

    def __init__(self, ev):
        self.ev = ev
        self.quaternion = isinstance(ev, Q.Evaluator)
        self.n = ev.n_t if self.quaternion else ev.n

    def evaluate(self, x):
        return self.ev.evaluate(x)

    def cost(self, x):
        return self.ev.cost(x)

    def dense_jacobian(self, vals):
        return self.ev.dense_jacobian(vals)

    def plus(self, x, delta):
        return self.ev.plus(x, delta) if self.quaternion else x + delta

    def gradient_max_norm(self, x, g):
        return self.ev.gradient_max_norm(x, g) if self.quaternion else float(np.max(np.abs(g)))


def problem(snavely_batch, model, num_cameras, num_points, camera_index, point_index, observations, row_order, loss=None):
    """A Problem for camera model 0 (angle-axis), 1 (quaternion) or 2 (quaternion manifold)."""
    if model == 0:
        return Problem(R.Evaluator(snavely_batch, num_cameras, num_points, camera_index, point_index, observations, row_order, loss))
    return Problem(Q.Evaluator(model, num_cameras, num_points, camera_index, point_index, observations, row_order, loss))


class LevenbergMarquardt:
    """LevenbergMarquardtStrategy as robust_reference.minimize runs it (the solve dense and exact), with dogleg_reference.Strategy's
    interface: the radius and the decrease factor live here."""

    def __init__(self, radius, min_diagonal, max_diagonal, max_radius):
        self.radius, self.decrease_factor = float(radius), 2.0
        self.min_d, self.max_d, self.max_radius = min_diagonal, max_diagonal, max_radius
        self.reuse, self.diag, self.branch = False, None, "lm"

    def compute_step(self, Js, r):
        if not self.reuse:
            self.diag = np.clip(np.sum(Js * Js, axis=0), self.min_d, self.max_d)
        step = -np.linalg.solve(Js.T @ Js + np.diag(self.diag / self.radius), Js.T @ r)
        self.reuse = True
        return "ok", step, 1, 1

    def accepted(self, q):
        self.radius = min(self.max_radius, self.radius / max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3))
        self.decrease_factor = 2.0
        self.reuse = False

    def rejected(self):
        self.radius /= self.decrease_factor
        self.decrease_factor *= 2.0

    invalid = rejected


def minimize(ev, x0, strategy="lm", inner=None, inner_iteration_tolerance=1e-3, jacobian_noise=None, **opts):
    """TrustRegionMinimizer::Minimize, statement by statement as ceres_hip_bal_minimize runs it.  ev: a Problem; strategy: "lm",
    "traditional" or "subspace"; inner: (group, num_groups) of inner_reference.ordering, angle-axis only.  Returns (x, summary dict:
    initial_cost, final_cost, termination_type, num_linear_solves, num_inner_iteration_steps, inner_enabled_at_end, iterations: [dict(
    cost, step_is_successful, step_is_valid, trust_region_radius, gradient_max_norm, branch, solves, linear_solver_iterations,
    inner_step)]).

    jacobian_noise = (relative size, seed): every Jacobian value times 1 + size N(0, 1), a stand-in for the device's rounding (its
    Jacobian agrees with this one to ~1e-14): how far the trajectory moves under it measures how well a case is conditioned."""
    o = dict(DEFAULTS)
    noise_rng = np.random.default_rng(jacobian_noise[1]) if jacobian_noise else None
    o.update(opts)
    assert strategy in STRATEGIES, strategy
    assert inner is None or not ev.quaternion, "inner iterations are angle-axis only"
    x = np.array(x0, dtype=np.float64)
    if strategy == "lm":
        strat = LevenbergMarquardt(o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"],
                                   o["max_trust_region_radius"])
    else:
        strat = DR.Strategy(strategy, o["initial_trust_region_radius"], o["min_lm_diagonal"], o["max_lm_diagonal"])
    one_success, invalid_run, iteration, num_solves = False, 0, 0, 0
    inner_enabled, inner_steps = inner is not None, 0
    scale = np.ones(ev.n)
    its = []
    st = {}

    def eval_jacobian():
        cost, r, vals, g = ev.evaluate(x)
        if noise_rng is not None:
            vals = vals * (1.0 + jacobian_noise[0] * noise_rng.standard_normal(vals.shape))
        J = ev.dense_jacobian(vals)
        if o["jacobi_scaling"] and iteration == 0:
            scale[:] = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        st.update(cost=cost, r=r, Js=J * scale[None, :] if o["jacobi_scaling"] else J, grad_max=ev.gradient_max_norm(x, g))

    eval_jacobian()
    S = dict(initial_cost=st["cost"], termination_type=NO_CONVERGENCE)
    its.append(dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius, step_is_valid=1,
                    step_is_successful=1, branch="initial", solves=0, linear_solver_iterations=0, inner_step=False))
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"] or strat.radius <= o["min_trust_region_radius"]:
            S["termination_type"] = CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0, inner_step=False)
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
                S["termination_type"] = FAILURE
                break
            strat.invalid()
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=strat.radius)
            its.append(it)
            continue
        invalid_run = 0
        delta = step * scale if o["jacobi_scaling"] else step
        cand = ev.plus(x, delta)
        cand_cost = ev.cost(cand)
        inner_useful = False
        if inner_enabled and np.isfinite(cand_cost):   # DoInnerIterationsIfNeeded
            inner_steps += 1
            it["inner_step"] = True
            xi, _ = IR.one_pass(ev.ev, cand, inner[0], inner[1])
            ic = ev.cost(xi)
            if np.isfinite(ic):
                cand = xi
                mcc += cand_cost - ic
                inner_useful = ic < min(st["cost"], cand_cost)
                inner_enabled = (1.0 - ic / cand_cost) > inner_iteration_tolerance
                cand_cost = ic
        # |x - candidate| where inner iterations are set, else the tangent |delta| (ceres_hip_bal_minimize's step norm)
        step_norm = float(np.linalg.norm(x - cand)) if inner is not None else float(np.linalg.norm(delta))
        if one_success and step_norm <= o["parameter_tolerance"] * (float(np.linalg.norm(x)) + o["parameter_tolerance"]):
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        if abs(st["cost"] - cand_cost) <= o["function_tolerance"] * st["cost"]:
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=strat.radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        it["relative_decrease"] = rel_dec
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
    S["num_inner_iteration_steps"] = inner_steps
    S["inner_enabled_at_end"] = inner_enabled
    return x, S
