"""A numpy restatement of the robust losses, the Corrector and the trust-region loop of the BAL front end with a loss set: what the
device evaluator (csrc/robust_loss.h, csrc/kernels_evaluator.hip) and ceres_hip_bal_minimize (csrc/bal_frontend.inc) are checked
against.  It imports nothing from the product; the Snavely residual and its Jacobian come from the oracle (oracle.snavely_batch: dual
numbers), passed in by the caller.

  rho(s), rho'(s), rho''(s)       include/ceres/loss_function.h:131-330, internal/ceres/loss_function.cc:46-175
  ResidualBlock::Evaluate         internal/ceres/residual_block.cc:161-195 (cost rho / 2; J corrected before r)
  Corrector                       internal/ceres/corrector.cc:41-135
  the loop                        internal/ceres/trust_region_minimizer.cc (Jacobi scaling from the corrected Jacobian at iteration 0),
                                  internal/ceres/levenberg_marquardt_strategy.cc — here with a dense solve: small problems only."""
import numpy as np

LOSSES = ("trivial", "huber", "soft_l_one", "cauchy", "arctan", "tolerant", "tukey")
DBL_MIN = np.finfo(np.float64).tiny


def rho(kind, s, a=1.0, b=1.0, scale=1.0):
    """(rho, rho', rho'') of ScaledLoss(kind(a[, b]), scale) at s (array, s >= 0)."""
    s = np.asarray(s, dtype=np.float64)
    r0, r1, r2 = np.empty_like(s), np.empty_like(s), np.empty_like(s)
    if kind == "trivial":
        r0[...], r1[...], r2[...] = s, 1.0, 0.0
    elif kind == "huber":
        bb = a * a
        out = s > bb
        r = np.sqrt(np.where(out, s, 1.0))
        r0[...] = np.where(out, 2.0 * a * r - bb, s)
        r1[...] = np.where(out, np.maximum(DBL_MIN, a / r), 1.0)
        r2[...] = np.where(out, -r1 / (2.0 * np.where(out, s, 1.0)), 0.0)
    elif kind in ("soft_l_one", "cauchy"):
        bb = a * a
        c = 1.0 / bb
        total = 1.0 + s * c
        if kind == "soft_l_one":
            tmp = np.sqrt(total)
            r0[...] = 2.0 * bb * (tmp - 1.0)
            r1[...] = np.maximum(DBL_MIN, 1.0 / tmp)
            r2[...] = -(c * r1) / (2.0 * total)
        else:
            inv = 1.0 / total
            r0[...] = bb * np.log(total)
            r1[...] = np.maximum(DBL_MIN, inv)
            r2[...] = -c * (inv * inv)
    elif kind == "arctan":
        bb = 1.0 / (a * a)
        inv = 1.0 / (1.0 + s * s * bb)
        r0[...] = a * np.arctan2(s, a)
        r1[...] = np.maximum(DBL_MIN, inv)
        r2[...] = -2.0 * s * bb * (inv * inv)
    elif kind == "tolerant":
        c = b * np.log(1.0 + np.exp(-a / b))
        x = (s - a) / b
        big = x > 36.7   # ln(2^53)
        xs = np.where(big, 0.0, x)
        e_x = np.exp(xs)
        r0[...] = np.where(big, s - a - c, b * np.log(1.0 + e_x) - c)
        r1[...] = np.where(big, 1.0, np.maximum(DBL_MIN, e_x / (1.0 + e_x)))
        r2[...] = np.where(big, 0.0, 0.5 / (b * (1.0 + np.cosh(xs))))
    elif kind == "tukey":
        a2 = a * a
        inl = s <= a2
        v = 1.0 - s / a2
        r0[...] = np.where(inl, a2 / 3.0 * (1.0 - v * v * v), a2 / 3.0)
        r1[...] = np.where(inl, v * v, 0.0)
        r2[...] = np.where(inl, -2.0 / a2 * v, 0.0)
    else:
        raise ValueError(kind)
    return scale * r0, scale * r1, scale * r2


def corrector(s, rhos):
    """(sqrt(rho'), residual scaling, alpha / s) per residual block."""
    _, r1, r2 = rhos
    s = np.asarray(s, dtype=np.float64)
    sqrt_rho1 = np.sqrt(r1)
    full = (s != 0.0) & (r2 > 0.0)
    ss = np.where(full, s, 1.0)
    alpha = np.where(full, 1.0 - np.sqrt(1.0 + 2.0 * ss * np.where(full, r2, 0.0) / np.where(full, r1, 1.0)), 0.0)
    return sqrt_rho1, np.where(full, sqrt_rho1 / (1.0 - alpha), sqrt_rho1), np.where(full, alpha / ss, 0.0)


def correct(r, J, rhos, s=None):
    """(r~, J~) of blocks r (n, k) and J (n, k, m): J~ = sqrt(rho') (J - (alpha / s) r (r^T J)), r~ = residual scaling * r."""
    if s is None:
        s = np.sum(r * r, axis=1)
    sqrt_rho1, rs, asn = corrector(s, rhos)
    rtj = np.einsum("nk,nkm->nm", r, J)
    Jt = sqrt_rho1[:, None, None] * (J - (asn[:, None] * r)[:, :, None] * rtj[:, None, :])
    return r * rs[:, None], Jt


class Evaluator:
    """Cost, residuals, Jacobian values and gradient of a BAL problem with one loss for every observation, in the solver layout
    ceres_hip_bal_evaluate uses: rows in `row_order`, E cell of row r at 6 r, F cell at 6 n_rows + 18 r (row-major 2 x 3, 2 x 9);
    state = [3 per point | 9 per camera]."""

    def __init__(self, snavely_batch, num_cameras, num_points, camera_index, point_index, observations, row_order, loss=None):
        self.snavely = snavely_batch
        self.nc, self.np_ = int(num_cameras), int(num_points)
        order = np.asarray(row_order)
        self.cam = np.asarray(camera_index)[order].astype(np.int64)
        self.pt = np.asarray(point_index)[order].astype(np.int64)
        self.obs = np.asarray(observations, dtype=np.float64).reshape(-1, 2)[order]
        self.n_rows = self.cam.shape[0]
        self.n = 3 * self.np_ + 9 * self.nc
        self.loss = loss   # None: the squared loss; else (kind, a, b, scale)

    def _blocks(self, x):
        x = np.asarray(x, dtype=np.float64)
        cams = x[3 * self.np_:].reshape(-1, 9)[self.cam]
        pts = x[:3 * self.np_].reshape(-1, 3)[self.pt]
        return self.snavely(cams, pts, self.obs)

    def cost(self, x):
        r, _, _ = self._blocks(x)
        s = np.sum(r * r, axis=1)
        if self.loss is None:
            return 0.5 * float(np.sum(s))
        return 0.5 * float(np.sum(rho(self.loss[0], s, *self.loss[1:])[0]))

    def evaluate(self, x, corrector_free_gradient=False):
        """(cost, residuals, values, gradient); corrector_free_gradient: also sum rho' J^T r, computed without the Corrector."""
        r, jc, jp = self._blocks(x)
        s = np.sum(r * r, axis=1)
        if self.loss is None:
            cost, rt, jct, jpt, rhos = 0.5 * float(np.sum(s)), r, jc, jp, None
        else:
            rhos = rho(self.loss[0], s, *self.loss[1:])
            cost = 0.5 * float(np.sum(rhos[0]))
            J = np.concatenate([jp, jc], axis=2)
            rt, Jt = correct(r, J, rhos, s)
            jpt, jct = Jt[:, :, :3], Jt[:, :, 3:]
        vals = np.concatenate([jpt.reshape(-1), jct.reshape(-1)])
        g = self.jtr(jpt, jct, rt)
        if corrector_free_gradient:
            w = np.ones(self.n_rows) if rhos is None else rhos[1]
            return cost, rt.reshape(-1), vals, g, self.jtr(jp, jc, r * w[:, None])
        return cost, rt.reshape(-1), vals, g

    def jtr(self, jp, jc, r):
        g = np.zeros(self.n)
        gp = g[:3 * self.np_].reshape(-1, 3)
        gc = g[3 * self.np_:].reshape(-1, 9)
        np.add.at(gp, self.pt, np.einsum("nkm,nk->nm", jp, r))
        np.add.at(gc, self.cam, np.einsum("nkm,nk->nm", jc, r))
        return g

    def dense_jacobian(self, vals):
        """The (2 n_rows) x n matrix of solver-layout values."""
        J = np.zeros((2 * self.n_rows, self.n))
        jp = vals[:6 * self.n_rows].reshape(-1, 2, 3)
        jc = vals[6 * self.n_rows:].reshape(-1, 2, 9)
        rows = np.arange(self.n_rows)
        for k in range(2):
            for m in range(3):
                J[2 * rows + k, 3 * self.pt + m] = jp[:, k, m]
            for m in range(9):
                J[2 * rows + k, 3 * self.np_ + 9 * self.cam + m] = jc[:, k, m]
        return J


DEFAULTS = dict(max_num_iterations=50, jacobi_scaling=1, max_consecutive_invalid_steps=5, initial_trust_region_radius=1e4,
                max_trust_region_radius=1e16, min_trust_region_radius=1e-32, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


def minimize(ev: Evaluator, x0, **opts):
    """TrustRegionMinimizer::Minimize with LEVENBERG_MARQUARDT and monotonic steps, statement by statement as ceres_hip_bal_minimize
    runs it, the linear solve exact (dense).  Returns (x, summary dict with 'iterations': [dict(cost, step_is_successful,
    step_is_valid, trust_region_radius, gradient_max_norm)], initial_cost, final_cost, termination_type)."""
    o = dict(DEFAULTS)
    o.update(opts)
    x = np.array(x0, dtype=np.float64)
    n = ev.n
    radius, decrease_factor = o["initial_trust_region_radius"], 2.0
    reuse_diagonal, one_success, invalid_run, iteration = False, False, 0, 0
    scale = np.ones(n)
    its = []
    st = {}

    def eval_jacobian():
        cost, r, vals, g = ev.evaluate(x)
        J = ev.dense_jacobian(vals)
        if o["jacobi_scaling"] and iteration == 0:
            scale[:] = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        st.update(cost=cost, r=r, Js=J * scale[None, :] if o["jacobi_scaling"] else J, grad_max=float(np.max(np.abs(g))))

    eval_jacobian()
    S = dict(initial_cost=st["cost"], termination_type=NO_CONVERGENCE, iterations=[])
    its.append(dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius, step_is_valid=1, step_is_successful=1))
    diag = None
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"]:
            S["termination_type"] = CONVERGENCE
            break
        if radius <= o["min_trust_region_radius"]:
            S["termination_type"] = CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0)
        Js, r = st["Js"], st["r"]
        if not reuse_diagonal:
            diag = np.clip(np.sum(Js * Js, axis=0), o["min_lm_diagonal"], o["max_lm_diagonal"])
        lmd2 = diag / radius
        step = -np.linalg.solve(Js.T @ Js + np.diag(lmd2), Js.T @ r)
        reuse_diagonal = True
        model = Js @ step
        mcc = -float(np.sum(model * (r + model / 2.0)))
        valid = bool(np.all(np.isfinite(step))) and mcc > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            invalid_run += 1
            if invalid_run >= o["max_consecutive_invalid_steps"]:
                S["termination_type"] = FAILURE
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius)
            its.append(it)
            continue
        invalid_run = 0
        delta = step * scale if o["jacobi_scaling"] else step
        cand = x + delta
        cand_cost = ev.cost(cand)
        step_norm = float(np.linalg.norm(delta))
        if one_success and step_norm <= o["parameter_tolerance"] * (float(np.linalg.norm(x)) + o["parameter_tolerance"]):
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        if abs(st["cost"] - cand_cost) <= o["function_tolerance"] * st["cost"]:
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        if rel_dec > o["min_relative_decrease"]:
            x = cand
            one_success = True
            eval_jacobian()
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rel_dec - 1.0) ** 3))
            decrease_factor = 2.0
            reuse_diagonal = False
            it["step_is_successful"] = 1
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
        it.update(cost=st["cost"] if it["step_is_successful"] else cand_cost, gradient_max_norm=st["grad_max"], trust_region_radius=radius)
        its.append(it)
    S["final_cost"] = st["cost"]
    S["iterations"] = its
    return x, S
