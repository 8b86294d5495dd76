"""A numpy restatement of inner iterations in the BAL front end: what ceres_hip_debug_inner_iteration_ordering, the per-block
Levenberg-Marquardt kernels (csrc/kernels_inner.hip) and ceres_hip_bal_minimize with inner iterations set (csrc/bal_frontend.inc) are
checked against.  It imports nothing from the product; losses, the Corrector and the Evaluator come from tests/robust_reference.py.

  the AUTOMATIC ordering    CoordinateDescentMinimizer::CreateOrdering (internal/ceres/coordinate_descent_minimizer.cc:268-273):
                            ComputeRecursiveIndependentSetOrdering (internal/ceres/parameter_block_ordering.cc:101-123), then Reverse();
                            degree ties broken by state position (points, then cameras) — the ABI's rule
  one block                 CoordinateDescentMinimizer::Solve (:213-240): TrustRegionMinimizer with default options, LM, the
                            normal equations by Cholesky (a non-positive pivot: an invalid step), batched over the blocks of a group
  one pass                  CoordinateDescentMinimizer::Minimize (:130-211)
  the outer loop            TrustRegionMinimizer::DoInnerIterationsIfNeeded (internal/ceres/trust_region_minimizer.cc:509-587)"""
import numpy as np

import robust_reference as R

KINDS = ("automatic", "cameras", "points", "cameras,points", "points,cameras")
DBL_MAX = np.finfo(np.float64).max


def ordering(num_cameras, num_points, camera_index, point_index, blocks):
    """(group of every block in state order — points, then cameras; -1 outside the ordering —, number of groups)."""
    nc, npt = int(num_cameras), int(num_points)
    nv = npt + nc
    g = np.full(nv, -1, dtype=np.int64)
    if blocks == "cameras":
        g[npt:] = 0
        return g, 1
    if blocks == "points":
        g[:npt] = 0
        return g, 1
    if blocks == "cameras,points":
        g[npt:], g[:npt] = 0, 1
        return g, 2
    if blocks == "points,cameras":
        g[:npt], g[npt:] = 0, 1
        return g, 2
    assert blocks == "automatic", blocks
    adj = [set() for _ in range(nv)]
    for c, q in zip(np.asarray(camera_index), np.asarray(point_index)):
        adj[int(q)].add(npt + int(c))
        adj[npt + int(c)].add(int(q))
    round_of = np.full(nv, -1)
    rounds = 0
    while np.any(round_of < 0):
        alive = [v for v in range(nv) if round_of[v] < 0]
        deg = {v: sum(1 for u in adj[v] if round_of[u] < 0) for v in alive}
        color = {v: 0 for v in alive}
        for v in sorted(alive, key=lambda v: (deg[v], v)):
            if color[v] != 0:
                continue
            color[v] = 2
            for u in adj[v]:
                if round_of[u] < 0 and color[u] != 2:
                    color[u] = 1
        for v in alive:
            if color[v] == 2:
                round_of[v] = rounds
        rounds += 1
    return rounds - 1 - round_of, rounds


def _cholesky_solve(M, g):
    """x = -M^-1 g per block (M: (n, k, k)), the kernel's Cholesky; ok = False where a pivot is not positive and finite."""
    n, k = g.shape
    U = np.zeros_like(M)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for i in range(k):
            d = M[:, i, i] - sum(U[:, j, i] * U[:, j, i] for j in range(i)) if i else M[:, i, i].copy()
            ok &= (d > 0.0) & np.isfinite(d)
            u = np.sqrt(np.where(ok, d, 1.0))
            U[:, i, i] = u
            for j in range(i + 1, k):
                v = M[:, i, j] - sum(U[:, m, i] * U[:, m, j] for m in range(i)) if i else M[:, i, j].copy()
                U[:, i, j] = v / u
        y = np.zeros_like(g)
        for i in range(k):
            y[:, i] = (-g[:, i] - sum(U[:, m, i] * y[:, m] for m in range(i))) / U[:, i, i]
        x = np.zeros_like(g)
        for i in reversed(range(k)):
            x[:, i] = (y[:, i] - sum(U[:, i, m] * x[:, m] for m in range(i + 1, k))) / U[:, i, i]
    return x, ok


class _Group:
    """The blocks of one kind (points or cameras) of one group, with their observations (rows of the Evaluator)."""

    def __init__(self, ev, cameras, blocks):
        self.ev, self.cameras = ev, cameras
        self.blocks = np.asarray(blocks, dtype=np.int64)
        self.k = 9 if cameras else 3
        owner = ev.cam if cameras else ev.pt
        pos = np.full(ev.nc if cameras else ev.np_, -1)
        pos[self.blocks] = np.arange(self.blocks.size)
        self.rows = np.flatnonzero(pos[owner] >= 0)
        self.row_block = pos[owner[self.rows]]

    def get(self, x):
        base = 3 * self.ev.np_ if self.cameras else 0
        return x[base:].reshape(-1, self.k)[self.blocks] if self.cameras else x[:3 * self.ev.np_].reshape(-1, 3)[self.blocks]

    def put(self, x, P, mask):
        v = x[3 * self.ev.np_:].reshape(-1, 9) if self.cameras else x[:3 * self.ev.np_].reshape(-1, 3)
        v[self.blocks[mask]] = P[mask]

    def evaluate(self, x, P, jac):
        """Per block: cost (NaN where a residual is not finite) and, jac, H = J^T J and g = J^T f (unscaled, corrected)."""
        ev, nb = self.ev, self.blocks.size
        xx = np.array(x, dtype=np.float64)
        self.put(xx, P, np.ones(nb, bool))
        cams = xx[3 * ev.np_:].reshape(-1, 9)[ev.cam[self.rows]]
        pts = xx[:3 * ev.np_].reshape(-1, 3)[ev.pt[self.rows]]
        with np.errstate(all="ignore"):
            r, jc, jp = ev.snavely(cams, pts, ev.obs[self.rows])
            s = np.sum(r * r, axis=1)
            J = jc if self.cameras else jp
            if ev.loss is None:
                c = 0.5 * s
            else:
                rhos = R.rho(ev.loss[0], s, *ev.loss[1:])
                c = 0.5 * rhos[0]
                if jac:
                    r, J = R.correct(r, J, rhos, s)
        cost = np.zeros(nb)
        np.add.at(cost, self.row_block, c)
        bad = np.zeros(nb, bool)
        np.logical_or.at(bad, self.row_block, ~np.all(np.isfinite(r), axis=1))
        cost[bad] = np.nan
        if not jac:
            return cost, None, None
        H = np.zeros((nb, self.k, self.k))
        g = np.zeros((nb, self.k))
        np.add.at(H, self.row_block, np.einsum("nki,nkj->nij", J, J))
        np.add.at(g, self.row_block, np.einsum("nki,nk->ni", J, r))
        return cost, H, g


def solve_group(grp, x):
    """Every block of grp by its own TrustRegionMinimizer (default options) with everything else at x.  Returns (new block values,
    iterations per block)."""
    P = grp.get(x).copy()
    nb, k = P.shape
    cost, H0, g0 = grp.evaluate(x, P, True)
    its = np.zeros(nb, dtype=np.int64)
    active = np.isfinite(cost)
    x_cost = cost
    with np.errstate(all="ignore"):
        scale = 1.0 / (1.0 + np.sqrt(np.einsum("nii->ni", H0)))
    H = H0 * scale[:, :, None] * scale[:, None, :]
    g = g0 * scale
    grad_max = np.max(np.abs(g0), axis=1)
    radius, df = np.full(nb, 1e4), np.full(nb, 2.0)
    reuse, one_success = np.zeros(nb, bool), np.zeros(nb, bool)
    invalid_run = np.zeros(nb, dtype=np.int64)
    diag = np.zeros((nb, k))
    while True:
        active &= (its < 50) & (grad_max > 1e-10) & (radius > 1e-32)
        if not active.any():
            break
        act = active.copy()
        its[act] += 1
        need = act & ~reuse
        diag[need] = np.clip(np.einsum("nii->ni", H)[need], 1e-6, 1e32)
        reuse[act] = True
        M = H + np.einsum("ni,ij->nij", diag / radius[:, None], np.eye(k))
        step, ok = _cholesky_solve(M, g)
        with np.errstate(all="ignore"):
            mcc = -(np.sum(step * g, axis=1) + 0.5 * np.einsum("ni,nij,nj->n", step, H, step))
        valid = ok & np.all(np.isfinite(step), axis=1) & (mcc > 0.0)
        inv = act & ~valid
        invalid_run[inv] += 1
        stop = inv & (invalid_run >= 5)
        active[stop] = False
        shrink = inv & ~stop
        radius[shrink] /= df[shrink]
        df[shrink] *= 2.0
        v = act & valid
        if not v.any():
            continue
        invalid_run[v] = 0
        cand = P + step * scale
        dn = np.sqrt(np.sum((P - cand) ** 2, axis=1))
        xn = np.sqrt(np.sum(P * P, axis=1))
        cc, _, _ = grp.evaluate(x, np.where(v[:, None], cand, P), False)
        cc = np.where(np.isfinite(cc), cc, DBL_MAX)
        stop_p = v & one_success & (dn <= 1e-8 * (xn + 1e-8))
        with np.errstate(all="ignore"):
            stop_f = v & ~stop_p & (np.abs(x_cost - cc) <= 1e-6 * x_cost)
            rest = v & ~stop_p & ~stop_f
            rd = (x_cost - cc) / mcc
        active[stop_p | stop_f] = False
        acc = rest & (rd > 1e-3)
        rej = rest & ~acc
        radius[rej] /= df[rej]
        df[rej] *= 2.0
        if acc.any():
            c1, H1, g1 = grp.evaluate(x, np.where(acc[:, None], cand, P), True)
            failed = acc & ~np.isfinite(c1)
            active[failed] = False
            a = acc & ~failed
            P[a] = cand[a]
            x_cost = np.where(a, c1, x_cost)
            H[a] = (H1 * scale[:, :, None] * scale[:, None, :])[a]
            g[a] = (g1 * scale)[a]
            grad_max = np.where(a, np.max(np.abs(g1), axis=1), grad_max)
            one_success |= a
            t = 2.0 * rd - 1.0
            radius[a] = np.minimum(1e32, radius[a] / np.maximum(1.0 / 3.0, 1.0 - t[a] ** 3))
            df[a] = 2.0
            reuse[a] = False
    return P, its


def one_pass(ev, x, group, num_groups):
    """CoordinateDescentMinimizer::Minimize at x: (new x, iterations per block in state order, -1 outside the ordering)."""
    x = np.array(x, dtype=np.float64)
    its = np.full(ev.np_ + ev.nc, -1, dtype=np.int64)
    for gi in range(num_groups):
        for cameras in (False, True):
            sel = np.flatnonzero(group[ev.np_:] == gi) if cameras else np.flatnonzero(group[:ev.np_] == gi)
            if sel.size == 0:
                continue
            grp = _Group(ev, cameras, sel)
            P, it = solve_group(grp, x)
            grp.put(x, P, np.ones(sel.size, bool))
            its[(ev.np_ if cameras else 0) + sel] = it
    return x, its


def minimize(ev, x0, group, num_groups, inner_iteration_tolerance=1e-3, **opts):
    """robust_reference.minimize with DoInnerIterationsIfNeeded after the candidate's cost.  The summary also has
    num_inner_iteration_steps, and per iteration inner_useful / relative_decrease."""
    o = dict(R.DEFAULTS)
    o.update(opts)
    x = np.array(x0, dtype=np.float64)
    n = ev.n
    radius, decrease_factor = o["initial_trust_region_radius"], 2.0
    reuse_diagonal, one_success, invalid_run, iteration = False, False, 0, 0
    inner_enabled, inner_steps = True, 0
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
    its.append(dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius, step_is_valid=1, step_is_successful=1))
    diag = None
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = R.NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"]:
            S["termination_type"] = R.CONVERGENCE
            break
        if radius <= o["min_trust_region_radius"]:
            S["termination_type"] = R.CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0, inner_useful=False)
        Js, r = st["Js"], st["r"]
        if not reuse_diagonal:
            diag = np.clip(np.sum(Js * Js, axis=0), o["min_lm_diagonal"], o["max_lm_diagonal"])
        step = -np.linalg.solve(Js.T @ Js + np.diag(diag / radius), Js.T @ r)
        reuse_diagonal = True
        model = Js @ step
        mcc = -float(np.sum(model * (r + model / 2.0)))
        valid = bool(np.all(np.isfinite(step))) and mcc > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            invalid_run += 1
            if invalid_run >= o["max_consecutive_invalid_steps"]:
                S["termination_type"] = R.FAILURE
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius)
            its.append(it)
            continue
        invalid_run = 0
        cand = x + step * scale if o["jacobi_scaling"] else x + step
        cand_cost = ev.cost(cand)
        inner_useful = False
        if inner_enabled and np.isfinite(cand_cost):   # DoInnerIterationsIfNeeded
            inner_steps += 1
            xi, _ = one_pass(ev, cand, group, num_groups)
            ic = ev.cost(xi)
            if np.isfinite(ic):
                cand = xi
                mcc += cand_cost - ic
                inner_useful = ic < min(st["cost"], cand_cost)
                inner_enabled = (1.0 - ic / cand_cost) > inner_iteration_tolerance
                cand_cost = ic
        it["inner_useful"] = inner_useful
        step_norm = float(np.linalg.norm(x - cand))
        if one_success and step_norm <= o["parameter_tolerance"] * (float(np.linalg.norm(x)) + o["parameter_tolerance"]):
            S["termination_type"] = R.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        if abs(st["cost"] - cand_cost) <= o["function_tolerance"] * st["cost"]:
            S["termination_type"] = R.CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        it["relative_decrease"] = rel_dec
        if inner_useful or rel_dec > o["min_relative_decrease"]:
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
    S["num_inner_iteration_steps"] = inner_steps
    S["inner_enabled_at_end"] = inner_enabled
    return x, S
