"""ITERATIVE_SCHUR restated in float64 numpy from the block structure alone (p.bs, p.values, p.D, p.b): no oracle, no device.

With J = [E | F] (E: the first num_eliminate_blocks column blocks, each row holding at most one E cell) and M_e = E^T E + D_e^2, which is
block diagonal with one block per eliminated column block:

    S        = F^T F + D_f^2 - F^T E M_e^-1 E^T F                       (applied implicitly; dense only for num_cols_f <= 3100)
    rhs      = F^T (b - E M_e^-1 E^T b)                                 (ImplicitSchurComplement::UpdateRhs)
    back-sub = [M_e^-1 E^T (b - F z) ; z]                               (ImplicitSchurComplement::BackSubstitute)
    B        = blockdiag(F^T F + D_f^2)                                 (JACOBI for ITERATIVE_SCHUR)
    T x      = B^-1 F^T E M_e^-1 E^T F x                                (the power-series operator adds T x to y)
    spse(x)  = sum_{i=0..k} T^i B^-1 x, cut short when a term's norm < tol |B^-1 x|   (PowerSeriesExpansionPreconditioner)

and the preconditioned CG of ConjugateGradientsSolver, x_0 = 0, with the back-substitution behind it unless CG failed.  Every sum is a
numpy reduction in float64; nothing here shares code with the kernels or the oracle, so a disagreement names the side at fault when the
other two agree.
"""
import numpy as np

SCHUR_DENSE_MAX_COLS_F = 3100   # (343 cameras 9 wide, the smallest DENSE_SCHUR system with look-ahead: tests/test_gpu_dense_cholesky.py)
IDENTITY, JACOBI, SCHUR_JACOBI, SCHUR_POWER_SERIES_EXPANSION = 0, 1, 2, 3
SUCCESS, NO_CONVERGENCE, FAILURE = 0, 1, 2


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


class SchurReference:
    def __init__(self, p):
        bs = p.bs
        self.bs = bs
        self.nelim = int(p.num_eliminate_blocks)
        self.values = np.asarray(p.values, dtype=np.float64)
        self.b = np.asarray(p.b, dtype=np.float64)
        self.num_rows, self.num_cols = bs.num_rows, bs.num_cols
        cbs, cbp = bs.col_block_size.astype(np.int64), bs.col_block_pos.astype(np.int64)
        self.ne = int(cbp[self.nelim]) if self.nelim < bs.num_col_blocks else self.num_cols
        self.nf = self.num_cols - self.ne
        self.D = np.zeros(self.num_cols) if p.D is None else np.asarray(p.D, dtype=np.float64)
        self.e_sizes, self.f_sizes = cbs[:self.nelim], cbs[self.nelim:]
        # ---- J as coordinate triplets (one per stored entry of every cell)
        rows_of_cell = np.repeat(np.arange(bs.num_row_blocks), np.diff(bs.row_cell_ptr))
        ri, ci, vi = [], [], []
        for k in range(bs.num_cells):
            r, c = int(rows_of_cell[k]), int(bs.cell_col_block[k])
            rs, rp, cs, cp, vp = int(bs.row_block_size[r]), int(bs.row_block_pos[r]), int(cbs[c]), int(cbp[c]), int(bs.cell_value_pos[k])
            ri.append(np.repeat(np.arange(rp, rp + rs), cs))
            ci.append(np.tile(np.arange(cp, cp + cs), rs))
            vi.append(self.values[vp:vp + rs * cs])
        self.ri = np.concatenate(ri) if ri else np.zeros(0, np.int64)
        self.ci = np.concatenate(ci) if ci else np.zeros(0, np.int64)
        self.vi = np.concatenate(vi) if vi else np.zeros(0)
        self.is_e = self.ci < self.ne
        # ---- M_e^-1, one block per eliminated column block (E^T E from the E cells alone: at most one per row)
        self.ete = [np.diag(self.D[int(cbp[j]):int(cbp[j] + cbs[j])] ** 2) for j in range(self.nelim)]
        self.ftf = [np.diag(self.D[int(cbp[j]):int(cbp[j] + cbs[j])] ** 2) for j in range(self.nelim, bs.num_col_blocks)]
        # (point block, F block) -> E_p^T F_c over the rows they share
        self.ef = {}
        for r in range(bs.num_row_blocks):
            rs, rp = int(bs.row_block_size[r]), int(bs.row_block_pos[r])
            e_cell, f_cells = None, []
            for k in range(int(bs.row_cell_ptr[r]), int(bs.row_cell_ptr[r + 1])):
                c = int(bs.cell_col_block[k])
                blk = self.values[int(bs.cell_value_pos[k]):int(bs.cell_value_pos[k]) + rs * int(cbs[c])].reshape(rs, int(cbs[c]))
                if c < self.nelim:
                    assert e_cell is None, "a row with two E cells is not a Schur structure"
                    e_cell = (c, blk)
                else:
                    f_cells.append((c - self.nelim, blk))
            if e_cell is not None:
                self.ete[e_cell[0]] = self.ete[e_cell[0]] + e_cell[1].T @ e_cell[1]
            for c, blk in f_cells:
                self.ftf[c] = self.ftf[c] + blk.T @ blk
                if e_cell is not None:
                    key = (e_cell[0], c)
                    self.ef[key] = self.ef.get(key, 0.0) + e_cell[1].T @ blk
        self.ete_inv = [np.linalg.inv(m) for m in self.ete]
        self.ftf_inv = [np.linalg.inv(m) for m in self.ftf]
        self.e_pos = cbp[:self.nelim]
        self.f_pos = cbp[self.nelim:] - self.ne

    # ---- sparse products
    def J(self, x):
        return np.bincount(self.ri, weights=self.vi * x[self.ci], minlength=self.num_rows)

    def Jt(self, y):
        return np.bincount(self.ci, weights=self.vi * y[self.ri], minlength=self.num_cols)

    def E(self, xe):
        return self.J(np.concatenate([xe, np.zeros(self.nf)]))

    def F(self, xf):
        return self.J(np.concatenate([np.zeros(self.ne), xf]))

    def Et(self, y):
        return self.Jt(y)[:self.ne]

    def Ft(self, y):
        return self.Jt(y)[self.ne:]

    def _block_apply(self, blocks, pos, x):
        y = np.zeros_like(x)
        for m, o in zip(blocks, pos):
            n = m.shape[0]
            y[o:o + n] = m @ x[o:o + n]
        return y

    def ete_inv_apply(self, xe):
        return self._block_apply(self.ete_inv, self.e_pos, xe)

    # ---- ImplicitSchurComplement
    def sx(self, xf):
        Fx = self.F(xf)
        return self.Ft(Fx - self.E(self.ete_inv_apply(self.Et(Fx)))) + self.D[self.ne:] ** 2 * xf

    def rhs(self):
        return self.Ft(self.b - self.E(self.ete_inv_apply(self.Et(self.b))))

    def ete_inverse(self):
        return np.concatenate([m.reshape(-1) for m in self.ete_inv]) if self.ete_inv else np.zeros(0)

    def back_substitute(self, z):
        xe = self.ete_inv_apply(self.Et(self.b - self.F(z)))
        return np.concatenate([xe, z])

    def dense_S(self):
        assert self.nf <= SCHUR_DENSE_MAX_COLS_F, self.nf
        Fd = np.zeros((self.num_rows, self.nf))
        m = ~self.is_e
        np.add.at(Fd, (self.ri[m], self.ci[m] - self.ne), self.vi[m])
        Ed = np.zeros((self.num_rows, self.ne))
        np.add.at(Ed, (self.ri[self.is_e], self.ci[self.is_e]), self.vi[self.is_e])
        EtF = Ed.T @ Fd
        Minv = np.zeros((self.ne, self.ne))
        for blk, o in zip(self.ete_inv, self.e_pos):
            Minv[o:o + blk.shape[0], o:o + blk.shape[0]] = blk
        return Fd.T @ Fd + np.diag(self.D[self.ne:] ** 2) - EtF.T @ Minv @ EtF

    # ---- preconditioners
    def schur_jacobi_raw(self):
        """Diagonal blocks of S, one per F block, full (both triangles)."""
        blocks = [m.copy() for m in self.ftf]
        for (pt, c), W in self.ef.items():
            blocks[c] -= W.T @ self.ete_inv[pt] @ W
        return blocks

    def schur_jacobi_inv(self):
        return [np.linalg.inv(m) for m in self.schur_jacobi_raw()]

    @staticmethod
    def flat(blocks):
        return np.concatenate([m.reshape(-1) for m in blocks]) if blocks else np.zeros(0)

    def block_apply_f(self, blocks, x):
        return self._block_apply(blocks, self.f_pos, x)

    # ---- SCHUR_POWER_SERIES_EXPANSION
    def power_series_operator(self, x, y=None):
        """y + B^-1 F^T E M_e^-1 E^T F x."""
        y = np.zeros(self.nf) if y is None else np.asarray(y, dtype=np.float64).copy()
        return y + self.block_apply_f(self.ftf_inv, self.Ft(self.E(self.ete_inv_apply(self.Et(self.F(x))))))

    def spse_apply(self, x, max_num_spse_iterations=5, spse_tolerance=0.0):
        y = self.block_apply_f(self.ftf_inv, x)
        term = y.copy()
        threshold = spse_tolerance * np.linalg.norm(y)
        i = 1
        while True:
            term = self.power_series_operator(term)
            y = y + term
            if i >= max_num_spse_iterations or np.linalg.norm(term) < threshold:
                return y
            i += 1

    # ---- the solver
    def preconditioner(self, kind, max_num_spse_iterations=5):
        if kind == IDENTITY:
            return lambda r: r.copy()
        if kind == JACOBI:
            return lambda r: self.block_apply_f(self.ftf_inv, r)
        if kind == SCHUR_JACOBI:
            inv = self.schur_jacobi_inv()
            return lambda r: self.block_apply_f(inv, r)
        if kind == SCHUR_POWER_SERIES_EXPANSION:   # inside CG the series is never cut short (tolerance 0)
            return lambda r: self.spse_apply(r, max_num_spse_iterations, 0.0)
        raise ValueError(kind)

    def solve(self, preconditioner, min_it, max_it, q_tol=-1.0, r_tol=-1.0, reset_period=10, max_num_spse_iterations=5):
        """ITERATIVE_SCHUR: returns (x over all columns, Summary); x is None if CG failed (no back-substitution then)."""
        if self.nf == 0:
            return self.back_substitute(np.zeros(0)), Summary(SUCCESS, 0, "")
        z, summ = cg(self.sx, self.rhs(), self.preconditioner(preconditioner, max_num_spse_iterations), min_it, max_it, q_tol, r_tol,
                     reset_period)
        return (None if summ.termination_type == FAILURE else self.back_substitute(z)), summ

    def with_D(self, D):
        """The same J and b under another regulariser (the LM step's sqrt(diag / radius))."""
        q = _Problem(self.bs, self.values, self.b, D, self.nelim)
        return SchurReference(q)

    def squared_column_norm(self):
        return np.bincount(self.ci, weights=self.vi ** 2, minlength=self.num_cols)

    def model_cost_change(self, step):
        """TrustRegionMinimizer's model cost change of the step x (the LM step is -x of the solve): -(J s).(b + J s / 2)."""
        Js = self.J(step)
        return float(-Js @ (self.b + Js / 2.0))


class _Problem:
    def __init__(self, bs, values, b, D, num_eliminate_blocks):
        self.bs, self.values, self.b, self.D, self.num_eliminate_blocks = bs, values, b, D, num_eliminate_blocks


class Summary:
    def __init__(self, termination_type, num_iterations, message):
        self.termination_type, self.num_iterations, self.message = termination_type, num_iterations, message

    def __repr__(self):
        return f"Summary({self.termination_type}, {self.num_iterations}, {self.message!r})"


def cg(A, b, M, min_it, max_it, q_tol, r_tol, reset_period=10):
    """ConjugateGradientsSolver from x = 0: returns (x, Summary); the messages are the reference's where callers parse them."""
    n = b.shape[0]
    x = np.zeros(n)
    norm_b = np.linalg.norm(b)
    if norm_b == 0.0:
        return x, Summary(SUCCESS, 0, "Convergence. |b| = 0.")
    tol_r = r_tol * norm_b
    r = b - A(x)
    if min_it == 0 and np.linalg.norm(r) <= tol_r:
        return x, Summary(SUCCESS, 0, "Convergence. |r| <= tol_r.")
    bad = lambda v: v == 0.0 or np.isinf(v)
    rho, Q0, p = 1.0, -x @ (b + r), None
    i = 1
    while True:
        z = M(r)
        last_rho, rho = rho, r @ z
        if bad(rho):
            return x, Summary(FAILURE, i, f"Numerical failure. rho = r'z = {rho:e}.")
        if i == 1:
            p = z
        else:
            beta = rho / last_rho
            if bad(beta):
                return x, Summary(FAILURE, i, "Numerical failure. beta")
            p = z + beta * p
        q = A(p)
        pq = p @ q
        if pq <= 0 or np.isinf(pq):
            return x, Summary(NO_CONVERGENCE, i, "Matrix is indefinite")
        alpha = rho / pq
        if np.isinf(alpha):
            return x, Summary(FAILURE, i, "Numerical failure. alpha")
        x = x + alpha * p
        r = b - A(x) if i % reset_period == 0 else r - alpha * q
        Q1 = -x @ (b + r)
        zeta = i * (Q1 - Q0) / Q1
        if zeta < q_tol and i >= min_it:
            return x, Summary(SUCCESS, i, f"Iteration: {i} Convergence: zeta = {zeta:e} < {q_tol:e}. |r| = {np.linalg.norm(r):e}")
        Q0 = Q1
        if np.linalg.norm(r) <= tol_r and i >= min_it:
            return x, Summary(SUCCESS, i, "Convergence. |r| <= tol_r.")
        if i >= max_it:
            return x, Summary(NO_CONVERGENCE, i, "Maximum number of iterations reached.")
        i += 1


# ---- the cases of tests/test_schur_dense_cpu.py and tests/test_gpu_schur_state.py, built through fuzz_cases.build (problems.structured_bal)
FUZZ_SEED = 17   # 500 cameras (about 270 unobserved), 65 points, one of them a whole 64-observation tile, blocks <2,4,6>


def _track_case(name, shape, n_cams, long_track, n_short, prior_rows=0, seed=0):
    rng = np.random.default_rng(1009 * seed + 5)
    k = np.concatenate([[long_track], rng.integers(1, 4, size=n_short)]) if long_track else rng.integers(1, 5, size=n_short)
    case = dict(seed=seed, n_cams=n_cams, n_points=int(k.shape[0]), n_obs=int(k.sum()), max_track=int(k.max()), shape=list(shape),
                shared=[], locked=[], prior_rows=prior_rows, skew=0.0)
    return name, case, k.astype(np.int64)


def constructed_cases():
    """(name, case, track lengths): one point with a track around the 64-row tile (63, 64, 65, 128) among short ones on 500 cameras of
    which at least 250 see nothing, for <2,4,6> and <2,3,9>; 2300 cameras 9 wide (past the LDS limit of the camera accumulators: the
    camera-major pass); and camera-only prior rows."""
    out = []
    for shape in ((2, 4, 6), (2, 3, 9)):
        for i, L in enumerate((63, 64, 65, 128)):
            out.append(_track_case(f"track{L}_{''.join(map(str, shape))}", shape, 500, L, 50, seed=10 * shape[1] + i))
    out.append(_track_case("cameras2300_239", (2, 3, 9), 2300, 0, 4000, seed=90))
    out.append(_track_case("prior_rows_239", (2, 3, 9), 500, 64, 50, prior_rows=40, seed=91))
    return out


def build_case(P, name):
    """The LinearProblem of a case name: 'fuzz17' or one of constructed_cases()."""
    import fuzz_cases
    if name == f"fuzz{FUZZ_SEED}":
        case, k, _ = fuzz_cases.draw_case(FUZZ_SEED)
        return fuzz_cases.build(P, case, k)
    for n, case, k in constructed_cases():
        if n == name:
            return fuzz_cases.build(P, case, k)
    raise KeyError(name)


def case_names():
    return [f"fuzz{FUZZ_SEED}"] + [n for n, _, _ in constructed_cases()]
