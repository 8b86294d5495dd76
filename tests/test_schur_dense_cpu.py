"""The oracle's ITERATIVE_SCHUR against the numpy restatement of tests/schur_dense_reference.py, on fuzz case 17 and the constructed cases
that tests/test_gpu_schur_state.py runs on the device: every operator, the three preconditioners and fixed-count solves.  The oracle is
called as the parity campaign (tools/fuzz_parity.py) calls it, on ONE long-lived Matrix per case, and a second, fresh Matrix must agree
with it bit for bit.  This keeps the reference honest, so that the device tests can compare against it alone."""
import numpy as np
import pytest

import schur_dense_reference as R

OP_TOL = 1e-12
SOLVE_TOL = 1e-10


def upper(blocks_flat, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(np.triu(blocks_flat[o:o + n * n].reshape(n, n)).reshape(-1))
        o += n * n
    return np.concatenate(out)


@pytest.mark.parametrize("name", R.case_names())
def test_oracle_matches_dense_reference(oracle, problems, name):
    p = R.build_case(problems, name)
    ref = R.SchurReference(p)
    m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    assert (m.num_cols_e, m.num_cols_f) == (ref.ne, ref.nf)
    rng = np.random.default_rng(3)
    errs = {}
    # fixed-count solves first, as the campaign does, then the operators on the same Matrix
    xs = {}
    for pre in (R.SCHUR_JACOBI, R.JACOBI, R.SCHUR_POWER_SERIES_EXPANSION):
        for k in (1, 2, 4, 8):
            if pre == R.SCHUR_POWER_SERIES_EXPANSION:
                xo, so = oracle.iterative_schur_solve_spse(m, p.values, p.b, p.D, preconditioner=pre, min_it=k, max_it=k, q_tol=-1.0, r_tol=-1.0)
            else:
                xo, so = m.iterative_schur_solve(p.values, p.b, p.D, preconditioner=pre, min_it=k, max_it=k, q_tol=-1.0, r_tol=-1.0)
            xr, sr = ref.solve(pre, k, k)
            assert (so.termination_type, so.num_iterations) == (sr.termination_type, sr.num_iterations), (pre, k, so, sr)
            errs[f"solve:pre{pre}:k{k}"] = R.rel(xo, xr)
            xs[(pre, k)] = xo
    isc = oracle.ImplicitSchurComplement(m)
    isc.init(p.values, p.D, p.b)
    isc.compute_ftf_inverse()
    errs["schur_rhs"] = R.rel(isc.rhs(), ref.rhs())
    errs["ete_inverse"] = R.rel(isc.ete_inverse(), ref.ete_inverse())
    xf, y0 = rng.standard_normal(ref.nf), rng.standard_normal(ref.nf)
    errs["sx"] = R.rel(isc.sx(xf), ref.sx(xf))
    errs["back_substitute"] = R.rel(isc.back_substitute(xf), ref.back_substitute(xf))
    errs["power_series_operator"] = R.rel(isc.power_series_operator(xf, y0), ref.power_series_operator(xf, y0))
    errs["spse_apply_5"] = R.rel(isc.spse_apply(xf, 5, 0.0), ref.spse_apply(xf, 5, 0.0))
    errs["spse_apply_tol"] = R.rel(isc.spse_apply(xf, 8, 0.1), ref.spse_apply(xf, 8, 0.1))
    inv, raw = m.schur_jacobi(p.values, p.D)
    sizes = ref.f_sizes
    errs["schur_jacobi_raw"] = R.rel(upper(raw, sizes), upper(R.SchurReference.flat(ref.schur_jacobi_raw()), sizes))
    errs["schur_jacobi_inv"] = R.rel(inv, R.SchurReference.flat(ref.schur_jacobi_inv()))
    ftf = m.block_diagonal_ftf(p.values)
    Df = p.D[ref.ne:]
    want, o, pos = [], 0, 0
    for n in sizes:
        want.append(ftf[o:o + n * n].reshape(n, n) + np.diag(Df[pos:pos + n] ** 2))
        o, pos = o + n * n, pos + n
    errs["ftf_plus_D"] = R.rel(R.SchurReference.flat(want), R.SchurReference.flat(ref.ftf))
    if ref.nf <= R.SCHUR_DENSE_MAX_COLS_F:
        errs["dense_S_x"] = R.rel(ref.dense_S() @ xf, ref.sx(xf))
    bad = {k: v for k, v in errs.items() if not (v <= (SOLVE_TOL if k.startswith("solve") else OP_TOL))}
    assert not bad, f"{name}: {bad}   (all: {errs})"
    # the long-lived Matrix holds no state between calls: a fresh one gives the same solves, bit for bit
    m2 = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    for k in (1, 4):
        x2, _ = m2.iterative_schur_solve(p.values, p.b, p.D, preconditioner=R.SCHUR_JACOBI, min_it=k, max_it=k, q_tol=-1.0, r_tol=-1.0)
        assert np.array_equal(x2, xs[(R.SCHUR_JACOBI, k)]), (name, k)


def test_reference_cg_solves_the_dense_system():
    """The restatement's CG, run to convergence on a small dense SPD system, solves it (a check of the reference itself)."""
    rng = np.random.default_rng(1)
    A = rng.standard_normal((30, 30))
    A = A @ A.T + 30 * np.eye(30)
    b = rng.standard_normal(30)
    x, s = R.cg(lambda v: A @ v, b, lambda r: r / np.diag(A), 0, 200, -1.0, 1e-14)
    assert s.termination_type == R.SUCCESS and R.rel(A @ x, b) <= 1e-12
