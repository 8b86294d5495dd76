"""tests/dense_cholesky_reference.py without a device: the schedule restatement against the source it restates, every named condition met
by a size of the table, numpy's own factor and solve within both bounds on every matrix (so a miss on the device is the device's), the
hidden failures' properties, and the measured pivot constant."""
import re

import numpy as np
import pytest

import dense_cholesky_reference as R


def test_constants_are_read_from_the_source():
    k = R.constants()
    assert k["kPanel"] % k["kSub"] == 0 and k["kPanel"] % k["kNb"] == 0
    assert k["look_ahead_min_n"] % (2 * k["kPanel"]) == 0
    text = open(R.KERNELS).read()
    # what the restatement takes for granted about the update kernel: 128 x 128 workgroup tiles, 64 x 64 per wavefront
    assert "const int ib = first + 128 * bi, jb = first + 128 * bj;" in text
    assert "const int i0 = ib + 64 * (wv >> 1), j0 = jb + 64 * (wv & 1);" in text
    assert R.UPDATE_TILE == 128 and R.WAVE_TILE == 64
    # ... and about the loop itself: pairs, the look-ahead only with more than two block columns behind the pair
    assert re.search(r"for \(int k0 = 0; k0 < n; k0 \+= 2 \* kPanel\)", text)
    assert "if (la && blocks > 2) {" in text


def test_the_size_table_is_what_the_conditions_give_today():
    assert R.SIZES == (1, 15, 16, 17, 33, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 383, 384, 385, 513, 1000,
                       3072, 3073, 3201, 3329)
    assert R.GRADED_AND_SCALED_SIZES == (145, 257, 1000, 3201)
    assert R.FROM_MEMORY_SIZES == (129, 145, 257, 1000, 3073)
    assert sorted(R.HIDDEN_FAILURES) == [300, 3201]


@pytest.mark.parametrize("name", list(R.CONDITIONS))
def test_every_named_schedule_condition_is_met_by_a_size_of_the_table(name):
    assert R.sizes_meeting(name), name


def test_every_size_meets_a_condition_no_other_size_of_its_group_meets():
    """No size is in the table for nothing: each is the only one of its group under some condition."""
    for group, sizes in R.SIZE_GROUPS.items():
        for n in sizes:
            own = [name for name in R.CONDITIONS if R.sizes_meeting(name) and n in R.sizes_meeting(name)
                   and not any(m in R.sizes_meeting(name) for m in sizes if m != n)]
            assert own, (group, n)


def test_triangular_solve_edges_are_inside_the_table():
    nb = R.constants()["kNb"]
    for n in (nb + 1, 4 * nb - 1, 4 * nb, 4 * nb + 1):
        assert n in R.SIZES
    kinds = {(l.kernel, l.nb == nb, l.transposed) for n in (33, 127, 128, 129) for l in R.solve_schedule(n)}
    # (a partial block is the last one: forward, nothing lies under it to update)
    assert kinds == {(k, full, t) for k in ("diag", "update") for full in (True, False) for t in (True, False)} - {("update", False, False)}


def test_schedule_covers_every_trailing_entry_exactly_once_per_panel():
    """The restated launches as sets of (entry, panel) updates: every entry (i, j), i >= j, behind a panel takes that panel exactly once,
    and on the side stream only what no launch on the caller's stream touches before the next wait."""
    P = R.constants()["kPanel"]
    for n in R.SIZES:
        sched = R.schedule(n)
        nblk = (n + P - 1) // P
        taken = np.zeros((nblk, nblk, nblk), dtype=int)   # [panel, block row, block column]
        pending_cols = None
        for l in sched:
            if l.kernel == "join":
                pending_cols = None
                continue
            if l.waited:
                pending_cols = None
            if l.kernel in ("potrf", "trsm") and pending_cols is not None:
                assert l.k0 // P < pending_cols, (n, l)      # the panels never run into columns a bulk update still owns
            if l.kernel != "syrk":
                continue
            first = (l.k0 + l.kw) // P
            if l.kw == P:
                cols = [first]
            elif l.stream == "side":
                cols = list(range(first + 2, nblk))
                pending_cols = first + 2
            else:
                cols = list(range(first, min(nblk, first + l.blocks[0])))
                if pending_cols is not None:
                    assert max(cols) < pending_cols or l.waited, (n, l)
            for p in range(l.k0 // P, (l.k0 + l.kw) // P):
                for c in cols:
                    taken[p, c:, c] += 1
        for p in range(nblk):
            for c in range(p + 1, nblk):
                assert (taken[p, c:, c] == 1).all(), (n, p, c)
        assert pending_cols is None, n                          # nothing is left pending when the call returns


@pytest.fixture(scope="module")
def numpy_results():
    out = {}
    for kind in R.KINDS:
        for n in R.SIZES if kind == "random" else R.GRADED_AND_SCALED_SIZES:
            A, b = R.matrix(kind, n)
            L = np.linalg.cholesky(A)                          # raises LinAlgError if A is not positive definite
            out[kind, n] = R.check(A, b, L, np.linalg.solve(A, b)) + (float(np.linalg.eigvalsh(A)[0]) if n <= 1000 and kind == "random" else None,)
    return out


def test_numpy_factor_and_solve_are_within_both_bounds_on_every_matrix(numpy_results):
    bad = {k: v for k, v in numpy_results.items() if not (v[0] <= 1.0 and v[1] <= 1.0)}
    assert not bad, bad
    # positive definite with a margin, not at the edge: the smallest eigenvalue of the random matrices is the 1/2 that was added
    assert all(v[2] >= 0.49 for v in numpy_results.values() if v[2] is not None)


def test_metrics_notice_a_wrong_entry():
    """One entry of L off by 1e-9 relative, one entry of x likewise: far below what 1e-10 on a solution vector sees, far above the bound."""
    for n in (145, 1000):
        A, b = R.matrix("random", n)
        L = np.linalg.cholesky(A)
        x = np.linalg.solve(A, b)
        L2 = L.copy()
        L2[n - 1, n // 2] *= 1.0 + 1e-9
        assert R.factor_backward_error(A, L) <= 1.0 < R.factor_backward_error(A, L2)
        x2 = x.copy()
        x2[np.argmax(np.abs(x))] *= 1.0 + 1e-9
        assert R.solve_residual(A, b, x) <= 1.0 < R.solve_residual(A, b, x2)
    assert R.factor_backward_error(A, np.full_like(L, np.nan)) == np.inf


def test_both_evaluations_of_the_factor_metric_agree():
    """The blocked evaluation (beyond LONGDOUBLE_MAX_N) against the all-longdouble one at a size both can take: it may only read higher, by
    at most its own allowance."""
    n = 400
    A, _ = R.matrix("random", n)
    L = np.linalg.cholesky(A)
    exact = R.factor_backward_error(A, L)
    old = R.LONGDOUBLE_MAX_N
    try:
        R.LONGDOUBLE_MAX_N = 0
        blocked = R.factor_backward_error(A, L)
    finally:
        R.LONGDOUBLE_MAX_N = old
    allowance = R._k_block(n) / (n + 1.0 + R.PIVOT_EXCESS_ULPS)
    assert exact - 1e-12 <= blocked <= exact + 2 * allowance, (exact, blocked)


def test_device_input_keeps_the_upper_triangle_and_nothing_finite_below():
    A, _ = R.matrix("random", 17)
    G = R.device_input(A)
    assert (np.triu(G) == np.triu(A)).all()
    r, c = np.tril_indices(17, -1)
    assert np.isnan(G[r, c][r % 2 == 0]).all() and np.isinf(G[r, c][r % 2 == 1]).all()
    assert (G[r, c][r % 2 == 1] > 0).any() and (G[r, c][r % 2 == 1] < 0).any()


@pytest.mark.parametrize("n", sorted(R.HIDDEN_FAILURES))
def test_hidden_failures_are_indefinite_with_a_positive_diagonal(n):
    A, _ = R.matrix("random", n)
    L = np.linalg.cholesky(A)
    for k in R.HIDDEN_FAILURES[n]:
        B = R.hidden_failure(A, k, L)
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(B)
        if k > 0:   # (k = 0: the leading minor of order 1 is the diagonal entry itself)
            assert (np.diag(B) > 0).all(), (n, k, B[k, k])
            np.linalg.cholesky(B[:k, :k])                                     # the minor of order k is still fine ...
        assert np.linalg.eigvalsh(B[:k + 1, :k + 1])[0] < 0                   # ... the one of order k + 1 is indefinite
        # the pivot the factorisation meets there is -1 up to the rounding of the reference factor
        piv = B[k, k] - float(L[k, :k].astype(np.longdouble) @ L[k, :k].astype(np.longdouble))
        assert abs(piv + 1.0) <= 1e-9 * A[k, k]


def test_measured_pivot_excess_is_under_the_constant():
    """The device's pivot arithmetic restated: how far d y and s y are from sqrt(d) and s / sqrt(d), in units of u (the design note has the
    figures).  The constant added to (n + 1) is that count rounded up."""
    diag, offdiag, block = R.pivot_rounding_excess()
    assert max(diag, offdiag) <= R.PIVOT_EXCESS_ULPS <= np.ceil(max(diag, offdiag)) + 1, (diag, offdiag)
    assert block <= R.PIVOT_EXCESS_ULPS, block
