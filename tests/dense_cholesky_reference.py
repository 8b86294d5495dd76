"""The dense Cholesky of csrc/kernels_schur.hip (LaunchDenseCholesky / LaunchDenseCholeskySolve) held to its factor: the launch
schedule restated, the sizes at which that schedule changes shape, the matrices, and two backward-error metrics with bounds from
theory (design/24_dense_cholesky_tests.md).  numpy only; tests/test_dense_cholesky_cpu.py covers this file without a device,
tests/test_gpu_dense_cholesky.py runs the kernels against it."""
import collections
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "ceres-solver_amd", "csrc", "kernels_schur.hip")
U = 2.0 ** -53          # unit roundoff of float64


@functools.lru_cache(maxsize=None)
def constants():
    """kPanel, kSub, kNb and the look-ahead threshold of kernels_schur.hip, by name (parsed, never repeated)."""
    with open(KERNELS) as f:
        text = f.read()
    k = {name: int(v) for name, v in re.findall(r"constexpr\s+int\s+(kPanel|kSub|kNb)\s*=\s*(\d+)\s*;", text)}
    for name in ("kPanel", "kSub", "kNb"):
        assert name in k, name
    m = re.search(r"n\s*>=\s*(\d+)\s*\*\s*kPanel\s*\?\s*look_ahead_for_current_device\(\)", text)
    assert m, "the look-ahead threshold of LaunchDenseCholesky"
    k["look_ahead_min_n"] = int(m.group(1)) * k["kPanel"]
    k["from_memory_switch"] = "CERES_HIP_AB_TRSM_GLOBAL" in text   # whether the from-memory substitution kernel is still selectable
    return k


# ---- the schedule, restated ---------------------------------------------------------------------------------------------------------------
# kernel: 'potrf' (the diagonal block), 'trsm' (the rows under a full panel), 'syrk' (a trailing update over kw panel columns from k0).
# rest: the rows behind the panel(s).  blocks: the grid.  stream: 'main' (the caller's) or 'side'.  waited: the launch was preceded by a
# wait on the side stream's bulk event (a bulk update was pending).
Launch = collections.namedtuple("Launch", "kernel k0 kw rest blocks stream waited")
UPDATE_TILE = 128       # the trailing update's workgroup tile; a wavefront takes a quarter of it
WAVE_TILE = UPDATE_TILE // 2


def schedule(n):
    """LaunchDenseCholesky's loop: panels in pairs, the second panel's columns updated by the first alone (K = kPanel), everything behind
    the pair by both at once (K = 2 kPanel) - from look_ahead_min_n columns on split into the next pair's two block columns on the
    caller's stream and the bulk behind them on a side stream."""
    k = constants()
    P, S = k["kPanel"], k["kSub"]
    out = []
    look_ahead = n >= k["look_ahead_min_n"]
    pending = False

    def panel(k0, kw):
        rest = n - k0 - kw
        out.append(Launch("potrf", k0, kw, rest, (1, 1), "main", False))
        if rest > 0:
            out.append(Launch("trsm", k0, P, rest, (min((rest + 63) // 64, 256), 1), "main", False))
        return rest

    k0 = 0
    while k0 < n:
        rest0 = panel(k0, min(n - k0, P))
        if rest0 <= 0:
            break
        out.append(Launch("syrk", k0, P, rest0, (1, (rest0 + UPDATE_TILE - 1) // UPDATE_TILE), "main", False))
        k1 = k0 + P
        rest1 = panel(k1, min(n - k1, P))
        if rest1 <= 0:
            break
        blocks = (rest1 + UPDATE_TILE - 1) // UPDATE_TILE
        if look_ahead and blocks > 2:
            out.append(Launch("syrk", k0, 2 * P, rest1, (2, blocks), "main", pending))
            out.append(Launch("syrk", k0, 2 * P, rest1, (blocks - 2, blocks), "side", False))
            pending = True
        else:
            out.append(Launch("syrk", k0, 2 * P, rest1, (blocks, blocks), "main", pending))
            pending = False
        k0 += 2 * P
    if pending:
        out.append(Launch("join", n, 0, 0, (0, 0), "main", True))
    assert S > 0
    return out


SolveLaunch = collections.namedtuple("SolveLaunch", "kernel k0 nb rest transposed")


def solve_schedule(n):
    """LaunchDenseCholeskySolve: forward then backward substitution in blocks of kNb."""
    nb_ = constants()["kNb"]
    out = []
    for k0 in range(0, n, nb_):
        nb = min(n - k0, nb_)
        out.append(SolveLaunch("diag", k0, nb, n - k0 - nb, False))
        if n - k0 - nb > 0:
            out.append(SolveLaunch("update", k0, nb, n - k0 - nb, False))
    for k0 in range((n - 1) // nb_ * nb_, -1, -nb_):
        nb = min(n - k0, nb_)
        out.append(SolveLaunch("diag", k0, nb, k0, True))
        if k0 > 0:
            out.append(SolveLaunch("update", k0, nb, k0, True))
    return out


def _of(sched, kernel, stream=None):
    return [l for l in sched if l.kernel == kernel and (stream is None or l.stream == stream)]


def _second_of_pair(l):
    P = constants()["kPanel"]
    return l.k0 % (2 * P) == P


def _side_launches_at_threshold():
    return len(_of(schedule(constants()["look_ahead_min_n"]), "syrk", "side"))


def _conditions():
    k = constants()
    P, S, NB = k["kPanel"], k["kSub"], k["kNb"]
    potrf = lambda s: _of(s, "potrf")
    trsm = lambda s: _of(s, "trsm")
    pair_update = lambda s: [l for l in _of(s, "syrk") if l.kw == 2 * P]
    panel_update = lambda s: [l for l in _of(s, "syrk") if l.kw == P]
    la = lambda s: bool(_of(s, "syrk", "side"))
    return collections.OrderedDict([
        # ---- inside one diagonal block
        ("a_single_entry", lambda n, s: len(potrf(s)) == 1 and potrf(s)[0].kw == 1),
        ("one_step_one_row_short", lambda n, s: len(potrf(s)) == 1 and potrf(s)[0].kw == S - 1),
        ("one_step_exact", lambda n, s: len(potrf(s)) == 1 and n == S),
        ("two_steps_last_one_padded_with_the_identity", lambda n, s: len(potrf(s)) == 1 and S < n < 2 * S),
        ("three_steps_one_row_in_the_last", lambda n, s: len(potrf(s)) == 1 and n == 2 * S + 1),
        ("narrow_single_panel_no_inverses_parked", lambda n, s: len(potrf(s)) == 1 and potrf(s)[0].kw == P - 1),
        ("full_panel_inverses_parked_nothing_below", lambda n, s: potrf(s)[-1].kw == P and potrf(s)[-1].rest == 0 and len(potrf(s)) == 1),
        # ---- rows under a full panel: the substitution kernel's strips
        ("one_row_under_a_full_panel", lambda n, s: any(l.rest == 1 for l in trsm(s))),
        ("last_strip_one_row_short", lambda n, s: any(l.rest % S == S - 1 for l in trsm(s))),
        ("strips_exact", lambda n, s: len(trsm(s)) == 1 and trsm(s)[0].rest == S),
        ("one_row_in_a_second_strip", lambda n, s: any(l.rest == S + 1 for l in trsm(s))),
        # ---- the trailing update's 64 x 64 wave tiles
        ("update_one_row_short_of_a_wave_tile", lambda n, s: any(l.rest == WAVE_TILE - 1 for l in panel_update(s))),
        ("update_exactly_a_wave_tile", lambda n, s: any(l.rest == WAVE_TILE for l in panel_update(s))),
        ("update_one_row_into_the_second_wave_tile", lambda n, s: any(l.rest == WAVE_TILE + 1 for l in panel_update(s))),
        # ---- pair edges
        ("second_panel_one_column_short", lambda n, s: any(_second_of_pair(l) and l.kw == P - 1 for l in potrf(s))),
        ("pair_ends_exactly_inverses_parked_nothing_below", lambda n, s: len(potrf(s)) == 2 and potrf(s)[1].kw == P and potrf(s)[1].rest == 0),
        ("one_row_behind_a_pair", lambda n, s: any(l.rest == 1 for l in pair_update(s))),
        ("third_panel_one_column_short", lambda n, s: len(potrf(s)) == 3 and potrf(s)[2].kw == P - 1),
        ("third_panel_full_and_last", lambda n, s: len(potrf(s)) == 3 and potrf(s)[2].kw == P and potrf(s)[2].rest == 0),
        ("second_pair_one_row_behind_its_first_panel", lambda n, s: any(l.k0 == 2 * P and l.rest == 1 for l in trsm(s))),
        # ---- more than one block column in the K = 2 kPanel update, one stream
        ("pair_update_one_row_into_a_third_block", lambda n, s: not la(s) and any(l.rest == 2 * UPDATE_TILE + 1 and l.blocks == (3, 3) for l in pair_update(s))),
        ("several_pairs_without_look_ahead", lambda n, s: not la(s) and len(pair_update(s)) >= 3),
        # ---- look-ahead
        ("look_ahead_exact_pairs_tail_update_waits_for_the_bulk",
         lambda n, s: la(s) and n % (2 * P) == 0 and any(l.waited and l.stream == "main" and l.blocks[0] == l.blocks[1] for l in pair_update(s))),
        ("look_ahead_pair_update_waits_for_the_previous_bulk", lambda n, s: any(l.waited and l.blocks[0] == 2 and l.blocks[1] > 2 for l in pair_update(s))),
        ("look_ahead_last_bulk_is_one_block_column_one_row_high",
         lambda n, s: la(s) and _of(s, "syrk", "side")[-1].blocks[0] == 1 and _of(s, "syrk", "side")[-1].rest == 2 * UPDATE_TILE + 1),
        ("look_ahead_one_bulk_more_than_at_the_threshold_last_panel_one_wide_first_of_its_pair",
         lambda n, s: len(_of(s, "syrk", "side")) == _side_launches_at_threshold() + 1 and potrf(s)[-1].kw == 1 and not _second_of_pair(potrf(s)[-1])),
        ("look_ahead_last_panel_one_wide_second_of_its_pair", lambda n, s: la(s) and potrf(s)[-1].kw == 1 and _second_of_pair(potrf(s)[-1])),
        ("look_ahead_odd_number_of_full_panels", lambda n, s: la(s) and sum(l.kw == P for l in potrf(s)) % 2 == 1),
        ("look_ahead_two_more_bulks_than_at_the_threshold", lambda n, s: len(_of(s, "syrk", "side")) >= _side_launches_at_threshold() + 2),
        # ---- the triangular solves' blocks of kNb
        ("solve_one_row_in_the_last_block", lambda n, s: n > NB and n % NB == 1),
        ("solve_last_block_one_row_short", lambda n, s: n > NB and n % NB == NB - 1),
        ("solve_blocks_exact", lambda n, s: n > NB and n % NB == 0),
        ("solve_single_block", lambda n, s: n <= NB),
    ])


CONDITIONS = _conditions()


def _sizes():
    k = constants()
    P, S, T = k["kPanel"], k["kSub"], k["look_ahead_min_n"]
    return collections.OrderedDict([
        ("inside_one_diagonal_block", (1, S - 1, S, S + 1, 2 * S + 1, P - 1, P)),
        ("under_a_full_panel", (P + 1, P + S - 1, P + S, P + S + 1)),
        ("trailing_tile_edges", (P + WAVE_TILE - 1, P + WAVE_TILE, P + WAVE_TILE + 1)),
        ("pair_edges", (2 * P - 1, 2 * P, 2 * P + 1, 3 * P - 1, 3 * P, 3 * P + 1)),
        ("two_update_block_columns", (4 * P + 1, 1000)),   # 1000: the old test's largest size (three pairs and a ragged fourth)
        ("look_ahead", (T, T + 1, T + P + 1, T + 2 * P + 1)),
    ])


SIZE_GROUPS = _sizes()
SIZES = tuple(n for group in SIZE_GROUPS.values() for n in group)
LOOK_AHEAD_SIZES = SIZE_GROUPS["look_ahead"]
SMALL_SIZES = tuple(n for n in SIZES if n not in LOOK_AHEAD_SIZES)
GRADED_AND_SCALED_SIZES = (SIZE_GROUPS["under_a_full_panel"][3], SIZE_GROUPS["pair_edges"][2], SIZE_GROUPS["two_update_block_columns"][1],
                           LOOK_AHEAD_SIZES[2])
FROM_MEMORY_SIZES = (SIZE_GROUPS["under_a_full_panel"][0], SIZE_GROUPS["under_a_full_panel"][3], SIZE_GROUPS["pair_edges"][2],
                     SIZE_GROUPS["two_update_block_columns"][1], LOOK_AHEAD_SIZES[1])


def sizes_meeting(name):
    return [n for n in SIZES if CONDITIONS[name](n, schedule(n))]


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------
KINDS = ("random", "graded", "scaled_up", "scaled_down")
SCALE = 4.0 ** 150


@functools.lru_cache(maxsize=4)
def _random(n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n + 3))
    A = M @ M.T + 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


def matrix(kind, n):
    """(A, b): A symmetric positive definite with a margin, both triangles filled; seeded by n.
    random: M M^T + I / 2 with M n x (n + 3).  graded: D A D, D = 10^linspace(-6, 6) (the spread of an unscaled Schur complement), b
    scaled by D.  scaled_up / scaled_down: A and b times 4^150 / 4^-150 (exact: powers of two)."""
    A, b = _random(n)
    if kind == "random":
        return A, b
    if kind == "graded":
        d = 10.0 ** np.linspace(-6.0, 6.0, n)
        G = d[:, None] * A * d[None, :]
        return (G + G.T) / 2.0, d * b
    if kind == "scaled_up":
        return A * SCALE, b * SCALE
    if kind == "scaled_down":
        return A / SCALE, b / SCALE
    raise KeyError(kind)


def device_input(A):
    """What the device is handed: the upper triangle of A, and below the diagonal NaN in the even rows, +-Inf in the odd rows."""
    n = A.shape[0]
    out = np.triu(A)
    r, c = np.tril_indices(n, -1)
    out[r, c] = np.where(r % 2 == 0, np.nan, np.where(c % 2 == 0, np.inf, -np.inf))
    return out


def hidden_failure(A, k, L=None):
    """A with A[k, k] lowered by (pivot k of the reference factor)^2 + 1: the leading minor of order k + 1 turns indefinite (its last
    pivot becomes -1) while, for k > 0 and a row with enough weight left of the diagonal, every diagonal entry stays positive - nothing
    a look at the diagonal would find.  (k = 0: the minor IS the diagonal entry, which becomes -1.)"""
    L = np.linalg.cholesky(A) if L is None else L
    B = A.copy()
    B[k, k] -= L[k, k] ** 2 + 1.0
    return B


HIDDEN_FAILURES = {300: (0, 5, 20, 127, 128, 130, 256, 299), SIZE_GROUPS["look_ahead"][2]: (3071, 3200)}


# ---- metrics --------------------------------------------------------------------------------------------------------------------------------
# c: what the device's pivot arithmetic (one reciprocal square root, refined, and multiplications by it - no sqrt, no divide) adds to the
# (n + 1) of Higham's componentwise bound, in units of u.  Measured by pivot_rounding_excess() below; tests/test_dense_cholesky_cpu.py holds
# the measurement under this constant.
PIVOT_EXCESS_ULPS = 4
LONGDOUBLE_MAX_N = 400       # up to here L L^T is formed entirely in longdouble
EVALUATION_SHARE = 0.05      # beyond: float64 products over k-blocks this share of (n + 1) wide at most, block sums added in longdouble


def _k_block(n):
    kb = 1
    while 2 * kb <= min(128.0, EVALUATION_SHARE * (n + 1)):
        kb *= 2
    return kb


def factor_backward_error(A, F):
    """max over i >= j of |A - L L^T|_ij / ((n + 1 + c) u (|L| |L^T|)_ij), L = the lower triangle of F.  Higham (Accuracy and Stability of
    Numerical Algorithms, Theorem 10.3) bounds |A - L L^T| by gamma_{n+1} |L| |L^T| for any order of the sums: the value is <= 1 / (1 - (n +
    1) u) for a correct factorisation.  Up to LONGDOUBLE_MAX_N the product is formed in longdouble.  Beyond, the products of kb columns at
    a time are float64 (BLAS) and their sums longdouble: the evaluation's own error is at most kb u (|L| |L^T|)_ij, and kb / (n + 1 + c)
    is ADDED to the returned value - the test can only get stricter by it.  Returns inf for a factor with a NaN or Inf in it."""
    n = A.shape[0]
    L = np.tril(F)
    if not np.isfinite(L).all():
        return np.inf
    scale = (n + 1 + PIVOT_EXCESS_ULPS) * U
    aL = np.abs(L)
    worst = 0.0
    if n <= LONGDOUBLE_MAX_N:
        Ll = L.astype(np.longdouble)
        R = np.abs(A.astype(np.longdouble) - Ll @ Ll.T)
        den = np.abs(Ll) @ np.abs(Ll).T
        i, j = np.tril_indices(n)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = R[i, j] / den[i, j]
        q = np.where(den[i, j] == 0, np.where(R[i, j] == 0, 0.0, np.inf), q)
        return float(q.max() / scale)
    kb = _k_block(n)
    rows = 512
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        acc = np.zeros((r1 - r0, r1), dtype=np.longdouble)
        for c0 in range(0, r1, kb):
            acc += L[r0:r1, c0:c0 + kb] @ L[:r1, c0:c0 + kb].T
        R = np.abs(A[r0:r1, :r1].astype(np.longdouble) - acc)
        den = aL[r0:r1, :r1] @ aL[:r1, :r1].T          # (float64: a relative error of n u in the denominator)
        keep = np.arange(r1)[None, :] <= np.arange(r0, r1)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(keep, R / den, 0.0)
        q = np.where(keep & (den == 0), np.where(R == 0, 0.0, np.inf), q)
        worst = max(worst, float(q.max()))
    return worst / scale + kb / (n + 1.0 + PIVOT_EXCESS_ULPS)


def solve_residual(A, b, x):
    """|b - A x|_inf / ((|A|_inf |x|_inf + |b|_inf) n u): the normwise backward error of the solve in units of n u, the product in
    longdouble.  A backward stable solve stays under 1.  inf for an x that is not finite."""
    n = A.shape[0]
    if not np.isfinite(x).all():
        return np.inf
    xl = x.astype(np.longdouble)
    r = np.empty(n, dtype=np.longdouble)
    for r0 in range(0, n, 256):
        r[r0:r0 + 256] = b[r0:r0 + 256].astype(np.longdouble) - A[r0:r0 + 256].astype(np.longdouble) @ xl
    den = (np.abs(A).sum(axis=1).max().astype(np.longdouble) * np.abs(xl).max() + np.abs(b).max()) * n * U
    return float(np.abs(r).max() / den)


def check(A, b, F, x):
    """(factor backward error, solve residual): both must be <= 1."""
    return factor_backward_error(A, F), solve_residual(A, b, x)


# ---- the pivot arithmetic, restated -----------------------------------------------------------------------------------------------------------
def _device_pivot(d, seed_error, rng):
    """One pivot as dense_potrf_panel_kernel computes it, in float64: y ~ d^-1/2 from a seed refined by two Newton steps, L_jj = d y
    corrected once.
    The hardware seed is modelled as the correctly rounded value times (1 + e), |e| <= seed_error."""
    y = np.float64(1.0) / np.sqrt(d) * (1.0 + seed_error * rng.uniform(-1.0, 1.0, size=d.shape))
    for _ in range(2):
        y = y * (1.5 - 0.5 * d * y * y)
    l = d * y
    # one correction step from the residual d - l^2 (two FMAs on the device; longdouble stands in for the exact product)
    r = (d.astype(np.longdouble) - l.astype(np.longdouble) ** 2).astype(np.float64)
    return y, (l.astype(np.longdouble) + r.astype(np.longdouble) * (0.5 * y).astype(np.longdouble)).astype(np.float64)


def pivot_rounding_excess(samples=200_000, seed=7):
    """What the multiplied form costs against sqrt and divide, in units of u: max of |L_jj^2 - d| / (u d) (Higham's sqrt: 2) and of
    |l L_jj - s| / (u |s|) for l = fl(s y) (Higham's divide: 1), over pivots d spread across many binades and sums s, plus the same
    recurrence run on whole 16 x 16 blocks, n = 1 .. kSub, against the exact factor in longdouble.  Returns (diag, offdiag, block)."""
    rng = np.random.default_rng(seed)
    d = np.exp2(rng.uniform(-600.0, 600.0, samples))
    s = rng.standard_normal(samples) * np.sqrt(d)
    worst_d = worst_o = 0.0
    for seed_error in (0.0, 2.0 ** -40, 2.0 ** -26):
        y, ljj = _device_pivot(d, seed_error, rng)
        dl, sl = d.astype(np.longdouble), s.astype(np.longdouble)
        worst_d = max(worst_d, float((np.abs(ljj.astype(np.longdouble) ** 2 - dl) / (U * dl)).max()))
        l = s * y
        worst_o = max(worst_o, float((np.abs(l.astype(np.longdouble) * ljj.astype(np.longdouble) - sl) / (U * np.abs(sl))).max()))
    # whole sub-blocks: the recurrence of the kernel (column j scaled by y_j, the columns to its right updated) on n = 1 .. kSub
    worst_b = 0.0
    S = constants()["kSub"]
    for n in range(1, S + 1):
        for trial in range(40):
            M = rng.standard_normal((n, n + 3))
            A = M @ M.T + 0.5 * np.eye(n)
            T = np.tril(A).copy()
            for j in range(n):
                y, ljj = _device_pivot(T[j:j + 1, j], 2.0 ** -26, rng)
                T[j, j] = ljj[0]
                T[j + 1:, j] *= y[0]
                for c in range(j + 1, n):
                    T[c:, c] -= T[c:, j] * T[c, j]
            Ll = T.astype(np.longdouble)
            R = np.abs(np.tril(A).astype(np.longdouble) - np.tril(Ll @ Ll.T))
            den = np.abs(Ll) @ np.abs(Ll).T
            worst_b = max(worst_b, float((R / (U * den)).max()) - (n + 1))
    return worst_d, worst_o, worst_b
