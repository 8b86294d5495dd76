"""What a call does depends on its own arguments only (design/21_solve_context.md): one handle runs a sequence of LM steps, operator-level
calls and plain solves that take different ways through the solve, and every result is held to the same call on a fresh handle.

The bound is the rule of tests/test_gpu_point_tail.py::compare: ten times what two fresh handles differ by between themselves (their
LDS sums add in arrival order), or 1e-11, whichever is larger; iteration counts and termination types are equal.

The handle's options are fixed at creation, so the step that back-substitutes over J is pushed past kPointTailMaxIterations by its
tolerance (eta = 1e-8, as in test_route_does_not_depend_on_earlier_solves).  The step with reuse_diagonal needs a diagonal to reuse:
its fresh handles have run the first step, and nothing else, before it."""
import functools

import numpy as np
import pytest

from test_gpu_operators import rel
from test_gpu_point_tail import ETA, K, RADIUS, SCHUR, SCHUR_JACOBI, cameras_scene, lm_diag

pytestmark = pytest.mark.gpu
CGNR, JACOBI = 6, 1


@functools.lru_cache(maxsize=None)
def scene(problems, oracle, n_cams):
    """The scene, the caller's D of the plain solve and of the operator-level calls, and an F-space vector for them."""
    p = cameras_scene(problems, n_cams)
    z = np.random.default_rng(5).standard_normal(9 * n_cams)
    return p, lm_diag(oracle, p, RADIUS), z


def new_handle(hip, monkeypatch, p, solver, pre):
    for name in ("CERES_HIP_POINT_TAIL", "CERES_HIP_FUSED_GRID", "CERES_HIP_SPECULATE"):
        monkeypatch.delenv(name, raising=False)
    o = hip.LinearSolverOptions(type=solver, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=500,
                                elimination_groups=[p.num_eliminate_blocks])
    s = hip.HipLinearSolver(o)
    s.set_structure(p.bs)
    assert s.info().kernel_path == hip.PATH_BAL
    return s


# ---- the calls: each returns (vectors, scalars, (iterations, termination type) or None) ---------------------------------------------------
def lm(s, p, radius, eta, **kw):
    step, summ, mcc = s.lm_compute_step(p.values, p.b, radius, eta, **kw)
    return [step], [mcc], (summ.num_iterations, summ.termination_type)


def first_step(hip, s, p, Dv, z):
    return lm(s, p, RADIUS, ETA)


def operators(hip, s, p, Dv, z):
    s.load(p.values, p.b, Dv)
    s.schur_init()
    return [s.schur_rhs(), s.schur_sx(z), s.back_substitute(z)], [], None


def plain_solve(hip, s, p, Dv, z):
    x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=Dv, q_tolerance=ETA, r_tolerance=-1.0))
    return [x], [], (summ.num_iterations, summ.termination_type)


def reuse_step(hip, s, p, Dv, z):
    return lm(s, p, RADIUS / 8, ETA, reuse_diagonal=True)


def long_step(hip, s, p, Dv, z):
    return lm(s, p, RADIUS, 1e-8)


# (the call, the route the handle reports after it — None: unchanged —, the calls its fresh handles run before it)
SCHUR_SEQUENCE = [(first_step, 1, []), (operators, None, []), (plain_solve, 1, []), (reuse_step, 1, [first_step]), (long_step, 0, []),
                  (first_step, 1, [])]
CGNR_SEQUENCE = [(first_step, None, []), (plain_solve, None, []), (reuse_step, None, [first_step]), (first_step, None, [])]


def fresh_result(hip, monkeypatch, p, Dv, z, solver, pre, call, before):
    s = new_handle(hip, monkeypatch, p, solver, pre)
    for c in before:
        c(hip, s, p, Dv, z)
    r = call(hip, s, p, Dv, z)
    s.close()
    return r


def hold(case, used, fresh_a, fresh_b):
    assert used[2] == fresh_a[2] == fresh_b[2], (case, used[2], fresh_a[2], fresh_b[2])
    figures = []
    for u, a, b in zip(used[0], fresh_a[0], fresh_b[0]):
        assert np.isfinite(u).all(), case
        figures.append((rel(u, a), rel(a, b)))
    for u, a, b in zip(used[1], fresh_a[1], fresh_b[1]):
        figures.append((abs(u - a) / abs(a), abs(a - b) / abs(b)))
    print(case, " ".join(f"used_fresh={d:.3e}/fresh_fresh={sp:.3e}" for d, sp in figures), flush=True)
    for d, sp in figures:
        assert d <= max(10 * sp, 1e-11), (case, d, sp)


@pytest.mark.parametrize("n_cams", [40, 80])
@pytest.mark.parametrize("solver,pre,sequence", [(SCHUR, SCHUR_JACOBI, SCHUR_SEQUENCE), (CGNR, JACOBI, CGNR_SEQUENCE)], ids=["schur", "cgnr"])
def test_results_do_not_depend_on_earlier_calls(hip, oracle, problems, monkeypatch, n_cams, solver, pre, sequence):
    """40 cameras: the S.x pass finishes the CG iteration itself; 80: the separate CG kernels.  ITERATIVE_SCHUR: an LM step that takes the
    point tail, Schur init + S.x + back-substitution as operators, a plain solve, an LM step with reuse_diagonal, an LM step that goes past
    kPointTailMaxIterations and back-substitutes over J, and the first step again.  CGNR + JACOBI: the steps and the solve."""
    p, Dv, z = scene(problems, oracle, n_cams)
    used = new_handle(hip, monkeypatch, p, solver, pre)
    route = used.last_backsub_route()
    for k, (call, want_route, before) in enumerate(sequence):
        got = call(hip, used, p, Dv, z)
        if solver == SCHUR:
            route = route if want_route is None else want_route
            assert used.last_backsub_route() == route, (k, call.__name__, used.last_backsub_route(), route)
            if call is long_step:
                assert got[2][0] > K, got[2]
            elif got[2] is not None:
                assert got[2][0] <= K, got[2]
        fresh = [fresh_result(hip, monkeypatch, p, Dv, z, solver, pre, call, before) for _ in range(2)]
        hold(f"{'schur' if solver == SCHUR else 'cgnr'}_{n_cams}_{k}_{call.__name__}", got, *fresh)
    used.close()
