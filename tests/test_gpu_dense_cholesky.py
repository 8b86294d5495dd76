"""LaunchDenseCholesky / LaunchDenseCholeskySolve (csrc/kernels_schur.hip) held to the factor itself, at every size where the launch
schedule changes shape (tests/dense_cholesky_reference.py, design/24_dense_cholesky_tests.md): the componentwise backward error of L
and the residual of x against bounds from theory, guard bands around the matrix and the vector, bit-identical repeats, pivots that
fail where a look at the diagonal finds nothing, four factorisations at once on the shared look-ahead stream, DENSE_SCHUR with 343
cameras through the public API, and the from-memory substitution kernel in a child interpreter."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import dense_cholesky_reference as R
import schur_dense_reference as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_TOL = 1e-10     # a solve against the dense reference (tests/test_gpu_schur_state.py, tests/test_gpu_explicit_schur.py)
STEP_TOL = 1e-9       # an LM step against it


def new_handle(hip):
    return hip.HipLinearSolver(hip.LinearSolverOptions(type=hip.DENSE_SCHUR, elimination_groups=[1], max_num_iterations=1))


@pytest.fixture(scope="module")
def handle(hip):
    s = new_handle(hip)
    yield s
    s.close()


def measure(s, kind, n, repeats=2):
    """One matrix of the table through the debug entry: {failed, guard, same, factor, residual}."""
    A, b = R.matrix(kind, n)
    F, x, failed, changed, same = s.dense_cholesky_factor(R.device_input(A), b, repeats=repeats)
    return evaluate(kind, n, F, x, failed, changed, same)


def evaluate(kind, n, F, x, failed, changed, same):
    A, b = R.matrix(kind, n)
    fe, sr = (np.inf, np.inf) if failed else R.check(A, b, F, x)
    out = dict(kind=kind, n=n, failed=bool(failed), guard=int(changed), same=bool(same), factor=fe, residual=sr)
    print("dense_cholesky", json.dumps(out), flush=True)
    return out


def bad_of(res):
    """What of a result misses: the flag clear, both metrics within 1, no guard word changed, the repeats bit-identical."""
    bad = {}
    if res["failed"]:
        bad["failed"] = True
    if res["guard"] != 0:
        bad["guard"] = res["guard"]
    if not res["same"]:
        bad["same"] = False
    for key in ("factor", "residual"):
        if not res[key] <= 1.0:
            bad[key] = res[key]
    return bad


@pytest.mark.parametrize("n", R.SIZES)
def test_every_size_of_the_table_on_the_random_matrix(handle, n):
    res = measure(handle, "random", n)
    assert not bad_of(res), res


@pytest.mark.parametrize("n", R.GRADED_AND_SCALED_SIZES)
@pytest.mark.parametrize("kind", [k for k in R.KINDS if k != "random"])
def test_graded_and_scaled_matrices(handle, kind, n):
    res = measure(handle, kind, n)
    assert not bad_of(res), res


# ---- pivots that fail ---------------------------------------------------------------------------------------------------------------------
def probes(n, positions):
    """(name, k, edit): the old test's -1 on the diagonal, a NaN on the diagonal, a NaN in the upper triangle beside it."""
    out = []
    for k in positions:
        j = k + 1 if k + 1 < n else k - 1
        out.append(("minus_one", k, lambda G, k=k: G.__setitem__((k, k), -1.0)))
        out.append(("nan_diagonal", k, lambda G, k=k: G.__setitem__((k, k), np.nan)))
        out.append(("nan_upper", k, lambda G, k=k, j=j: G.__setitem__((min(k, j), max(k, j)), np.nan)))
    return out


@pytest.mark.parametrize("n", sorted(R.HIDDEN_FAILURES))
def test_failing_pivots_raise_the_flag_and_the_handle_goes_on(handle, n):
    """An indefinite leading minor under a positive diagonal, in the first and a later 16-wide step, in the second panel, behind a pair,
    in the narrow last panel; at the look-ahead size in the last full panel and the 1-wide one behind it."""
    A, b = R.matrix("random", n)
    L = np.linalg.cholesky(A)
    missed = []
    for k in R.HIDDEN_FAILURES[n]:
        _, x, failed, changed, _ = handle.dense_cholesky_factor(R.device_input(R.hidden_failure(A, k, L)), b)
        if not failed or changed or not (x == b).all():   # (no solve behind a refused pivot: x is b)
            missed.append(("hidden", k, failed, changed))
    P = R.constants()["kPanel"]
    regions = (5, 20, P + 2, 2 * P + 1, n - 1) if n == 300 else (n - 1,)   # one position per region
    for name, k, edit in probes(n, regions):
        G = R.device_input(A)
        edit(G)
        _, _, failed, changed, _ = handle.dense_cholesky_factor(G, b)
        if not failed or changed:
            missed.append((name, k, failed, changed))
    assert not missed, missed
    res = measure(handle, "random", n, repeats=1)   # the same handle, the clean matrix
    assert not bad_of(res), res


# ---- four factorisations at once ------------------------------------------------------------------------------------------------------------
def test_four_handles_on_four_threads_share_the_look_ahead_stream(hip):
    """Three factorisations with look-ahead and one without, each on its own handle and host thread, started from one barrier, three
    repeats each: the side stream, its two events and the enqueue lock are per device, not per handle.  A thread still alive at the
    time-out is a failure to investigate, not to rerun."""
    la = R.LOOK_AHEAD_SIZES
    sizes = (la[2], la[3], la[0], 300)
    inputs = {n: (R.device_input(R.matrix("random", n)[0]), R.matrix("random", n)[1]) for n in sizes}
    handles = {n: new_handle(hip) for n in sizes}
    results, errors = {}, []
    start = threading.Barrier(len(sizes))

    def work(n):
        try:
            start.wait(timeout=60)
            results[n] = handles[n].dense_cholesky_factor(inputs[n][0], inputs[n][1], repeats=3)
        except BaseException as ex:  # noqa: BLE001 - reported by the main thread
            errors.append((n, repr(ex)))

    threads = [threading.Thread(target=work, args=(n,), name=f"cholesky{n}") for n in sizes]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a factorisation hangs"
    for s in handles.values():
        s.close()
    assert not errors, errors
    bad = {n: bad_of(evaluate("random", n, *results[n])) for n in sizes}
    assert not any(bad.values()), bad


# ---- through the public API -------------------------------------------------------------------------------------------------------------------
def test_dense_schur_with_343_cameras_takes_the_look_ahead(hip, problems):
    """DENSE_SCHUR on 343 cameras = 3087 reduced columns (the look-ahead starts at 3072) against numpy's solve of the dense S and rhs of
    tests/schur_dense_reference.py, then an LM step on the same handle: the factorisation runs twice on a live solver."""
    p = problems.synthetic_bal(None, layout="schur", num_cameras=343, num_points=500, num_observations=6000, seed=41)
    ref = SR.SchurReference(p)
    assert ref.nf == 343 * 9 >= R.constants()["look_ahead_min_n"]
    assert any(l.stream == "side" for l in R.schedule(ref.nf))
    s = hip.HipLinearSolver(hip.LinearSolverOptions(type=hip.DENSE_SCHUR, elimination_groups=[p.num_eliminate_blocks], max_num_iterations=1))
    s.set_structure(p.bs)
    x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D))
    assert summ.termination_type == hip.SUCCESS, summ
    want = ref.back_substitute(np.linalg.solve(ref.dense_S(), ref.rhs()))
    err = SR.rel(x, want)
    radius = 1e4
    step, summ2, mcc = s.lm_compute_step(p.values, p.b, radius)
    s.close()
    assert summ2.termination_type == hip.SUCCESS and np.isfinite(step).all(), summ2
    ref_lm = ref.with_D(np.sqrt(np.clip(ref.squared_column_norm(), 1e-6, 1e32) / radius))
    want_lm = ref_lm.back_substitute(np.linalg.solve(ref_lm.dense_S(), ref_lm.rhs()))
    err_lm = SR.rel(-step, want_lm)
    want_mcc = ref_lm.model_cost_change(-want_lm)
    print("dense_cholesky", json.dumps(dict(api_solve=err, api_lm_step=err_lm, mcc=mcc, want_mcc=want_mcc)), flush=True)
    assert err <= SOLVE_TOL and err_lm <= STEP_TOL, (err, err_lm)
    assert abs(mcc - want_mcc) <= STEP_TOL * abs(want_mcc), (mcc, want_mcc)


# ---- the from-memory substitution kernel ----------------------------------------------------------------------------------------------------
def child_main():
    """In the child interpreter (CERES_HIP_AB_TRSM_GLOBAL=1, read once per process): the sizes with rows under a full panel; one JSON line
    each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library, as tests/test_gpu_dispatch.py loads it)
    import __graft_entry__ as entry
    hip = entry.load_package().hip_solver
    hip.load_library()
    s = new_handle(hip)
    failed = 0
    for n in R.FROM_MEMORY_SIZES:
        res = measure(s, "random", n)
        bad = bad_of(res)
        failed += bool(bad)
        print(json.dumps({"n": n, "bad": bad}), flush=True)
    s.close()
    return 1 if failed else 0


def test_from_memory_substitution_kernel_in_a_child(hip):
    """dense_trsm_mfma_kernel (every operand of the substitution straight from memory) is selected by an environment switch that the
    library reads once: a fresh child interpreter, the same checks.  A signal or a time-out is a failure to investigate, not to rerun."""
    assert R.constants()["from_memory_switch"]
    env = dict(os.environ, CERES_HIP_AB_TRSM_GLOBAL="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_dense_cholesky as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"n"')]
    assert r.returncode == 0 and len(lines) == len(R.FROM_MEMORY_SIZES) and all('"bad": {}' in ln for ln in lines), \
        f"exit {r.returncode}\n" + "\n".join(lines) + "\n" + r.stderr[-3000:]
