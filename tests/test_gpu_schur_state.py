"""ITERATIVE_SCHUR on fresh handles against the numpy restatement (tests/schur_dense_reference.py), not against the oracle, so that a
failure names the device.  Aimed at state a handle did not write: before every case a larger problem with values a thousand times as
big runs on a handle of its own and is closed, so that the allocator hands its memory to the case; every operator, the three
preconditioners, fixed-count solves and one LM step are then checked on new handles.  The same checks run again in child interpreters
with CERES_HIP_DEBUG_POISON=nan and =big (every new floating-point buffer filled), together with the parity campaign's seeds 0 .. 19.

The cases: fuzz case 17 (the campaign's one unexplained failure), one point with a track of 63, 64, 65 or 128 observations among short
ones on 500 cameras that are mostly unobserved (<2,4,6> and <2,3,9>), 2300 cameras 9 wide (not in LDS: the camera-major pass and the
global accumulators) and camera-only prior rows."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_dense_reference as R
from step_check import assert_lm_style_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_TOL = 1e-12
SOLVE_TOL = 1e-10
STEP_TOL = 1e-9
PRECONDITIONERS = (R.SCHUR_JACOBI, R.JACOBI, R.SCHUR_POWER_SERIES_EXPANSION)


def make(hip, p, pre, min_it=0, max_it=50):
    s = hip.HipLinearSolver(hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=pre, min_num_iterations=min_it,
                                                    max_num_iterations=max_it, elimination_groups=[p.num_eliminate_blocks]))
    s.set_structure(p.bs)
    return s


@functools.lru_cache(maxsize=1)
def _dirty_problem(P):
    d = P.synthetic_bal(None, layout="schur", num_cameras=2600, num_points=12000, num_observations=60000, seed=77)
    d.values = d.values * 1e3
    d.b = d.b * 1e3
    return d


def dirty_allocator(hip, P):
    """A larger problem, values scaled by 1e3, through the Schur operators and a short solve on a handle that is then closed."""
    d = _dirty_problem(P)
    s = make(hip, d, hip.SCHUR_JACOBI, 3, 3)
    s.load(d.values, d.b, d.D)
    s.schur_init()
    s.schur_jacobi_update()
    s.schur_sx(np.ones(d.bs.num_cols - d.bs.col_block_pos[d.num_eliminate_blocks]))
    s.solve(d.values, d.b, hip.PerSolveOptions(D=d.D, q_tolerance=-1.0, r_tolerance=-1.0))
    s.close()


def upper(blocks_flat, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(np.triu(blocks_flat[o:o + n * n].reshape(n, n)).reshape(-1))
        o += n * n
    return np.concatenate(out)


def check_case(hip, P, name, dirty=True):
    """Every quantity of a fresh handle against the reference; returns {quantity: relative error} (NaN where the device gave NaN)."""
    p = R.build_case(P, name)
    ref = R.SchurReference(p)
    errs = {}
    rng = np.random.default_rng(11)
    xf, y0 = rng.standard_normal(ref.nf), rng.standard_normal(ref.nf)
    sizes = ref.f_sizes

    def err(key, got, want):
        errs[key] = R.rel(got, want) if np.isfinite(got).all() else float("nan")

    # ---- operators (SCHUR_JACOBI handle)
    if dirty:
        dirty_allocator(hip, P)
    s = make(hip, p, hip.SCHUR_JACOBI)
    if name.startswith("cameras2300"):
        assert s.info().camera_accum_in_lds == 0, "the 2300-camera case must leave the camera accumulators out of LDS"
    s.load(p.values, p.b, p.D)
    s.schur_init()
    err("schur_rhs", s.schur_rhs(), ref.rhs())
    err("ete_inverse", s.ete_inverse(), ref.ete_inverse())
    err("sx", s.schur_sx(xf), ref.sx(xf))
    err("back_substitute", s.back_substitute(xf), ref.back_substitute(xf))
    s.schur_jacobi_update()
    err("schur_jacobi_raw", upper(s.preconditioner_blocks(not_inverted=True), sizes), upper(R.SchurReference.flat(ref.schur_jacobi_raw()), sizes))
    s.schur_jacobi_update()
    err("schur_jacobi_inv", s.preconditioner_blocks(), R.SchurReference.flat(ref.schur_jacobi_inv()))
    s.close()
    # ---- JACOBI: blockdiag(F^T F + D_f^2)^-1
    if dirty:
        dirty_allocator(hip, P)
    s = make(hip, p, hip.JACOBI)
    s.load(p.values, p.b, p.D)
    s.block_jacobi_update()
    err("ftf_jacobi_inv", s.preconditioner_blocks(), R.SchurReference.flat(ref.ftf_inv))
    s.close()
    # ---- SCHUR_POWER_SERIES_EXPANSION: the operator and the preconditioner's apply
    if dirty:
        dirty_allocator(hip, P)
    s = make(hip, p, hip.SCHUR_POWER_SERIES_EXPANSION)
    s.load(p.values, p.b, p.D)
    s.schur_init()
    err("power_series_operator", s.power_series_operator(xf, y0), ref.power_series_operator(xf, y0))
    err("spse_apply_5", s.spse_apply(xf, 5, 0.0), ref.spse_apply(xf, 5, 0.0))
    s.close()
    # ---- fixed-count solves
    for pre in PRECONDITIONERS:
        for k in (1, 2, 4, 8):
            if dirty:
                dirty_allocator(hip, P)
            s = make(hip, p, pre, k, k)
            x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=-1.0))
            s.close()
            xr, sr = ref.solve(pre, k, k)
            assert (summ.termination_type, summ.num_iterations) == (sr.termination_type, sr.num_iterations), (name, pre, k, summ, sr)
            err(f"solve:pre{pre}:k{k}", x, xr)
    # ---- one LM step (LevenbergMarquardtStrategy's solve: q_tolerance = eta, r_tolerance = -1), radius 1
    if dirty:
        dirty_allocator(hip, P)
    s = make(hip, p, hip.SCHUR_JACOBI, 0, 500)
    step, summ, mcc = s.lm_compute_step(p.values, p.b, 1.0, 0.1)
    s.close()
    ref_lm = ref.with_D(np.sqrt(np.clip(ref.squared_column_norm(), 1e-6, 1e32) / 1.0))
    assert np.isfinite(step).all(), (name, "lm step not finite", summ)

    def solve(lo, hi, q, r):
        return ref_lm.solve(R.SCHUR_JACOBI, lo, hi, q, r)
    xo, so = assert_lm_style_step(-step, summ, solve, 0.1, hip.SUCCESS, STEP_TOL)
    if so.num_iterations != summ.num_iterations:
        xo, _ = solve(summ.num_iterations, summ.num_iterations, -1.0, -1.0)
    want = ref_lm.model_cost_change(-xo)
    errs["lm_step:model_cost_change"] = abs(mcc - want) / abs(want) if np.isfinite(mcc) else float("nan")
    return errs


def bad_of(errs):
    return {k: v for k, v in errs.items() if not (v <= (STEP_TOL if k.startswith("lm_step") else SOLVE_TOL if k.startswith("solve") else OP_TOL))}


@pytest.mark.parametrize("name", R.case_names())
def test_fresh_handles_after_a_dirty_allocator(hip, problems, name):
    errs = check_case(hip, problems, name)
    bad = bad_of(errs)
    assert not bad, f"{name}: device against the dense reference: {bad}   (all: {errs})"


@pytest.mark.parametrize("name", [f"fuzz{R.FUZZ_SEED}", "track64_246", "cameras2300_239"])
def test_same_handle_repeated(hip, problems, name):
    """schur_sx and the power-series operator twenty times each on one handle, every result against the reference: a contribution
    dropped by a race would show in one of them.  (A bounded check, not a hunt.)"""
    p = R.build_case(problems, name)
    ref = R.SchurReference(p)
    rng = np.random.default_rng(5)
    s = make(hip, p, hip.SCHUR_POWER_SERIES_EXPANSION)
    s.load(p.values, p.b, p.D)
    s.schur_init()
    for i in range(20):
        xf, y0 = rng.standard_normal(ref.nf), rng.standard_normal(ref.nf)
        e1 = R.rel(s.schur_sx(xf), ref.sx(xf))
        e2 = R.rel(s.power_series_operator(xf, y0), ref.power_series_operator(xf, y0))
        assert e1 <= OP_TOL and e2 <= OP_TOL, (name, i, e1, e2)
    s.close()


def _load_fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def child_main():
    """Runs in the child interpreter (CERES_HIP_DEBUG_POISON set): every case, then the campaign's seeds 0 .. 19; one JSON line each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library, as tools/fuzz_parity.py loads it)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    hip = pkg.hip_solver
    hip.load_library()
    failed = 0
    for name in R.case_names():
        try:
            bad = bad_of(check_case(hip, pkg.problems, name, dirty=False))
        except AssertionError as ex:
            bad = {"assertion": repr(ex)[:400]}
        failed += bool(bad)
        print(json.dumps({"case": name, "bad": bad}), flush=True)
    fuzz = _load_fuzz()
    for seed in range(20):
        try:
            bad = fuzz.run_case(seed)["bad"]
        except AssertionError as ex:
            bad = {"assertion": repr(ex)[:400]}
        failed += bool(bad)
        print(json.dumps({"fuzz_seed": seed, "bad": bad}), flush=True)
    return 1 if failed else 0


@pytest.mark.parametrize("pattern", ["nan", "big"])
def test_poisoned_allocations(hip, pattern):
    """CERES_HIP_DEBUG_POISON in a fresh child interpreter: a read of a value nothing wrote becomes NaN (nan) or a 1e16-sized error
    (big) in some result.  A signal or a time-out is a failure to investigate, not to rerun."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON=pattern)
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_schur_state as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    failures = [ln for ln in lines if '"bad": {}' not in ln]
    assert f"CERES_HIP_DEBUG_POISON={pattern}: new floating-point device buffers are filled" in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and len(lines) == len(R.case_names()) + 20, \
        f"CERES_HIP_DEBUG_POISON={pattern}: exit {r.returncode}\n" + "\n".join(failures) + "\n" + r.stderr[-3000:]
