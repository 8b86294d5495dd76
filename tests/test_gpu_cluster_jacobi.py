"""ITERATIVE_SCHUR + CLUSTER_JACOBI through the C ABI against the numpy restatement (tests/visibility_reference.py on top of
tests/schur_dense_reference.py): the preconditioner's application, fixed-count and converged solves, the LM step, identities, the
failure path, the retry and the BAL front end.  The clustering itself is held to the restatement on the CPU
(tests/test_visibility_clustering_cpu.py); here the membership comes from the same host analysis (ceres_hip_debug_cluster_cameras) and the
restatement builds M from it.

Apply parity is judged by the backward error |M z - x| / |x| (independent of the clusters' conditioning).  Its bound is computed, not
chosen: the same quantity for numpy's own Cholesky solve of the same M, times 10 (another summation order, a blocked factor), floored at
the OP_TOL of tests/test_gpu_schur_state.py.  The worst measured ratio device / numpy is recorded in design/14_cluster_jacobi.md."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_reference as F
import schur_dense_reference as R
import visibility_reference as V
from step_check import assert_lm_style_step
from test_gpu_schur_state import OP_TOL, SOLVE_TOL, STEP_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER_JACOBI = 4
TYPES = {"canonical_views": V.CANONICAL_VIEWS, "single_linkage": V.SINGLE_LINKAGE}


def make(hip, p, ctype=V.CANONICAL_VIEWS, min_it=0, max_it=500, pre=CLUSTER_JACOBI, generic=False, **kw):
    s = hip.HipLinearSolver(hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=pre, min_num_iterations=min_it,
                                                    max_num_iterations=max_it, elimination_groups=[p.num_eliminate_blocks],
                                                    visibility_clustering_type=ctype, force_generic_path=generic), **kw)
    s.set_structure(p.bs)
    return s


def all_see_all(P, n_cams=20, n_points=150, seed=2):
    """Every camera sees every point: every edge weighs 1, one cluster under either clustering."""
    rng = np.random.default_rng(seed)
    po = np.repeat(np.arange(n_points, dtype=np.int64), n_cams)
    co = np.tile(np.arange(n_cams, dtype=np.int64), n_points)
    p = P._assemble_bal(rng, n_cams, n_points, po, co, "schur", True)
    ref = R.SchurReference(p)
    p.D = np.sqrt(ref.squared_column_norm() * 1e-4)
    return p


def grouped(P):
    import test_visibility_clustering_cpu as C
    p = C.grouped_bal(n_points=1500)
    rng = np.random.default_rng(8)
    p.values = rng.standard_normal(p.bs.values_extent())
    p.b = rng.standard_normal(p.bs.num_rows)
    p.D = np.sqrt(R.SchurReference(p).squared_column_norm() * 1e-4)
    return p


# name -> (builder(P), force_generic_path)
CASES = {
    "banded_239": (lambda P: P.banded_bal(shape=None, num_cameras=120, num_points=2000, num_observations=9000), False),
    "track64_246": (lambda P: R.build_case(P, "track64_246"), False),
    "generic_random_schur": (lambda P: P.random_schur_problem(num_e_blocks=60, num_f_blocks=14, seed=5), True),
    "generic_banded": (lambda P: P.banded_bal(shape=None, num_cameras=40, num_points=500, num_observations=2400), True),
    "libmv_strip": (lambda P: P.libmv_structured(problem=2), False),
    "prior_rows_with_pairs": (lambda P: P.add_camera_rows(P.banded_bal(shape=None, num_cameras=60, num_points=900, num_observations=4000), 50,
                                                          seed=4, pair_fraction=0.4), False),
    "cameras2300_239": (lambda P: R.build_case(P, "cameras2300_239"), False),
    "grouped": (grouped, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    import conftest
    P = conftest.pkg.problems
    build, generic = CASES[name]
    p = build(P)
    return p, R.SchurReference(p), generic


def membership_of(hip, p, ctype):
    m, n = hip.debug_cluster_cameras(p.bs, int(p.num_eliminate_blocks), ctype)
    return np.array(m), n


def backward_error(M, z, x):
    return float(np.linalg.norm(M.apply_M(z) - x) / np.linalg.norm(x))


# ---- apply parity ---------------------------------------------------------------------------------------------------------------------
# (the libmv strip under single linkage is two clusters, 2642 and 6 scalars: the restatement alone takes most of a minute there — left out)
APPLY_CASES = [(n, c) for n in sorted(CASES) for c in sorted(TYPES) if (n, c) != ("libmv_strip", "single_linkage")]


@pytest.mark.parametrize("name,ctype", APPLY_CASES)
def test_apply_parity(hip, name, ctype):
    p, ref, generic = case(name)
    ct = TYPES[ctype]
    mem, n_clusters = membership_of(hip, p, ct)
    M = V.cluster_jacobi(ref, mem)
    s = make(hip, p, ct, generic=generic)
    info = s.info()
    assert info.kernel_path == (hip.PATH_GENERIC if generic else hip.PATH_BAL), (name, info.kernel_path)
    if name == "cameras2300_239":
        assert info.camera_accum_in_lds == 0
    s.load(p.values, p.b, p.D)
    s.cluster_jacobi_update()
    nc, largest, nbytes, seconds = s.cluster_jacobi_stats()
    dims = np.array([ii.shape[0] for ii, _ in M.clusters])
    assert nc == n_clusters == len(M.clusters) and largest == dims.max() and nbytes == 8 * int((dims.astype(np.int64) ** 2).sum())
    if name == "track64_246" and ctype == "single_linkage":   # a cluster above and clusters below the LDS-resident limit in one problem
        assert dims.max() > 128 and dims.min() <= 128, dims
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        x = rng.standard_normal(ref.nf)
        y0 = rng.standard_normal(ref.nf)
        z = s.precond_apply(x, y0.copy()) - y0      # the entry point accumulates: y += M^-1 x
        z_np = M(x)
        e_dev, e_np = backward_error(M, z, x), backward_error(M, z_np, x)
        bound = max(10.0 * e_np, OP_TOL)
        worst = max(worst, e_dev / max(e_np, 1e-300))
        print(f"apply parity {name} {ctype}: clusters {nc} largest {largest}  device {e_dev:.3e}  numpy {e_np:.3e}  ratio {e_dev / max(e_np, 1e-300):.2f}")
        assert np.isfinite(z).all() and e_dev <= bound, (name, ctype, e_dev, e_np, bound)
    s.close()


# ---- solves ---------------------------------------------------------------------------------------------------------------------------
def ref_solve(ref, M, lo, hi, q=-1.0, r=-1.0):
    z, summ = R.cg(ref.sx, ref.rhs(), M, lo, hi, q, r)
    return (None if summ.termination_type == R.FAILURE else ref.back_substitute(z)), summ


@pytest.mark.parametrize("name,ctype", [("banded_239", "canonical_views"), ("grouped", "single_linkage"), ("generic_banded", "canonical_views"),
                                        ("prior_rows_with_pairs", "canonical_views"), ("track64_246", "canonical_views")])
def test_fixed_iteration_parity(hip, name, ctype):
    p, ref, generic = case(name)
    ct = TYPES[ctype]
    M = V.cluster_jacobi(ref, membership_of(hip, p, ct)[0])
    for k in (1, 3, 10):
        s = make(hip, p, ct, k, k, generic=generic)
        x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=-1.0))
        s.close()
        xr, sr = ref_solve(ref, M, k, k)
        assert (summ.termination_type, summ.num_iterations) == (sr.termination_type, sr.num_iterations), (name, k, summ, sr)
        e = R.rel(x, xr)
        print(f"fixed iterations {name} {ctype} k={k}: {e:.3e}")
        assert e <= SOLVE_TOL, (name, k, e)


@pytest.mark.parametrize("name,ctype", [("banded_239", "canonical_views"), ("grouped", "single_linkage"), ("generic_banded", "canonical_views")])
def test_converged_solve_and_lm_step(hip, name, ctype):
    p, ref, generic = case(name)
    ct = TYPES[ctype]
    mem = membership_of(hip, p, ct)[0]
    M = V.cluster_jacobi(ref, mem)
    # converged by the residual test: the iteration count equals the restatement's +- 1
    s = make(hip, p, ct, 0, 500, generic=generic)
    x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=1e-8))
    xr, sr = ref_solve(ref, M, 0, 500, -1.0, 1e-8)
    assert summ.termination_type == sr.termination_type == hip.SUCCESS, (summ, sr)
    assert abs(summ.num_iterations - sr.num_iterations) <= 1, (summ, sr)
    assert R.rel(x, xr) <= 1e-6
    # the LM step: D = sqrt(clip(diag(J'J)) / radius), q_tolerance = eta
    step, summ, mcc = s.lm_compute_step(p.values, p.b, 1.0, 0.1)
    ref_lm = ref.with_D(np.sqrt(np.clip(ref.squared_column_norm(), 1e-6, 1e32) / 1.0))
    M_lm = V.cluster_jacobi(ref_lm, mem)
    assert np.isfinite(step).all(), summ
    xo, so = assert_lm_style_step(-step, summ, lambda lo, hi, q, r: ref_solve(ref_lm, M_lm, lo, hi, q, r), 0.1, hip.SUCCESS, STEP_TOL)
    if so.num_iterations != summ.num_iterations:
        xo, _ = ref_solve(ref_lm, M_lm, summ.num_iterations, summ.num_iterations)
    want = ref_lm.model_cost_change(-xo)
    assert abs(mcc - want) <= STEP_TOL * abs(want), (mcc, want)
    # the device entry points: the same solve and the same step from arrays resident in HBM
    import torch
    dev = torch.device("cuda:0")
    tv, tb, tD = (torch.from_numpy(np.ascontiguousarray(a_, dtype=np.float64)).to(dev) for a_ in (p.values, p.b, p.D))
    tx = torch.full((p.bs.num_cols,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    xh, sh = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=0.1, r_tolerance=-1.0))
    sd = s.solve_device(tv.data_ptr(), tb.data_ptr(), tD.data_ptr(), tx.data_ptr(), 0.1, -1.0)
    assert (sd.termination_type, sd.num_iterations) == (sh.termination_type, sh.num_iterations)
    assert R.rel(tx.cpu().numpy(), xh) <= 1e-13
    sd, mcc_d, finite = s.lm_compute_step_device(tv.data_ptr(), tb.data_ptr(), tx.data_ptr(), 1.0, 0.1)
    assert finite and sd.num_iterations == summ.num_iterations and R.rel(tx.cpu().numpy(), step) <= 1e-13 and abs(mcc_d - mcc) <= 1e-12 * abs(mcc)
    s.close()


# ---- identities -----------------------------------------------------------------------------------------------------------------------
def test_only_singletons_is_schur_jacobi(hip, problems):
    p = problems.synthetic_bal(None, layout="schur", num_cameras=60, num_points=1500, num_observations=7000, seed=3)
    mem, n = membership_of(hip, p, V.SINGLE_LINKAGE)
    assert n == 60, n
    out = {}
    for pre in (CLUSTER_JACOBI, hip.SCHUR_JACOBI):
        s = make(hip, p, V.SINGLE_LINKAGE, 0, 500, pre=pre)
        assert s.info().kernel_path == hip.PATH_BAL
        out[pre] = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=1e-10))
        s.close()
    (xa, sa), (xb, sb) = out[CLUSTER_JACOBI], out[hip.SCHUR_JACOBI]
    assert sa.termination_type == sb.termination_type == hip.SUCCESS
    assert sa.num_iterations == sb.num_iterations, (sa, sb)
    assert R.rel(xa, xb) <= SOLVE_TOL


@pytest.mark.parametrize("ctype", sorted(TYPES))
def test_one_cluster_is_the_schur_complement(hip, problems, ctype):
    p = all_see_all(problems)
    ref = R.SchurReference(p)
    mem, n = membership_of(hip, p, TYPES[ctype])
    assert n == 1 and (mem == 0).all()
    s = make(hip, p, TYPES[ctype], 0, 50)
    assert s.info().kernel_path == hip.PATH_BAL
    x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=1e-10))
    s.close()
    assert summ.termination_type == hip.SUCCESS and summ.num_iterations <= 2, summ
    exact = ref.back_substitute(np.linalg.solve(ref.dense_S(), ref.rhs()))
    assert R.rel(x, exact) <= 1e-9, R.rel(x, exact)


def run_twice_numbers(hip, name, ctype=V.CANONICAL_VIEWS):
    p, _, generic = case(name)
    out = []
    for _ in range(2):
        s = make(hip, p, ctype, 7, 7, generic=generic)
        x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=-1.0))
        step, _, mcc = s.lm_compute_step(p.values, p.b, 10.0, 0.1)
        s.close()
        out.append((x, step, mcc, summ.num_iterations))
    return out


# The fused kernels' S x sums a camera's observations with LDS atomics: two runs of ANY fused ITERATIVE_SCHUR solve differ at rounding
# level (tests/test_gpu_solvers.py::test_summary_edge_cases allows 1e-13 for it).  The generic kernels use no atomics, and nothing this
# preconditioner adds does (gather elimination, one writer per matrix entry, fixed summation orders): there the results repeat bit
# for bit, on the fused path to that test's 1e-13.
FUSED_REPEAT_TOL = 1e-13


def same_numbers(a, b, exact):
    if exact:
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    return R.rel(a[0], b[0]) <= FUSED_REPEAT_TOL and R.rel(a[1], b[1]) <= FUSED_REPEAT_TOL and abs(a[2] - b[2]) <= FUSED_REPEAT_TOL * abs(b[2]) and a[3] == b[3]


@pytest.mark.parametrize("name", ["generic_banded", "banded_239"])
def test_two_runs_repeat(hip, name):
    a, b = run_twice_numbers(hip, name)
    assert same_numbers(a, b, exact=case(name)[2]), name


def child_main():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    import __graft_entry__ as entry
    hip = entry.load_package().hip_solver
    hip.load_library()
    for name in ("generic_banded", "banded_239"):
        a, _ = run_twice_numbers(hip, name)
        print(json.dumps({"name": name, "x": a[0].tolist(), "step": a[1].tolist(), "mcc": a[2], "its": a[3]}), flush=True)
    return 0


def test_poisoned_allocations_give_the_same_numbers(hip):
    """CERES_HIP_DEBUG_POISON=nan in a child interpreter: every new floating-point buffer filled with NaN; the numbers of a solve and an
    LM step equal the unpoisoned run's (generic path: bit for bit)."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_cluster_jacobi as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [g["name"] for g in lines] == ["generic_banded", "banded_239"]
    for g in lines:
        a, _ = run_twice_numbers(hip, g["name"])
        got = (np.array(g["x"]), np.array(g["step"]), g["mcc"], g["its"])
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert same_numbers(got, a, exact=case(g["name"])[2]), g["name"]


# ---- failure path, retry ------------------------------------------------------------------------------------------------------------
def test_reports_factorization_failure_and_stays_usable(hip, problems):
    # a cluster matrix that is singular: one camera with an all-zero Jacobian and no regularisation
    p = problems.synthetic_bal(None, layout="schur", num_cameras=9, num_points=200, num_observations=900, seed=5)
    cam0 = int(p.camera_of_row.min())
    rows = np.nonzero(p.camera_of_row == cam0)[0]
    fpos = p.bs.cell_value_pos[1::2][rows].astype(np.int64)
    vals = p.values.copy()
    vals[(fpos[:, None] + np.arange(18)[None, :]).reshape(-1)] = 0.0
    for ctype in TYPES.values():
        s = make(hip, p, ctype, 0, 50)
        x, summ = s.solve(vals, p.b, hip.PerSolveOptions(D=None))
        assert summ.termination_type == hip.FAILURE and summ.message == "Preconditioner update failed.", summ
        x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=1e-8))   # the instance stays usable
        assert summ.termination_type == hip.SUCCESS, summ
        s.close()


def test_retry_with_a_changed_radius_refactors(hip):
    p, _, generic = case("banded_239")
    s = make(hip, p, V.CANONICAL_VIEWS, 0, 500)
    s.lm_compute_step(p.values, p.b, 100.0, 0.1)
    step, summ, mcc = s.lm_compute_step(None, None, 1.0, 0.1, reuse_diagonal=True, values_unchanged=True)
    s.close()
    f = make(hip, p, V.CANONICAL_VIEWS, 0, 500)
    step_f, summ_f, mcc_f = f.lm_compute_step(p.values, p.b, 1.0, 0.1)
    f.close()
    assert summ.termination_type == summ_f.termination_type == hip.SUCCESS
    assert summ.num_iterations == summ_f.num_iterations, (summ, summ_f)
    assert R.rel(step, step_f) <= STEP_TOL and abs(mcc - mcc_f) <= STEP_TOL * abs(mcc_f)


def test_wrong_handle_and_sharded_handle(hip):
    p, _, _ = case("generic_banded")
    s = make(hip, p, pre=hip.SCHUR_JACOBI)
    s.load(p.values, p.b, p.D)
    with pytest.raises(hip.HipError, match="CLUSTER_JACOBI"):
        s.cluster_jacobi_update()
    with pytest.raises(hip.HipError):
        s.cluster_jacobi_stats()
    s.close()
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=CLUSTER_JACOBI, max_num_iterations=5,
                                elimination_groups=[p.num_eliminate_blocks])
    s = hip.HipLinearSolver(o, loopback_world=2)
    rc = s._lib.ceres_hip_set_structure(s._h, p.bs.as_ctypes())
    assert rc == hip.E_UNSUPPORTED and b"CLUSTER_JACOBI" in s._lib.ceres_hip_last_error(s._h)
    s.close()


# ---- the BAL front end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def banded_scene():
    import conftest
    return conftest.pkg.problems.bal_scene(shape=None, seed=11, num_cameras=30, num_points=300, num_observations=1500, visibility="banded")


@pytest.mark.parametrize("camera,loss,ctype", [("angle_axis", "none", "canonical_views"), ("angle_axis", "none", "single_linkage"),
                                               ("angle_axis", "huber", "canonical_views"), ("quaternion_manifold", "none", "single_linkage")])
def test_front_end_follows_the_composed_reference(hip, oracle, camera, loss, ctype):
    """BalProblem.minimize with ITERATIVE_SCHUR + CLUSTER_JACOBI against frontend_reference.minimize, with the checks, tolerances, eta
    and iteration limits tests/test_gpu_frontend_matrix.py applies to its ITERATIVE_SCHUR + LM cases (loop_deviations, limits)."""
    import test_gpu_frontend_matrix as FM
    sc = banded_scene()
    nc, npts, cam, pt, obs, par = sc
    fm_case = (camera, loss, 1.0, "lm", (5, 2), 0, None, 1, None, None)   # (the solver entry selects the ITERATIVE_SCHUR tolerances)
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=CLUSTER_JACOBI, min_num_iterations=0, max_num_iterations=10000,
                                visibility_clustering_type=TYPES[ctype])
    gp = hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=camera)
    try:
        assert gp.solver_info().kernel_path == hip.PATH_BAL
        lp = None if loss == "none" else (loss,) + FM.LOSS_PARAMS[loss] + (1.0,)
        if lp:
            gp.set_loss(*lp)
        ev = F.problem(oracle.snavely_batch, FM.MODELS[camera], nc, npts, cam, pt, obs, gp.row_order(), lp)
        x0 = gp.state_from_bal(par)
        dev = FM.loop_deviations(gp, ev, x0, fm_case, None, npts, 8)
    finally:
        gp.close()
    lim = {k: v for k, v in FM.limits(fm_case).items() if k in dev}
    print(f"front end {camera} {loss} {ctype}: {dev}")
    assert not FM.exceeded(dev, lim), (FM.exceeded(dev, lim), dev)
