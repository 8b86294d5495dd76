"""The size-selected kernels of the fused path on small scenes (design/19_dispatch_thresholds.md): the software-pipelined streaming
kernels and the 1024-thread variants (from kPipelineMinTilesPerWg tiles per workgroup), x staged in LDS (from kStagedXMinTilesPerWg)
and the lane-per-observation camera kernel (items of kCamItemLaneMinMean observations on average) — for every compiled shape, against
the oracle at the bounds of the small-problem tests.  Scenes of some 20 000 observations get there through the two per-handle
switches CERES_HIP_FUSED_GRID (fewer workgroups: more tiles each) and CERES_HIP_CAM_CHUNK_MIN (full-length camera items); every test
asserts on a live handle that the scene reaches the kernel it is meant for (tests/dispatch_cases.py restates the rule; the scenes'
preconditions are held on the CPU by tests/test_dispatch_cases_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_cases as D
from test_gpu_lm_step import check_step
from test_gpu_operators import assert_errs, check_cgnr_operators, check_schur_operators, make_solver, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every shape of common.h's compiled list (tests/test_dispatch_cases_cpu.py compares these with kernels_bal_common.hip's)
PIPELINED_SHAPES = ["f2_s0", "f3_s0", "f4_s0", "f5_s0", "f6_s0", "f7_s0", "f8_s0", "f9_s0", "f10_s0", "f6_s4", "f6_s8", "f9_s4", "f9_s8"]
OTHER_SHAPES = ["e2_f2_s0", "e2_f3_s0", "e2_f4_s0", "e2_f6_s0", "e2_f9_s0", "e4_f2_s0", "e4_f3_s0", "e4_f4_s0", "e4_f5_s0", "e4_f6_s0",
                "e4_f7_s0", "e4_f8_s0", "e4_f9_s0", "e4_f10_s0", "r3_e3_f3_s0", "r4_e4_f2_s0", "r4_e4_f3_s0", "r4_e4_f4_s0"]
ALL_SHAPES = PIPELINED_SHAPES + OTHER_SHAPES


def set_switches(setenv, delenv, grid_cap, chunk_min=None):
    for name, v in (("CERES_HIP_FUSED_GRID", grid_cap), ("CERES_HIP_CAM_CHUNK_MIN", chunk_min)):
        if v:
            setenv(name, str(v))
        else:
            delenv(name, raising=False)


def switches(monkeypatch, grid_cap, chunk_min=None):
    set_switches(monkeypatch.setenv, monkeypatch.delenv, grid_cap, chunk_min)


def assert_reaches(hip, p, name, grid_cap, kernel, staged, solver_type=None, chunk_min=None):
    """On a live handle built under the current switches: the fused path with every camera's sums in LDS, and by the restated rule the
    kernel and the staging the scene is meant for.  Returns the handle's tile count."""
    s = make_solver(hip, p, solver_type or hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI if solver_type is None else hip.JACOBI)
    info = s.info()
    s.close()
    assert info.kernel_path == hip.PATH_BAL and info.camera_accum_in_lds == 1, (info.kernel_path, info.camera_accum_in_lds)
    n_tiles = int(info.num_tiles)
    assert D.fused_kernel(n_tiles, grid_cap, name) == kernel, (n_tiles, grid_cap, D.fused_kernel(n_tiles, grid_cap, name))
    assert D.x_staged(n_tiles, grid_cap) == staged, (n_tiles, grid_cap)
    if solver_type is None:
        deg, planned = D.camera_degrees(hip, p)
        assert planned == n_tiles
        if chunk_min:
            assert D.camera_item_kernel(deg, len(p.bs.row_block_size), name, chunk_min) == "lane"
    return n_tiles


def big_kernel(name):
    return "pipelined" if D.pipelined(name) else "1024"


def lm_step_and_retry(hip, oracle, p):
    """One lm_compute_step and its values_unchanged retry: the model cost comes from back-substitution, with x in LDS."""
    s = make_solver(hip, p, hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI, max_it=500)
    radius = 1e4
    step, summ, mcc = s.lm_compute_step(p.values, p.b, radius, 0.1)
    diag = np.clip(oracle.Matrix(p.bs, 0).squared_column_norm(p.values), 1e-6, 1e32)
    assert rel(s.lm_diagonal(), np.sqrt(diag / radius)) <= 1e-13
    check_step(oracle, hip, p, hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI, np.sqrt(diag / radius), step, summ, mcc, 0.1)
    step, summ, mcc = s.lm_compute_step(None, None, radius / 2, 0.1, reuse_diagonal=True, values_unchanged=True)
    check_step(oracle, hip, p, hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI, np.sqrt(diag / (radius / 2)), step, summ, mcc, 0.1)
    s.close()


# ---- few cameras: 8 cameras, 319 tiles, items of 512 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_cap", D.FEW_GRID_CAPS)
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_schur_operators_on_few_cameras(hip, oracle, problems, monkeypatch, name, grid_cap):
    """S.x, rhs, back-substitution, SCHUR_JACOBI raw and inverted, JACOBI: the pipelined kernels (13 shapes) or the 1024-thread ones (18),
    every camera's x staged, full-length, ragged and short items in the lane-per-observation camera kernel."""
    switches(monkeypatch, grid_cap, D.CAM_CHUNK_MIN)
    p = D.few_cameras(problems, name)
    assert_reaches(hip, p, name, grid_cap, big_kernel(name), True, chunk_min=D.CAM_CHUNK_MIN)
    assert_errs(check_schur_operators(hip, oracle, p, False, hip.PATH_BAL))


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_lm_step_on_few_cameras(hip, oracle, problems, monkeypatch, name):
    switches(monkeypatch, 3, D.CAM_CHUNK_MIN)
    p = D.few_cameras(problems, name, seed=12)
    assert_reaches(hip, p, name, 3, big_kernel(name), True, chunk_min=D.CAM_CHUNK_MIN)
    lm_step_and_retry(hip, oracle, p)


@pytest.mark.parametrize("name", [n for n in PIPELINED_SHAPES if D.cgnr_fused(n)])
def test_cgnr_operators_on_few_cameras(hip, oracle, problems, monkeypatch, name):
    """JtJx on the pipelined kernel (CGNR reads a 3-wide camera or shared block as a point: those shapes run the generic kernels and
    are left to tests/test_gpu_shapes.py)."""
    switches(monkeypatch, 3, D.CAM_CHUNK_MIN)
    p = D.few_cameras(problems, name)
    q = type(p)(p.bs, p.values, p.b, p.D, 0)
    assert_reaches(hip, q, name, 3, "pipelined", True, solver_type=hip.CGNR)
    assert_errs(check_cgnr_operators(hip, oracle, p, False, hip.PATH_BAL))


# ---- cameras that fill LDS: eleven staged rows beside the accumulators -----------------------------------------------------------------
@pytest.mark.parametrize("name", PIPELINED_SHAPES)
def test_schur_operators_where_the_accumulators_fill_lds(hip, oracle, problems, monkeypatch, name):
    """Slots of staged and of unstaged cameras in the same tile.  schur_jacobi_raw is a max-norm over thousands of blocks of cameras
    with a handful of observations: 1e-11, as tests/test_gpu_shapes.py::test_narrow_cameras_beyond_lds and for its reason."""
    switches(monkeypatch, D.LDS_GRID_CAP)
    p = D.lds_filling(problems, name)
    assert_reaches(hip, p, name, D.LDS_GRID_CAP, "pipelined", True)
    errs = check_schur_operators(hip, oracle, p, False, hip.PATH_BAL)
    raw = errs.pop("schur_jacobi_raw")
    assert raw <= 1e-11, raw
    assert_errs(errs)


@pytest.mark.parametrize("name", PIPELINED_SHAPES)
def test_lm_step_and_cgnr_where_the_accumulators_fill_lds(hip, oracle, problems, monkeypatch, name):
    switches(monkeypatch, D.LDS_GRID_CAP)
    p = D.lds_filling(problems, name, seed=24)
    assert_reaches(hip, p, name, D.LDS_GRID_CAP, "pipelined", True)
    lm_step_and_retry(hip, oracle, p)
    if D.cgnr_fused(name):
        q = type(p)(p.bs, p.values, p.b, p.D, 0)
        assert_reaches(hip, q, name, D.LDS_GRID_CAP, "pipelined", True, solver_type=hip.CGNR)
        assert_errs(check_cgnr_operators(hip, oracle, p, False, hip.PATH_BAL))


# ---- the power-series operator (kSpseZ) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f9_s0", "f6_s0", "f6_s8", "e4_f6_s0"])
def test_power_series_operator_above_both_thresholds(hip, oracle, problems, monkeypatch, name):
    """kSpseZ pipelined with x staged (f9, f6, the libmv strip) and on the 1024-thread kernel (4-wide points), the pairs of
    tests/test_gpu_spse.py."""
    switches(monkeypatch, 1, D.CAM_CHUNK_MIN)
    p = D.few_cameras(problems, name, seed=13)
    assert_reaches(hip, p, name, 1, big_kernel(name), True)
    m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    isc = oracle.ImplicitSchurComplement(m)
    isc.init(p.values, p.D, p.b)
    isc.compute_ftf_inverse()
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=hip.SCHUR_POWER_SERIES_EXPANSION,
                                min_num_iterations=0, max_num_iterations=100, elimination_groups=[p.num_eliminate_blocks])
    s = hip.HipLinearSolver(o)
    s.set_structure(p.bs)
    info = s.info()
    assert info.kernel_path == hip.PATH_BAL and info.camera_accum_in_lds == 1
    assert D.fused_kernel(int(info.num_tiles), 1, name) == big_kernel(name) and D.x_staged(int(info.num_tiles), 1)
    s.load(p.values, p.b, p.D)
    s.schur_init()
    rng = np.random.default_rng(0)
    x, y0 = rng.standard_normal(m.num_cols_f), rng.standard_normal(m.num_cols_f)
    assert rel(s.power_series_operator(x, y0), isc.power_series_operator(x, y0)) <= 1e-12
    for iters, tol in ((1, 0.0), (5, 0.0), (8, 0.1), (50, 1e-3)):
        assert rel(s.spse_apply(x, iters, tol), isc.spse_apply(x, iters, tol)) <= 1e-11, (iters, tol)
    s.close()


# ---- solves: the CG loop around the pipelined operator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["few_cameras", "lds_filling"])
@pytest.mark.parametrize("name", ["f6_s0", "f8_s0", "f9_s8", "e4_f6_s0"])
def test_fixed_count_solves(hip, oracle, problems, monkeypatch, name, scene):
    """ITERATIVE_SCHUR + SCHUR_JACOBI at 1, 7 and 25 iterations (25 crosses two residual resets), 1e-9 as
    tests/test_gpu_shapes.py::test_solvers_of_every_shape: the CG loop around the pipelined (1024-thread: e4_f6) operator, every
    camera's x staged (few cameras) or eleven of thousands (LDS-filling).  (The S.x pass that finishes the CG iteration itself is f9's
    alone — kHasCgTail — and runs at full size.)"""
    if scene == "few_cameras":
        cap = 3
        switches(monkeypatch, cap, D.CAM_CHUNK_MIN)
        p = D.few_cameras(problems, name, seed=14)
    else:
        cap = D.LDS_GRID_CAP
        switches(monkeypatch, cap)
        p = D.lds_filling(problems, name, seed=25)
    assert_reaches(hip, p, name, cap, big_kernel(name), True)
    m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    for k in (1, 7, 25):
        s = make_solver(hip, p, hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI, min_it=k, max_it=k)
        x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=p.D, q_tolerance=-1.0, r_tolerance=0.0))
        s.close()
        xo, so = m.iterative_schur_solve(p.values, p.b, p.D, preconditioner=hip.SCHUR_JACOBI, min_it=k, max_it=k, q_tol=-1.0, r_tol=0.0)
        assert (summ.termination_type, summ.num_iterations) == (so.termination_type, so.num_iterations), (summ, so)
        assert rel(x, xo) <= 1e-9, (k, rel(x, xo))


# ---- both sides of each threshold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tiles", D.boundary_tiles())
def test_both_sides_of_each_threshold(hip, oracle, problems, monkeypatch, n_tiles):
    """One workgroup over exactly 39, 40, 99 and 100 tiles."""
    k = D.constants()
    name, cap = D.BOUNDARY_SHAPE, D.BOUNDARY_GRID_CAP
    switches(monkeypatch, cap)
    p = D.boundary(hip, problems, n_tiles)
    kernel = "pipelined" if n_tiles >= k["kPipelineMinTilesPerWg"] else "512"
    assert assert_reaches(hip, p, name, cap, kernel, n_tiles >= k["kStagedXMinTilesPerWg"]) == n_tiles
    assert_errs(check_schur_operators(hip, oracle, p, False, hip.PATH_BAL))
    assert_errs(check_cgnr_operators(hip, oracle, p, False, hip.PATH_BAL))
    lm_step_and_retry(hip, oracle, p)


# ---- points of more than 64 observations: cooperative rounds inside the pipelined kernel -----------------------------------------------------
@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("name", list(D.LONG_POINT_SHAPES))
def test_long_points_in_the_pipelined_kernels(hip, oracle, problems, monkeypatch, name, staged):
    p = D.long_points(problems, name)
    _, n_tiles = D.camera_degrees(hip, p)
    cap = D.LONG_POINTS_STAGED_CAP if staged else D.long_points_grid_cap(n_tiles)
    switches(monkeypatch, cap)
    assert_reaches(hip, p, name, cap, "pipelined", staged)
    assert_errs(check_schur_operators(hip, oracle, p, False, hip.PATH_BAL))
    if D.cgnr_fused(name):
        assert_errs(check_cgnr_operators(hip, oracle, p, False, hip.PATH_BAL))


# ---- a cap changes how the work is spread, not what is computed --------------------------------------------------------------------------------
def test_grid_caps_agree_with_each_other(hip, problems, monkeypatch):
    name = "f5_s0"
    p = D.few_cameras(problems, name, seed=15)
    xf = np.random.default_rng(4).standard_normal(D.FEW_CAMERAS * 5)
    got = {}
    for cap in (1, 3, None):
        switches(monkeypatch, cap, D.CAM_CHUNK_MIN)
        assert_reaches(hip, p, name, cap, "pipelined" if cap else "512", bool(cap))
        s = make_solver(hip, p, hip.ITERATIVE_SCHUR, hip.SCHUR_JACOBI)
        s.load(p.values, p.b, p.D)
        s.schur_init()
        r = dict(rhs=s.schur_rhs(), sx=s.schur_sx(xf), back_substitute=s.back_substitute(xf))
        s.schur_jacobi_update()
        r["schur_jacobi_raw"] = s.preconditioner_blocks(not_inverted=True)
        s.close()
        got[cap] = r
    for a, b in ((1, 3), (1, None), (3, None)):   # (sums re-associate: never bit for bit)
        assert_errs({f"{key} cap {a} vs {b}": rel(got[a][key], got[b][key]) for key in got[a]})


# ---- poisoned allocations ---------------------------------------------------------------------------------------------------------------------
POISON_SHAPE = "f7_s0"


def child_main():
    """In the child interpreter (CERES_HIP_DEBUG_POISON=nan): the few-cameras and the LDS-filling scene of one shape; one JSON line each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library, as tests/test_gpu_schur_state.py loads it)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hip = pkg.hip_solver
    hip.load_library()
    failed = 0
    for scene, cap, chunk_min in (("few_cameras", 3, D.CAM_CHUNK_MIN), ("lds_filling", D.LDS_GRID_CAP, None)):
        set_switches(os.environ.__setitem__, lambda k, raising=False: os.environ.pop(k, None), cap, chunk_min)
        p = getattr(D, scene)(pkg.problems, POISON_SHAPE)
        try:
            assert_reaches(hip, p, POISON_SHAPE, cap, "pipelined", True)
            errs = check_schur_operators(hip, oracle, p, False, hip.PATH_BAL)
            errs.update(check_cgnr_operators(hip, oracle, p, False, hip.PATH_BAL))
            lm_step_and_retry(hip, oracle, p)
            bad = {k: v for k, v in errs.items() if not v <= (1e-11 if k == "schur_jacobi_raw" else 1e-12)}
        except AssertionError as ex:
            bad = {"assertion": repr(ex)[:400]}
        failed += bool(bad)
        print(json.dumps({"scene": scene, "bad": bad}), flush=True)
    return 1 if failed else 0


def test_poisoned_allocations_above_the_thresholds(hip):
    """Every new floating-point device buffer filled with NaN, in a fresh child interpreter: a staged row of x or a partial sum that
    nothing wrote shows in some result.  A signal or a time-out is a failure to investigate, not to rerun."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_dispatch as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and len(lines) == 2 and all('"bad": {}' in ln for ln in lines), \
        f"exit {r.returncode}\n" + "\n".join(lines) + "\n" + r.stderr[-3000:]
