"""The point tail of short ITERATIVE_SCHUR solves (design/20_point_tail.md): with at most kPointTailMaxIterations CG iterations from
x = 0 the point part of the solution and the LM step's model cost come from the per-point sums E^T F p the S.x passes keep, not from a
pass over J.  Every case runs with the switch on (CERES_HIP_POINT_TAIL, read per handle at set_structure), asserts the route the
handle reports, and holds the step and the model cost to the oracle (1e-9, the rule of tests/test_gpu_lm_step.py::check_step) and to a
handle with the switch off.

On versus off: the two routes round differently (a few 1e-13 expected).  The bound is ten times what two switch-off handles differ by
among themselves on the scene (their LDS sums add in arrival order), or 1e-11, whichever is larger.  The measured figures go, one entry
per comparison, into the JSON array of the file CERES_HIP_POINT_TAIL_REPORT names: profiles/point_tail_on_off.json is that file of a run
of this module alone (CERES_HIP_POINT_TAIL_REPORT=profiles/point_tail_on_off.json, the file absent before)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_cases as D
from test_gpu_lm_step import check_step
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = D.constants()["kPointTailMaxIterations"]
SCHUR, SCHUR_JACOBI = 5, 2
RADIUS, ETA = 1e4, 0.1


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def cameras_scene(problems, n_cams, seed=71):
    """About 9 000 observations in some 150 tiles.  40 cameras: 360 camera scalars, the S.x pass finishes the CG iteration itself
    (kCgTailMax = 512); 80 cameras: the separate CG kernels."""
    return problems.synthetic_bal(None, layout="schur", num_cameras=n_cams, num_points=2000, num_observations=9000, seed=seed, skew=0.5)


LONG_TRACKS = [600] + [129] * 4 + [65] * 20 + [64] * 20 + [63] * 20 + [1] * 30 + [2] * 30 + [200] * 30 + [100] * 60


def long_scene(problems, seed=73):
    """700 cameras, 215 points, 17 046 observations: tracks of 1, 2, 63 and 64 (normal tiles), 65, 100 and 129 (two and three tiles: packed
    rounds), 200 (four) and one of 600 (ten tiles: sum rounds and apply rounds of its own)."""
    rng = np.random.default_rng(seed)
    tracks = np.asarray(LONG_TRACKS)[rng.permutation(len(LONG_TRACKS))]
    pt = np.repeat(np.arange(len(tracks), dtype=np.int64), tracks)
    cam = np.concatenate([np.sort(rng.choice(700, size=int(n), replace=False)) for n in tracks]).astype(np.int64)
    return problems.structured_bal(700, len(tracks), pt, cam, seed=seed)


def pipelined_cap(hip, p):
    """The largest CERES_HIP_FUSED_GRID that leaves kPipelineMinTilesPerWg tiles per workgroup: the pipelined streaming kernel."""
    return D.long_points_grid_cap(int(hip.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)["n_tiles"]))


# ---- handles, references, report ------------------------------------------------------------------------------------------------------
def handle(hip, monkeypatch, p, switch, grid_cap=None, speculate=None, max_it=500, min_it=0, **opts):
    monkeypatch.setenv("CERES_HIP_POINT_TAIL", "1" if switch else "0")
    for name, v in (("CERES_HIP_FUSED_GRID", grid_cap), ("CERES_HIP_SPECULATE", speculate)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    o = hip.LinearSolverOptions(type=SCHUR, preconditioner_type=SCHUR_JACOBI, min_num_iterations=min_it, max_num_iterations=max_it,
                                elimination_groups=[p.num_eliminate_blocks], **opts)
    s = hip.HipLinearSolver(o)
    s.set_structure(p.bs)
    return s


def lm_diag(oracle, p, radius):
    return np.sqrt(np.clip(oracle.Matrix(p.bs, 0).squared_column_norm(p.values), 1e-6, 1e32) / radius)


def model_cost(oracle, p, x):
    m = oracle.Matrix(p.bs, 0).right_multiply(p.values, -x)
    return -m @ (p.b + m / 2.0)


def check_fixed_count(oracle, hip, p, Dv, step, summ, mcc, tol=1e-9):
    """check_step's rule for a solve whose count the options fix: the step is the negated oracle iterate of that count, the model
    cost change the one of that iterate."""
    m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    k = summ.num_iterations
    xo, so = m.iterative_schur_solve(p.values, p.b, Dv, preconditioner=SCHUR_JACOBI, min_it=k, max_it=k, q_tol=-1.0, r_tol=-1.0)
    assert so.num_iterations == k and np.isfinite(step).all()
    assert rel(-step, xo) <= tol, rel(-step, xo)
    want = model_cost(oracle, p, xo)
    assert abs(mcc - want) <= tol * abs(want), (mcc, want)


def report(case, **figures):
    print(json.dumps(dict(case=case, **figures)), flush=True)
    path = os.environ.get("CERES_HIP_POINT_TAIL_REPORT")
    if path:   # one JSON array, rewritten with this entry behind the file's (profiles/point_tail_on_off.json is such a file, as written)
        rows = json.load(open(path)) if os.path.exists(path) else []
        with open(path, "w") as f:
            json.dump(rows + [dict(case=case, **figures)], f, indent=1)


def compare(case, on, off_a, off_b):
    """on / off_a / off_b: (step, summary, model cost change) of the switch-on handle and of two switch-off handles."""
    for r in (off_a, off_b):
        assert r[1].num_iterations == on[1].num_iterations and r[1].termination_type == on[1].termination_type, (on[1], r[1])
    spread_step, spread_mcc = rel(off_a[0], off_b[0]), abs(off_a[2] - off_b[2]) / abs(off_b[2])
    d_step, d_mcc = rel(on[0], off_a[0]), abs(on[2] - off_a[2]) / abs(off_a[2])
    bound_step, bound_mcc = max(10 * spread_step, 1e-11), max(10 * spread_mcc, 1e-11)
    report(case, iterations=on[1].num_iterations, off_off_step=spread_step, off_off_mcc=spread_mcc, on_off_step=d_step, on_off_mcc=d_mcc,
           bound_step=bound_step, bound_mcc=bound_mcc)
    assert d_step <= bound_step and d_mcc <= bound_mcc, (case, d_step, bound_step, d_mcc, bound_mcc)


def lm_three(hip, monkeypatch, p, radius=RADIUS, eta=ETA, **kw):
    """One lm_compute_step on a switch-on handle and on two switch-off handles; the on handle stays open (first of the return)."""
    on = handle(hip, monkeypatch, p, True, **kw)
    res_on = on.lm_compute_step(p.values, p.b, radius, eta)
    route = on.last_backsub_route()
    offs = []
    for _ in range(2):
        off = handle(hip, monkeypatch, p, False, **kw)
        offs.append(off.lm_compute_step(p.values, p.b, radius, eta))
        assert off.last_backsub_route() == 0
        off.close()
    return on, route, res_on, offs


# ---- camera-space size and kernel variant -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cams,pipelined", [(40, False), (40, True), (80, False), (80, True)])
def test_natural_stop_by_camera_space_and_kernel(hip, oracle, problems, monkeypatch, n_cams, pipelined):
    """eta = 0.1 ends CG after a few iterations.  40 cameras: the in-operator CG tail (always the pipelined kernel; the cap only changes
    its grid); 80 cameras: cg_update_kernel, on the 512-thread kernel and, with the grid narrowed, the pipelined one."""
    p = cameras_scene(problems, n_cams)
    cap = pipelined_cap(hip, p) if pipelined else None
    n_tiles = int(hip.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)["n_tiles"])
    assert D.fused_kernel(n_tiles, cap, "f9_s0") == ("pipelined" if pipelined else "512")
    on, route, res, offs = lm_three(hip, monkeypatch, p, grid_cap=cap)
    assert on.info().kernel_path == hip.PATH_BAL and on.info().camera_accum_in_lds == 1
    assert 1 <= res[1].num_iterations <= K and route == 1, (res[1], route)
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), res[0], res[1], res[2], ETA)
    compare(f"natural_{n_cams}_{'pipelined' if pipelined else '512'}", res, *offs)
    on.close()


@pytest.mark.parametrize("n_cams", [40, 80])
@pytest.mark.parametrize("count", ["1", "K", "K+1", "max_K"])
def test_iteration_counts(hip, oracle, problems, monkeypatch, n_cams, count):
    """min = max = 1, K and K + 1 iterations, and max = K reached without convergence (eta = 1e-12).  K + 1 is past the buffers: the pass
    over J runs, and the result is the switch-off handles' to their own spread."""
    p = cameras_scene(problems, n_cams)
    k = {"1": 1, "K": K, "K+1": K + 1, "max_K": K}[count]
    eta = 1e-12 if count == "max_K" else ETA
    kw = dict(max_it=k, min_it=0 if count == "max_K" else k)
    on, route, res, offs = lm_three(hip, monkeypatch, p, eta=eta, **kw)
    assert res[1].num_iterations == k, res[1]
    if count == "max_K":
        assert res[1].termination_type == hip.NO_CONVERGENCE
    assert route == (0 if count == "K+1" else 1)
    check_fixed_count(oracle, hip, p, lm_diag(oracle, p, RADIUS), res[0], res[1], res[2])
    compare(f"count_{count}_{n_cams}", res, *offs)
    if count == "K+1":   # the same route: the same spread
        spread = max(rel(offs[0][0], offs[1][0]), 1e-15)
        assert rel(res[0], offs[0][0]) <= 10 * spread, (rel(res[0], offs[0][0]), spread)
    on.close()


# ---- long points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("count", ["natural", "K"])
def test_long_points(hip, oracle, problems, monkeypatch, pipelined, count):
    """Tracks of 1 .. 600 observations: normal tiles, packed rounds of up to 8 tiles, and a point with sum and apply rounds of its own —
    in the pipelined kernel (compute_long_round) and in the 512-thread one (fused_long_rounds)."""
    p = long_scene(problems)
    cap = pipelined_cap(hip, p) if pipelined else None
    n_tiles = int(hip.debug_staged_x_plan(p.bs, p.num_eliminate_blocks)["n_tiles"])
    assert D.fused_kernel(n_tiles, cap, "f9_s0") == ("pipelined" if pipelined else "512")
    rounds = hip.debug_long_rounds(p.bs, p.num_eliminate_blocks)
    kw = dict(max_it=K, min_it=K) if count == "K" else {}
    on, route, res, offs = lm_three(hip, monkeypatch, p, grid_cap=cap, **kw)
    assert on.info().camera_accum_in_lds == 1 and route == 1 and res[1].num_iterations <= K, (res[1], route, rounds)
    Dv = lm_diag(oracle, p, RADIUS)
    if count == "K":
        check_fixed_count(oracle, hip, p, Dv, res[0], res[1], res[2])
    else:
        check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, Dv, res[0], res[1], res[2], ETA)
    compare(f"long_{count}_{'pipelined' if pipelined else '512'}", res, *offs)
    on.close()


def test_long_scene_has_every_kind_of_round(hip, problems):
    """The plan of the long-points scene: packed rounds and a point with rounds of its own (CPU-side data, checked where the scene runs)."""
    p = long_scene(problems)
    r = hip.debug_long_rounds(p.bs, p.num_eliminate_blocks)
    flags = np.asarray(r["round_flag"])
    assert (flags == 0).any() and (flags & 1).any() and (flags & 2).any() and ((flags & 5) == 5).any(), np.unique(flags)


# ---- other shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e4_f6_s0", "r3_e3_f3_s0"])
@pytest.mark.parametrize("grid_cap", [None, 3])
def test_other_shapes(hip, oracle, problems, monkeypatch, name, grid_cap):
    """<2,4,6> (4-wide points: ten packed entries per inverse) and <3,3,3> (3-high rows), on the 512- and the 1024-thread kernels."""
    p = D.few_cameras(problems, name)
    on = handle(hip, monkeypatch, p, True, grid_cap=grid_cap)
    res = on.lm_compute_step(p.values, p.b, RADIUS, ETA)
    assert on.info().kernel_path == hip.PATH_BAL and on.last_backsub_route() == 1 and res[1].num_iterations <= K, res[1]
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), res[0], res[1], res[2], ETA)
    offs = []
    for _ in range(2):
        off = handle(hip, monkeypatch, p, False, grid_cap=grid_cap)
        offs.append(off.lm_compute_step(p.values, p.b, RADIUS, ETA))
        off.close()
    compare(f"shape_{name}_{grid_cap}", res, *offs)
    on.close()


# ---- retry, entry points, speculation off -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cams", [40, 80])
def test_retry_on_resident_tiles(hip, oracle, problems, monkeypatch, n_cams):
    """values_unchanged with a smaller radius: kInit runs again on the resident tiles and leaves E^T b again."""
    p = cameras_scene(problems, n_cams)
    hs = [handle(hip, monkeypatch, p, sw) for sw in (True, False, False)]
    for s in hs:
        s.lm_compute_step(p.values, p.b, RADIUS, ETA)
    res = [s.lm_compute_step(None, None, RADIUS / 8, ETA, reuse_diagonal=True, values_unchanged=True) for s in hs]
    assert [s.last_backsub_route() for s in hs] == [1, 0, 0] and res[0][1].num_iterations <= K
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS / 8), res[0][0], res[0][1], res[0][2], ETA)
    compare(f"retry_{n_cams}", *res)
    for s in hs:
        s.close()


@pytest.mark.parametrize("n_cams", [40, 80])
def test_solve_entry_points(hip, oracle, problems, monkeypatch, n_cams):
    """solve and solve_unchanged_values with the caller's D (no negation, no model cost), and the device-pointer LM entry point: each
    against the oracle and against two switch-off handles, at the bound of compare()."""
    import torch
    p = cameras_scene(problems, n_cams)
    m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
    hs = [handle(hip, monkeypatch, p, sw) for sw in (True, False, False)]
    D1, D2 = lm_diag(oracle, p, RADIUS), lm_diag(oracle, p, RADIUS / 4)
    for which, Dv in (("solve", D1), ("unchanged", D2)):
        opt = hip.PerSolveOptions(D=Dv, q_tolerance=ETA, r_tolerance=-1.0)
        res = [(h.solve(p.values, p.b, opt) if which == "solve" else h.solve_unchanged_values(opt)) for h in hs]
        assert [h.last_backsub_route() for h in hs] == [1, 0, 0]
        (x, s), (xa, sa), (xb, sb) = res
        assert s.termination_type == sa.termination_type == sb.termination_type == hip.SUCCESS
        assert s.num_iterations == sa.num_iterations == sb.num_iterations <= K
        xo, so = m.iterative_schur_solve(p.values, p.b, Dv, preconditioner=SCHUR_JACOBI, min_it=s.num_iterations, max_it=s.num_iterations,
                                         q_tol=-1.0, r_tol=-1.0)
        assert rel(x, xo) <= 1e-9, rel(x, xo)
        spread, diff = rel(xa, xb), rel(x, xa)
        bound = max(10 * spread, 1e-11)
        report(f"{which}_{n_cams}", iterations=s.num_iterations, off_off_step=spread, on_off_step=diff, bound_step=bound)
        assert diff <= bound, (which, diff, bound)
    dev = torch.device("cuda:0")
    tv, tb = torch.from_numpy(p.values).to(dev), torch.from_numpy(p.b).to(dev)
    torch.cuda.synchronize()
    res = []
    for h in hs:
        tx = torch.full((p.num_cols,), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        summ, mcc, finite = h.lm_compute_step_device(tv.data_ptr(), tb.data_ptr(), tx.data_ptr(), RADIUS, ETA)
        assert finite
        res.append((tx.cpu().numpy(), summ, mcc))
    assert [h.last_backsub_route() for h in hs] == [1, 0, 0]
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, D1, res[0][0], res[0][1], res[0][2], ETA)
    compare(f"device_pointers_{n_cams}", *res)
    for h in hs:
        h.close()


@pytest.mark.parametrize("n_cams", [40, 80])
def test_without_speculation(hip, oracle, problems, monkeypatch, n_cams):
    """CERES_HIP_SPECULATE=0: the host picks the route after the poll, by the same rule."""
    p = cameras_scene(problems, n_cams)
    on, route, res, offs = lm_three(hip, monkeypatch, p, speculate=0)
    assert route == 1 and res[1].num_iterations <= K
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), res[0], res[1], res[2], ETA)
    compare(f"no_speculation_{n_cams}", res, *offs)
    on.close()
    # ... and a solve past K there
    on = handle(hip, monkeypatch, p, True, speculate=0, max_it=K + 2, min_it=K + 2)
    res = on.lm_compute_step(p.values, p.b, RADIUS, ETA)
    assert on.last_backsub_route() == 0 and res[1].num_iterations == K + 2
    check_fixed_count(oracle, hip, p, lm_diag(oracle, p, RADIUS), res[0], res[1], res[2])
    on.close()


# ---- history independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cams", [40, 80])
def test_route_does_not_depend_on_earlier_solves(hip, oracle, problems, monkeypatch, n_cams):
    """A handle whose previous solve went past K (its next first batch of CG iterations is that long: the pass over J is enqueued beside the
    tail, and the device picks) against a fresh handle: the same route, the same iterations, the same step."""
    p = cameras_scene(problems, n_cams)
    used, fresh = handle(hip, monkeypatch, p, True), handle(hip, monkeypatch, p, True)
    long_res = used.lm_compute_step(p.values, p.b, RADIUS, 1e-8)
    assert long_res[1].num_iterations > K and used.last_backsub_route() == 0, long_res[1]
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), long_res[0], long_res[1], long_res[2], 1e-8)
    a = used.lm_compute_step(p.values, p.b, RADIUS, ETA)
    b = fresh.lm_compute_step(p.values, p.b, RADIUS, ETA)
    assert used.last_backsub_route() == fresh.last_backsub_route() == 1
    assert a[1].num_iterations == b[1].num_iterations <= K and a[1].termination_type == b[1].termination_type
    assert rel(a[0], b[0]) <= 1e-12 and abs(a[2] - b[2]) <= 1e-12 * abs(b[2]), (rel(a[0], b[0]), a[2], b[2])
    check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), a[0], a[1], a[2], ETA)
    report(f"history_{n_cams}", used_fresh_step=rel(a[0], b[0]), used_fresh_mcc=abs(a[2] - b[2]) / abs(b[2]))
    used.close()
    fresh.close()


# ---- ineligible handles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ghost_peers", "many_cameras", "camera_rows", "spse_initialization"])
def test_ineligible_handles_back_substitute_over_j(hip, oracle, problems, monkeypatch, kind):
    monkeypatch.setenv("CERES_HIP_POINT_TAIL", "1")
    if kind == "many_cameras":   # the accumulators leave LDS
        p = problems.synthetic_bal(None, layout="schur", num_cameras=2500, num_points=12000, num_observations=62000, seed=43, skew=0.4)
    else:
        p = cameras_scene(problems, 40)
    if kind == "camera_rows":    # rows without a point cell: outside the tiles
        p = problems.add_camera_rows(p, 12, seed=5)
    o = hip.LinearSolverOptions(type=SCHUR, preconditioner_type=SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=300,
                                elimination_groups=[p.num_eliminate_blocks], use_spse_initialization=kind == "spse_initialization",
                                max_num_spse_iterations=5, spse_tolerance=0.1)
    s = hip.HipLinearSolver(o, ghost_world=8, p2p_max_elements=99 * 40 + 2) if kind == "ghost_peers" else hip.HipLinearSolver(o)
    s.set_structure(p.bs)
    if kind == "spse_initialization":
        m = oracle.Matrix(p.bs, p.num_eliminate_blocks)
        Dv = lm_diag(oracle, p, RADIUS)
        x, summ = s.solve(p.values, p.b, hip.PerSolveOptions(D=Dv, q_tolerance=ETA, r_tolerance=-1.0))
        xo, so = oracle.iterative_schur_solve_spse(m, p.values, p.b, Dv, preconditioner=SCHUR_JACOBI, min_it=0, max_it=300, q_tol=ETA,
                                                   r_tol=-1.0, use_spse_initialization=True, max_num_spse_iterations=5, spse_tolerance=0.1)
        assert summ.termination_type == so.termination_type == hip.SUCCESS and abs(summ.num_iterations - so.num_iterations) <= 1
        if summ.num_iterations == so.num_iterations:
            assert rel(x, xo) <= 1e-8
    else:
        step, summ, mcc = s.lm_compute_step(p.values, p.b, RADIUS, ETA)
        check_step(oracle, hip, p, SCHUR, SCHUR_JACOBI, lm_diag(oracle, p, RADIUS), step, summ, mcc, ETA)
    assert summ.num_iterations <= K and s.last_backsub_route() == 0, (summ, s.last_backsub_route())
    s.close()


# ---- poisoned allocations ---------------------------------------------------------------------------------------------------------------
def child_main():
    """In the child interpreter (CERES_HIP_DEBUG_POISON=nan): natural stops and min = max = 1 (buffers 2 .. K stay poisoned) on the three
    scenes, the retry, and a used handle; one JSON line each."""
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the HIP library, as tests/test_gpu_schur_state.py loads it)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    hip = pkg.hip_solver
    hip.load_library()

    class Env:   # monkeypatch's two methods on os.environ
        setenv = staticmethod(lambda k, v: os.environ.__setitem__(k, v))
        delenv = staticmethod(lambda k, raising=False: os.environ.pop(k, None))
    failed = 0
    scenes = (("cameras_40", cameras_scene(pkg.problems, 40), None), ("cameras_80", cameras_scene(pkg.problems, 80), "cap"),
              ("long", long_scene(pkg.problems), None), ("long_pipelined", long_scene(pkg.problems), "cap"))
    for name, p, cap in scenes:
        cap = pipelined_cap(hip, p) if cap else None
        for kw in (dict(), dict(max_it=1, min_it=1)):
            bad = {}
            try:
                s = handle(hip, Env, p, True, grid_cap=cap, **kw)
                for radius, retry in ((RADIUS, False), (RADIUS / 8, True)):
                    step, summ, mcc = (s.lm_compute_step(None, None, radius, ETA, reuse_diagonal=True, values_unchanged=True) if retry
                                       else s.lm_compute_step(p.values, p.b, radius, ETA))
                    assert s.last_backsub_route() == 1 and np.isfinite(step).all() and np.isfinite(mcc), (summ, mcc)
                    check_fixed_count(oracle, hip, p, lm_diag(oracle, p, radius), step, summ, mcc)
                s.close()
            except AssertionError as ex:
                bad = {"assertion": repr(ex)[:400]}
            failed += bool(bad)
            print(json.dumps({"scene": name, "options": kw, "bad": bad}), flush=True)
    return 1 if failed else 0


def test_poisoned_allocations(hip):
    """Every new floating-point device buffer filled with NaN, in a fresh child interpreter: a capture buffer, an E^T b or an alpha read
    before it is written shows in the step.  A signal or a time-out is a failure to investigate, not to rerun."""
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan")
    env.pop("CERES_HIP_POINT_TAIL_REPORT", None)
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gpu_point_tail as t; sys.exit(t.child_main())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "CERES_HIP_DEBUG_POISON=nan: new floating-point device buffers are filled" in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and len(lines) == 8 and all('"bad": {}' in ln for ln in lines), \
        f"exit {r.returncode}\n" + "\n".join(lines) + "\n" + r.stderr[-3000:]
