"""The line search minimizer on the device, through the C ABI: the gradient-only evaluator (ceres_hip_bal_evaluate_gradient) against the
front-end references' evaluators and against the handle's own Jacobian-form evaluation, the L-BFGS operator
(ceres_hip_debug_lbfgs_direction) against the numpy two-loop recursion, and ceres_hip_bal_minimize_line_search against
tests/line_search_reference.py on the runs tests/test_line_search_cpu.py holds to be non-degenerate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import constant_blocks_reference as CB
import line_search_cases as C
import line_search_reference as LS
from test_gpu_inner_iterations import scene as inner_scene_of
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

OP_TOL = 1e-12
MODELS = C.MODELS
LOSSES = {"none": None, "huber": ("huber", 1.0, 1.0, 1.0), "cauchy": ("cauchy", 1.0, 1.0, 1.0)}
HERE = os.path.dirname(os.path.abspath(__file__))


def project(oracle, nc, npts, cam, pt, state, seed, noise=1.0):
    """Pixels of the given (camera, point) pairs at `state` (the angle-axis evaluator's residual with a zero observation), noise added."""
    import robust_reference as R
    ev = R.Evaluator(oracle.snavely_batch, nc, npts, cam, pt, np.zeros((cam.shape[0], 2)), np.arange(cam.shape[0]))
    _, r, _, _ = ev.evaluate(state)
    return r.reshape(-1, 2) + np.random.default_rng(seed).normal(0.0, noise, (cam.shape[0], 2))


def tiny_scene(oracle):
    """(i) 3 cameras, 7 points, 19 observations — less than one wavefront.  Camera 2 sees the points 2 .. 6 only."""
    op = oracle.BalProblem.generate(3, 7, 21, seed=2)
    op.build_structure(True)
    st = op.state()
    cam = np.array([0] * 7 + [1] * 7 + [2] * 5, dtype=np.int32)
    pt = np.array(list(range(7)) * 2 + list(range(2, 7)), dtype=np.int32)
    return 3, 7, cam, pt, project(oracle, 3, 7, cam, pt, st, 1), st


BUILT_POINT_ROWS = [64, 65, 100, 60, 58, 58, 58, 59, 59, 59, 59, 1]   # 700 rows: 10 chunks of 64 and 60 more
BUILT_CAMERA_ROWS = [1, 64, 65, 257, 313]


def built_scene(oracle):
    """(iii) 700 observations over 12 points and FIVE cameras (the four prescribed camera lengths 1, 64, 65 and 257 leave 313 of the 700
    rows to a fifth camera).  Points of exactly 64 and exactly 65 rows (rows 0 .. 63: one whole chunk; 64 .. 128: a chunk and one row),
    point 3 on rows 229 .. 288 across the 256-row workgroup boundary, a last point of one row, 700 = 10 x 64 + 60.  With 5 cameras a
    point of 64 rows sees cameras more than once: several residual blocks on one (camera, point) pair."""
    nc, npts = len(BUILT_CAMERA_ROWS), len(BUILT_POINT_ROWS)
    op = oracle.BalProblem.generate(nc, npts, 40, seed=4)
    op.build_structure(True)
    st = op.state()
    pt = np.repeat(np.arange(npts), BUILT_POINT_ROWS).astype(np.int32)
    cam = np.repeat(np.arange(nc), BUILT_CAMERA_ROWS).astype(np.int32)
    np.random.default_rng(9).shuffle(cam)
    assert pt.shape[0] == cam.shape[0] == 700 and np.array_equal(np.bincount(cam), BUILT_CAMERA_ROWS)
    return nc, npts, cam, pt, project(oracle, nc, npts, cam, pt, st, 3, noise=2.0), st


@pytest.fixture(scope="module")
def scenes(oracle):
    return {"tiny": tiny_scene(oracle), "inner": inner_scene_of(oracle), "built": built_scene(oracle)}


def device_problem(hip, sc, camera, cc=None, cp=None, solver=(5, 2), generic=False):
    nc, npts, cam, pt, obs, _ = sc
    o = hip.LinearSolverOptions(type=solver[0], preconditioner_type=solver[1], min_num_iterations=0, max_num_iterations=500,
                                force_generic_path=generic)
    kw = {}
    if cc is not None or cp is not None:
        kw = dict(constant_cameras=CB.mask(cc, nc), constant_points=CB.mask(cp, npts))
    return hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=camera, **kw)


def block_deviation(g, gr, w):
    """max over the free blocks (3 per point, cw per camera) of max |g - gr| / max |gr| of the block"""
    nfp = int(np.count_nonzero(w.pcol >= 0))
    assert g.shape[0] == gr.shape[0] and g.shape[0] > 3 * nfp and (g.shape[0] - 3 * nfp) % w.cw == 0
    first = np.concatenate([np.arange(0, 3 * nfp, 3), np.arange(3 * nfp, g.shape[0], w.cw)])   # (one pass: 170 000 blocks at scale)
    return float(np.max(np.maximum.reduceat(np.abs(g - gr), first) / np.maximum.reduceat(np.abs(gr), first)))


_REFERENCE = {}


def reference_gradient(oracle, scenes, name, camera, loss, cc=None, cp=None):
    """(problem, x0, cost, gradient) of the reference evaluator, computed once per configuration and shared."""
    key = (name, camera, loss, tuple(cc or ()), tuple(cp or ()))
    if key not in _REFERENCE:
        sc = scenes[name]
        w = C.reference_problem(oracle, sc, camera, LOSSES[loss], cc, cp)
        x0 = C.initial_state(sc, camera)
        cost, _, _, g = w.evaluate(x0)
        _REFERENCE[key] = (w, x0, cost, g)
    return _REFERENCE[key]


def check_gradient(gp, w, x0, cost_r, g_r):
    cost, g = gp.evaluate_gradient(x0)
    cost2, g2 = gp.evaluate_gradient(x0)
    assert cost == cost2 and np.array_equal(g, g2)   # no atomics, a fixed order: the same bits
    cost_only, none = gp.evaluate_gradient(x0, gradient=False)
    assert none is None and cost_only == cost
    dc, dg = abs(cost - cost_r) / cost_r, block_deviation(g, g_r, w)
    cost_j, _, g_j, _ = gp.evaluate(x0, gradient=True)
    dj = abs(cost - cost_j) / cost_j, block_deviation(g, g_j, w)
    print("cost", dc, "gradient", dg, "against evaluate()", dj)
    assert dc <= OP_TOL and dg <= OP_TOL and max(dj) <= OP_TOL
    return cost, g


# ---- 6. the gradient evaluator ----
@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("camera", list(MODELS))
@pytest.mark.parametrize("name", ["tiny", "inner", "built"])
def test_gradient_matches_the_reference_evaluator(hip, oracle, scenes, name, camera, loss):
    w, x0, cost_r, g_r = reference_gradient(oracle, scenes, name, camera, loss)
    gp = device_problem(hip, scenes[name], camera)
    try:
        if LOSSES[loss]:
            gp.set_loss(*LOSSES[loss])
        before = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)
        check_gradient(gp, w, x0, cost_r, g_r)
        after = gp.evaluate(x0, residuals=True, gradient=True, jacobian=True)   # the new path leaves the handle as it was
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3])
        assert rel(after[2], before[2]) <= OP_TOL   # (J^T r of the loaded values: the solver's own sums, repeatable to rounding)
    finally:
        gp.close()


@pytest.mark.parametrize("solver,generic", [((5, 2), True), ((3, 0), False), ((5, 4), False), ((6, 1), False)],
                         ids=["generic_path", "dense_schur", "cluster_jacobi", "cgnr"])
def test_gradient_works_on_every_kind_of_handle(hip, oracle, scenes, solver, generic):
    w, x0, cost_r, g_r = reference_gradient(oracle, scenes, "built", "angle_axis", "huber")
    gp = device_problem(hip, scenes["built"], "angle_axis", solver=solver, generic=generic)
    try:
        gp.set_loss(*LOSSES["huber"])
        check_gradient(gp, w, x0, cost_r, g_r)
    finally:
        gp.close()


POISON_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
hs = entry.load_package().hip_solver
hs.load_library()
d = np.load(%(scene)r)
o = hs.LinearSolverOptions(type=5, preconditioner_type=2, min_num_iterations=0, max_num_iterations=100)
gp = hs.BalProblem(o, int(d["nc"]), int(d["npts"]), d["cam"], d["pt"], d["obs"], constant_cameras=d["cc"], constant_points=d["cp"])
gp.set_loss("huber", 1.0)
cost, g = gp.evaluate_gradient(d["x0"])
x, S = gp.minimize_line_search(d["x0"], max_num_iterations=3, max_lbfgs_rank=2)
print("RESULT " + json.dumps(dict(cost=cost, nan=int(np.isnan(g).sum()), g=g.tolist(), final=S.final_cost, x_nan=int(np.isnan(x).sum()))))
gp.close()
"""


def test_poisoned_allocations_do_not_reach_the_gradient(hip, oracle, scenes, tmp_path):
    """CERES_HIP_DEBUG_POISON=nan set before the library is loaded (a child process: the switch is read once per process): every
    gradient entry of a free block is written on every call — also a camera whose only rows are against constant points."""
    sc = scenes["built"]
    nc, npts, cam, pt, obs, _ = sc
    cc, cp = [4], [11, 0]
    w, x0, cost_r, g_r = reference_gradient(oracle, scenes, "built", "angle_axis", "huber", cc, cp)
    path = str(tmp_path / "scene.npz")
    np.savez(path, nc=nc, npts=npts, cam=cam, pt=pt, obs=obs, x0=x0, cc=CB.mask(cc, nc).astype(bool), cp=CB.mask(cp, npts).astype(bool))
    env = dict(os.environ, CERES_HIP_DEBUG_POISON="nan", CERES_HIP_NO_TORCH="1")
    code = POISON_CHILD % dict(root=os.path.dirname(HERE), tests=HERE, scene=path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "new floating-point device buffers are filled" in r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert out["nan"] == 0 and out["x_nan"] == 0 and np.isfinite(out["final"])
    assert abs(out["cost"] - cost_r) <= OP_TOL * cost_r and block_deviation(np.array(out["g"]), g_r, w) <= OP_TOL


# ---- 7. constant blocks ----
@pytest.mark.parametrize("camera", list(MODELS))
@pytest.mark.parametrize("cc,cp", [([0, 5], None), (None, list(range(10))), ([0, 5], list(range(10)))], ids=["cameras", "points", "both"])
def test_gradient_of_a_reduced_program(hip, oracle, scenes, cc, cp, camera):
    """A constant point's cameras still get those observations' contributions; the constant blocks have no entries."""
    w, x0, cost_r, g_r = reference_gradient(oracle, scenes, "inner", camera, "huber", cc, cp)
    gp = device_problem(hip, scenes["inner"], camera, cc, cp)
    try:
        gp.set_loss(*LOSSES["huber"])
        assert gp.num_effective_parameters == g_r.shape[0]
        check_gradient(gp, w, x0, cost_r, g_r)
    finally:
        gp.close()


def test_camera_whose_points_are_all_constant_gets_its_full_sum(hip, oracle, scenes):
    """Scene (i): camera 2 sees the points 2 .. 6 only; with them constant its gradient is the sum over its five rows, not zero."""
    cp = [2, 3, 4, 5, 6]
    w, x0, cost_r, g_r = reference_gradient(oracle, scenes, "tiny", "angle_axis", "none", None, cp)
    gp = device_problem(hip, scenes["tiny"], "angle_axis", None, cp)
    try:
        _, g = check_gradient(gp, w, x0, cost_r, g_r)
        assert np.max(np.abs(g[-9:])) > 0.0 and np.max(np.abs(g_r[-9:])) > 0.0
    finally:
        gp.close()


# ---- 8. the L-BFGS operator ----
def lbfgs_updates(n, rank, seed):
    """2 rank + 1 pairs (the circular buffer wraps); pair 1 fails the secant test (s.y < 0), pair 2 has s.y = 2e-10 (just accepted)."""
    rng = np.random.default_rng(seed)
    k = 2 * rank + 1
    dx = rng.standard_normal((k, n))
    dg = dx * rng.uniform(0.5, 2.0, (k, n)) + (0.1 * rng.standard_normal((k, n)) if n > 1 else 0.0)
    dg[1] = -dg[1]
    dg[2] *= 2e-10 / float(dx[2] @ dg[2])
    return dx, dg, rng.standard_normal(n)


def two_loop(rank, dx, dg, g, scaling, dtype):
    lb = LS.LowRankInverseHessian(rank, scaling)
    acc = [int(lb.update(s.astype(dtype), y.astype(dtype))) for s, y in zip(dx, dg)]
    return lb.direction(g.astype(dtype)), np.array(acc)


@pytest.mark.parametrize("scaling", [0, 1], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("rank", [1, 3, 20])
# (beyond 65 536 elements lbfgs_total adds more than 256 partials — its p[t + kVecBlock] leg; beyond kMaxVecGrid x kVecBlock = 131 072 a
# workgroup owns several strides of elements)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, 65537, 131071, 131072, 131073, 262145, 300001])
def test_lbfgs_direction_matches_the_two_loop_recursion(hip, n, rank, scaling):
    """The bound: the float64 numpy recursion's own rounding error, measured against the same recursion in extended precision
    (np.longdouble), times 8 — the device adds the same terms in another order (tree sums of 256-element strides instead of numpy's
    pairwise blocks), which changes the error's value but not its size — plus 8 (m + 1) eps of the direction, m the live pairs: each
    of the 2 m steps rounds a quotient, a product, a difference and a sum once more than the dot products the first term covers (with
    one element both precisions often round alike and the first term is 0)."""
    dx, dg, g = lbfgs_updates(n, rank, 100 * n + rank)
    d, acc = hip.debug_lbfgs_direction(rank, dx, dg, g, scaling)
    d64, acc64 = two_loop(rank, dx, dg, g, scaling, np.float64)
    dld, _ = two_loop(rank, dx, dg, g, scaling, np.longdouble)
    assert np.array_equal(acc, acc64) and acc64[1] == 0 and acc64[2] == 1
    own = float(np.max(np.abs(d64 - dld.astype(np.float64))))
    live = min(rank, int(acc64.sum()))
    bound = 8.0 * own + 8.0 * (live + 1) * np.finfo(np.float64).eps * float(np.max(np.abs(d64)))
    err = float(np.max(np.abs(d - d64)))
    print("n", n, "rank", rank, "error", err, "bound", bound, "the reference's own", own)
    assert err <= bound


# ---- 9. the minimizer ----
VALUE_TOL = 1e-7   # a tenth of the smallest decision margin tests/test_line_search_cpu.py asserts on these runs (1e-6): values that
                   # agree this well take the same branches, so the discrete path below must be IDENTICAL


def follow_the_restatement(gp, w, x0, reference, iterations, opts, constant, label):
    """ceres_hip_bal_minimize_line_search on the handle against line_search_reference.minimize's (x, summary) of the same run: the
    discrete path identical, every logged value within VALUE_TOL (shared with tests/test_gpu_frontend_scale.py)."""
    xr, Sr = reference
    x, S = gp.minimize_line_search(x0, max_num_iterations=iterations, **opts)
    assert S.termination_type == Sr["termination_type"], S.message
    assert S.num_iterations == Sr["num_iterations"] and S.num_iterations_logged == len(Sr["iterations"])
    worst = 0.0
    for k, itr in enumerate(Sr["iterations"]):
        it = S.iterations[k]
        if k > 0:   # the discrete path
            assert (it.line_search_function_evaluations, it.line_search_gradient_evaluations, it.line_search_iterations) == \
                (itr["line_search_function_evaluations"], itr["line_search_gradient_evaluations"], itr["line_search_iterations"]), k
        for field in ("cost", "gradient_max_norm", "gradient_norm", "step_norm", "step_size"):
            a, b = getattr(it, field), itr[field]
            dev = abs(a - b) / max(abs(b), 1e-300) if b else abs(a)
            worst = max(worst, dev)
            assert dev <= VALUE_TOL, (k, field, a, b)
    print(label, "worst relative deviation over", len(Sr["iterations"]), "iterations:", worst)
    assert S.num_line_search_steps == Sr["num_line_search_steps"] and S.num_line_search_direction_restarts == Sr["num_restarts"]
    assert (S.num_function_evaluations, S.num_gradient_evaluations) == (Sr["counts"]["function"], Sr["counts"]["gradient"])
    assert abs(S.final_cost - Sr["final_cost"]) <= VALUE_TOL * Sr["final_cost"]
    assert np.linalg.norm(x - xr) <= VALUE_TOL * np.linalg.norm(xr)
    if constant:
        assert np.array_equal(x[w.constant_state], x0[w.constant_state])   # bit-identical
    if opts.get("line_search_direction_type", LS.LBFGS) == LS.LBFGS:
        assert S.lbfgs_history_bytes == 2 * opts.get("max_lbfgs_rank", 20) * gp.num_effective_parameters * 8
    return x, S


@pytest.mark.parametrize("name", list(C.ALL_CASES))
def test_minimize_line_search_follows_the_restatement(hip, oracle, name):
    seed, camera, loss, cc, cp, opts, _ = C.ALL_CASES[name]
    sc, w, x0, reference = C.run_reference(oracle, name)
    gp = device_problem(hip, sc, camera, cc, cp)
    try:
        if loss:
            gp.set_loss(*loss)
        follow_the_restatement(gp, w, x0, reference, C.COMPARED_ITERATIONS, opts, cc or cp, name)
    finally:
        gp.close()


def test_minimize_line_search_on_a_live_handle_refuses_and_leaves_it_usable(hip, oracle, scenes):
    gp = device_problem(hip, scenes["tiny"], "angle_axis")
    try:
        x0 = C.initial_state(scenes["tiny"], "angle_axis")
        with pytest.raises(hip.HipError, match="WOLFE"):
            gp.minimize_line_search(x0, line_search_type=LS.ARMIJO)
        with pytest.raises(hip.HipError, match="L-BFGS"):
            gp.minimize_line_search(x0, line_search_direction_type=LS.BFGS)
        x, S = gp.minimize_line_search(x0)
        assert S.final_cost < S.initial_cost and S.message
        xt, St = gp.minimize(x0)   # the trust-region loop still runs on the handle
        assert St.final_cost < St.initial_cost
    finally:
        gp.close()


def test_null_arguments_on_a_live_handle_are_refused_with_a_message(hip, oracle, scenes):
    """Options, state and summary of ceres_hip_bal_minimize_line_search and state and cost of ceres_hip_bal_evaluate_gradient NULL in turn
    on a live handle (tests/test_line_search_cpu.py makes the same calls with a NULL handle): CERES_HIP_E_INVALID, the handle's last
    error names what was NULL, nothing is dereferenced and the handle stays usable."""
    import ctypes
    gp = device_problem(hip, scenes["tiny"], "angle_axis")
    try:
        lib, h = gp._lib, gp._h
        x0 = np.ascontiguousarray(C.initial_state(scenes["tiny"], "angle_axis"))
        x = x0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        o, S, cost = hip.line_search_options(), hip.CLineSearchSummary(), ctypes.c_double()
        calls = {"NULL options": lambda: lib.ceres_hip_bal_minimize_line_search(h, None, x, ctypes.byref(S)),
                 "NULL state": lambda: lib.ceres_hip_bal_minimize_line_search(h, ctypes.byref(o), None, ctypes.byref(S)),
                 "NULL summary": lambda: lib.ceres_hip_bal_minimize_line_search(h, ctypes.byref(o), x, None),
                 "evaluate_gradient: NULL state": lambda: lib.ceres_hip_bal_evaluate_gradient(h, None, ctypes.byref(cost), None),
                 "evaluate_gradient: NULL cost": lambda: lib.ceres_hip_bal_evaluate_gradient(h, x, None, None)}
        for what, call in calls.items():
            rc = call()
            msg = lib.ceres_hip_bal_last_error(h).decode()
            assert rc == -1 and what in msg, (what, rc, msg)
        c, g = gp.evaluate_gradient(x0)
        assert np.isfinite(c) and np.all(np.isfinite(g))
    finally:
        gp.close()


def test_alternating_lbfgs_ranks_reuse_the_history(hip, oracle, scenes):
    """The history is kept on the handle: a rank up to the allocated one runs in the front of the same buffer (and gives what a fresh
    handle gives, to the bit), a larger one replaces it — alternating ranks do not grow the handle's device memory."""
    sc = scenes["tiny"]
    x0 = C.initial_state(sc, "angle_axis")
    gp, fresh = device_problem(hip, sc, "angle_axis"), device_problem(hip, sc, "angle_axis")
    try:
        n = gp.num_effective_parameters
        x3, S3 = gp.minimize_line_search(x0, max_num_iterations=8, max_lbfgs_rank=3)
        assert S3.lbfgs_history_bytes == 2 * 3 * n * 8
        x5, S5 = gp.minimize_line_search(x0, max_num_iterations=8, max_lbfgs_rank=5)
        assert S5.lbfgs_history_bytes == 2 * 5 * n * 8
        gp.minimize_line_search(x0, max_num_iterations=8, max_lbfgs_rank=2)   # (another path may take one more slot of the sample pool)
        held = gp.solver_info().device_bytes
        for rank in (3, 5, 2, 5):
            x, S = gp.minimize_line_search(x0, max_num_iterations=8, max_lbfgs_rank=rank)
            assert S.lbfgs_history_bytes == 2 * 5 * n * 8 and gp.solver_info().device_bytes == held
            if rank == 3:
                assert np.array_equal(x, x3) and S.final_cost == S3.final_cost
        xf, Sf = fresh.minimize_line_search(x0, max_num_iterations=8, max_lbfgs_rank=3)
        assert np.array_equal(xf, x3) and Sf.num_iterations == S3.num_iterations > 3   # (more iterations than the rank: the buffer wraps)
    finally:
        gp.close()
        fresh.close()
