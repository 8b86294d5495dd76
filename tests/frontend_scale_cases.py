"""One "wide" BAL scene beyond every grid cap of the front end's kernels (csrc/device.h: kMaxEvalGrid, kMaxLsCameraGrid, kMaxVecGrid), and
the configurations tests/test_gpu_frontend_scale.py runs on it; tests/test_frontend_scale_cpu.py holds the scene to exceed the caps by a
real second trip of the grid-stride loops and the line search restatement's runs on it to be non-degenerate.  numpy and the oracle only.

The scene: oracle.BalProblem.generate (longest track 29, largest camera degree 48 at this size) plus
  - long points (65, 129 and 300 observations) at the highest point ids — the last rows of the device's point-grouped row order — and
    three more just below the ten points the reduced program holds constant;
  - cameras of more than one 64-row chunk (65, 257, 1000 observations) at the highest camera ids, and one more below the camera the
    reduced program holds constant;
the observations shuffled (the device's grouping has to sort them).  The generator's pixels are kept (the true scene's projections plus
noise) and its parameter noise is 0.25: residuals of some 25 px, coherent over a point's rows.  The added observations' pixels are the
projection at the state plus noise of 10 px.  With every pixel the state's projection plus 1 px of noise, a block's gradient is a sum of
noise terms that may cancel to a hundredth of its terms, each the difference of two pixels of several hundred: two float64 references
(angle-axis and quaternion cameras) then differ by 6e-12 of a point block, above the per-block tolerance; on this scene by 1.5e-13
(design/18_frontend_scale.md)."""
import functools
import os
import re
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import constant_blocks_reference as CB
import line_search_cases as C
import line_search_reference as LS

NUM_CAMERAS, NUM_POINTS, GENERATED_OBSERVATIONS, SEED = 20000, 150000, 598000, 71
LONG_POINT_ROWS = {NUM_POINTS - 13: 65, NUM_POINTS - 12: 129, NUM_POINTS - 11: 300, NUM_POINTS - 3: 65, NUM_POINTS - 2: 129, NUM_POINTS - 1: 300}
HEAVY_CAMERA_ROWS = {NUM_CAMERAS - 4: 1001, NUM_CAMERAS - 3: 65, NUM_CAMERAS - 2: 257, NUM_CAMERAS - 1: 1000}
PARAM_NOISE, PIXEL_NOISE = 0.25, 10.0

# The losses' scale is the scene's residual scale (|r|^2 has its median near 900 px^2: 39 % of the rows are inliers of a = 25, both
# branches of Huber are taken by many rows).  With a = 1 — 0.09 % inliers — Cauchy weighs a row by 1 / (1 + |r|^2): a block's gradient
# is then the few rows whose residual is the small difference of two pixels of several hundred, and two float64 references
# (angle-axis and quaternion cameras, the same point blocks) already differ by 2.7e-12 of a block there, 1.5e-13 with a = 25.
HUBER, CAUCHY = ("huber", 25.0, 1.0, 1.0), ("cauchy", 25.0, 1.0, 1.0)
# constant (cameras, points): the reduced program's constant-block lists reach into the second trip as well
MASKS = {"none": (None, None),
         "reduced": ([0, NUM_CAMERAS - 1], list(range(10)) + list(range(NUM_POINTS - 10, NUM_POINTS)))}


DEVICE_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ceres-solver_amd", "csrc", "device.h")


@functools.lru_cache(maxsize=None)
def caps():
    """What one launch covers without a second trip of its grid-stride loop, from the constants of csrc/device.h:
    rows (bal_evaluate_kernel: kVecBlock rows per workgroup; ls_point_pass_kernel: four 64-row chunks per workgroup), tiles
    (bal_evaluate_tiles_kernel: four per workgroup), camera_chunks (ls_camera_pass_kernel: four per workgroup) and vector (the vector
    kernels: kVecBlock scalars — or free blocks, ls_plus_kernel — per workgroup)."""
    with open(DEVICE_H) as f:
        k = {name: int(v) for name, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", f.read())}
    assert k["kVecBlock"] == 4 * 64
    return dict(rows=k["kMaxEvalGrid"] * k["kVecBlock"], tiles=k["kMaxEvalGrid"] * 4, camera_chunks=k["kMaxLsCameraGrid"] * 4,
                vector=k["kMaxVecGrid"] * k["kVecBlock"], constants=k)


def chunks(degrees):
    """ceil(d / 64) chunks per block, block-major: (first chunk of every block, chunks of every block)."""
    n = (np.asarray(degrees, dtype=np.int64) + 63) // 64
    return np.concatenate([[0], np.cumsum(n)[:-1]]), n


def _project(oracle, cam, pt, state, seed, noise):
    """Pixels of the (camera, point) pairs at `state` — the residual with a zero observation — plus noise, as
    test_gpu_line_search.project makes them."""
    cams = state[3 * NUM_POINTS:].reshape(-1, 9)[cam]
    pts = state[:3 * NUM_POINTS].reshape(-1, 3)[pt]
    r, _, _ = oracle.snavely_batch(cams, pts, np.zeros((cam.shape[0], 2)))
    return r + np.random.default_rng(seed).normal(0.0, noise, r.shape)


def build_scene(oracle, param_noise=PARAM_NOISE, pixel_noise=PIXEL_NOISE):
    """(camera_index, point_index, observations, state) before the oracle has read them back."""
    base = oracle.BalProblem.generate(NUM_CAMERAS, NUM_POINTS, GENERATED_OBSERVATIONS, param_noise=param_noise, seed=SEED)
    base.build_structure(True)
    cam, pt, obs = base.indices()
    state = base.state()
    rng = np.random.default_rng(SEED)
    cams, pts = [cam], [pt]
    ordinary_cameras, ordinary_points = NUM_CAMERAS - len(HEAVY_CAMERA_ROWS), min(LONG_POINT_ROWS)
    for q, rows in LONG_POINT_ROWS.items():   # (cameras below the heavy ones: the heavy cameras' lengths stay as listed)
        seen = cam[pt == q]
        add = rng.choice(np.setdiff1d(np.arange(ordinary_cameras), seen), rows - seen.shape[0], replace=False)
        cams.append(add.astype(np.int32))
        pts.append(np.full(add.shape[0], q, np.int32))
    for c, rows in HEAVY_CAMERA_ROWS.items():   # (points below the long ones: the long points' lengths stay as listed)
        seen = pt[cam == c]
        add = rng.choice(np.setdiff1d(np.arange(ordinary_points), seen), rows - seen.shape[0], replace=False)
        cams.append(np.full(add.shape[0], c, np.int32))
        pts.append(add.astype(np.int32))
    generated = cam.shape[0]
    cam, pt = np.concatenate(cams), np.concatenate(pts)
    obs = np.concatenate([obs, _project(oracle, cam[generated:], pt[generated:], state, SEED + 1, pixel_noise)])
    order = rng.permutation(cam.shape[0])
    return np.ascontiguousarray(cam[order]), np.ascontiguousarray(pt[order]), np.ascontiguousarray(obs[order]), state


@functools.lru_cache(maxsize=None)
def oracle_problem(oracle):
    """The scene as the oracle's BalProblem (structure built, Schur ordering): evaluate and lm_solve run on it.  The oracle takes a scene
    from a BAL file only; %.16e round-trips a double, so what it read is what was built (asserted)."""
    cam, pt, obs, state = build_scene(oracle)
    problems = sys.modules["ceres_solver_amd"].problems
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scale.txt")
        problems.write_bal(path, NUM_CAMERAS, NUM_POINTS, cam, pt, obs, np.concatenate([state[3 * NUM_POINTS:], state[:3 * NUM_POINTS]]))
        op = oracle.BalProblem.read(path)
    op.build_structure(True)
    cam2, pt2, obs2 = op.indices()
    assert np.array_equal(cam2, cam) and np.array_equal(pt2, pt) and np.array_equal(obs2, obs) and np.array_equal(op.state(), state)
    return op


@functools.lru_cache(maxsize=None)
def scene(oracle):
    """(num_cameras, num_points, camera_index, point_index, observations, angle-axis state): the tuple line_search_cases works on."""
    op = oracle_problem(oracle)
    cam, pt, obs = op.indices()
    state = op.state()
    for a in (cam, pt, obs, state):
        a.setflags(write=False)
    return NUM_CAMERAS, NUM_POINTS, cam, pt, obs, state


def initial_state(oracle, camera):
    return C.initial_state(scene(oracle), camera)


class _RowRanges:
    """frontend_reference.Problem with evaluate and cost run over ranges of rows in threads: every range by an evaluator of the wrapped
    one's class (robust_reference.Evaluator / quaternion_reference.Evaluator, unchanged) on those rows alone, the costs and gradients of
    the ranges added in range order, residuals and values put back in row order.  Per row the same arithmetic as the wrapped evaluator;
    numpy and the oracle release the interpreter lock, so 600 000 rows of the complex-step Jacobian take a second instead of several
    (tests/test_frontend_scale_cpu.py holds it to the plain evaluator)."""

    def __init__(self, full, pieces):
        self._full = full
        ev = full.ev
        edges = np.linspace(0, ev.n_rows, min(pieces, ev.n_rows) + 1).astype(np.int64)
        make = (lambda rows: type(ev)(ev.model, ev.nc, ev.np_, ev.cam, ev.pt, ev.obs, rows, ev.loss)) if full.quaternion else \
            (lambda rows: type(ev)(ev.snavely, ev.nc, ev.np_, ev.cam, ev.pt, ev.obs, rows, ev.loss))
        self._parts = [make(np.arange(lo, hi)) for lo, hi in zip(edges[:-1], edges[1:])]
        self._pool = ThreadPoolExecutor(max_workers=len(self._parts))

    def __getattr__(self, name):
        return getattr(self._full, name)

    def cost(self, x):
        return float(sum(self._pool.map(lambda p: p.cost(x), self._parts)))

    def evaluate(self, x):
        out = list(self._pool.map(lambda p: p.evaluate(x), self._parts))
        cost, g = 0.0, np.zeros_like(out[0][3])
        for c, _, _, gk in out:
            cost += c
            g += gk
        vals = [o[2][:6 * p.n_rows] for o, p in zip(out, self._parts)] + [o[2][6 * p.n_rows:] for o, p in zip(out, self._parts)]
        return float(cost), np.concatenate([o[1] for o in out]), np.concatenate(vals), g


def row_parallel(problem, pieces=None):
    """The constant_blocks_reference.Problem itself, its full evaluator replaced by _RowRanges over at most 16 threads."""
    problem.full = _RowRanges(problem.full, pieces or max(1, min(16, os.cpu_count() or 1)))
    return problem


@functools.lru_cache(maxsize=None)
def reference_problem(oracle, camera, loss, masks):
    cc, cp = MASKS[masks]
    return row_parallel(C.reference_problem(oracle, scene(oracle), camera, loss, cc, cp))


# (camera, loss, masks) of the configurations whose residuals and Jacobian values are compared; the gradient-only ones keep cost and gradient
EVALUATE_CONFIGS = [("angle_axis", HUBER, "none"), ("quaternion", None, "none"), ("quaternion_manifold", CAUCHY, "none"),
                    ("angle_axis", HUBER, "reduced"), ("quaternion_manifold", CAUCHY, "reduced")]
GRADIENT_CONFIGS = [(camera, loss, "none") for camera in C.MODELS for loss in (None, HUBER)] + \
    [("angle_axis", HUBER, "reduced"), ("quaternion_manifold", HUBER, "reduced")]


@functools.lru_cache(maxsize=None)
def reference_evaluation(oracle, camera, loss, masks):
    """(problem, x0, cost, residuals, values, gradient) of constant_blocks_reference.Problem.evaluate, once per configuration, read-only;
    residuals and values (115 MB a configuration) are kept for EVALUATE_CONFIGS only, None otherwise."""
    w = reference_problem(oracle, camera, loss, masks)
    x0 = initial_state(oracle, camera)
    cost, r, vals, g = w.evaluate(x0)
    if (camera, loss, masks) not in EVALUATE_CONFIGS:
        r = vals = None
    for a in (x0, r, vals, g):
        if a is not None:
            a.setflags(write=False)
    return w, x0, cost, r, vals, g


def row_cost_terms(w, x):
    """rho(|r|^2) / 2 of every kept row of a constant_blocks_reference.Problem, in its row order: the terms its cost adds up."""
    import robust_reference as R
    ev = w.full.ev
    if w.model == 0:
        r = ev._blocks(x)[0]
    else:
        import quaternion_reference as Q
        r = Q.residual(*ev._rows(x), ev.obs)
    s = np.sum(r * r, axis=1)
    return 0.5 * (s if w.loss is None else R.rho(w.loss[0], s, *w.loss[1:])[0])


# ---- the line search minimizer's runs: name -> (camera, loss, masks, options) ----
LINE_SEARCH_ITERATIONS = 3
LINE_SEARCH_CASES = {
    "lbfgs_default": ("angle_axis", None, "none", dict()),
    "lbfgs_manifold_huber_reduced": ("quaternion_manifold", HUBER, "reduced", dict()),
    "ncg_polak_ribiere": ("quaternion", None, "none",
                          dict(line_search_direction_type=LS.NONLINEAR_CONJUGATE_GRADIENT, nonlinear_conjugate_gradient_type=LS.POLAK_RIBIERE)),
}


@functools.lru_cache(maxsize=None)
def run_line_search_reference(oracle, name):
    """(problem, x0, (x, summary)) of line_search_reference.minimize on a case, once."""
    camera, loss, masks, opts = LINE_SEARCH_CASES[name]
    w = reference_problem(oracle, camera, loss, masks)
    x0 = initial_state(oracle, camera)
    return w, x0, LS.minimize(w, x0, max_num_iterations=LINE_SEARCH_ITERATIONS, **opts)
