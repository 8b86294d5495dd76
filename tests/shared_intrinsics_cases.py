"""The cases of the shared-intrinsics tests (tests/test_gpu_shared_intrinsics.py), shared with the CPU test that measures how well each
is conditioned (tests/test_shared_intrinsics_cpu.py): the scenes and limits of tests/test_gpu_frontend_matrix.py, the grouping layouts and
constant-camera sets of tests/shared_intrinsics_reference.py, and a table that gives every grouping layout every level of every other
factor, chosen greedily as tests/test_gpu_fixed_intrinsics.py chooses its own."""
import itertools

import numpy as np

import frontend_reference as F
import shared_intrinsics_reference as SI
from test_gpu_frontend_matrix import EDGE_INEXACT_SOLVERS, LOSS_PARAMS, NAMES, case_id, clean_scene, edge_scene, limits, tolerances

LAYOUTS = tuple(SI.LAYOUTS)
FACTORS = (
    ("solver", ((5, 2), (5, 1), (6, 1), (3, 0))),
    ("strategy", ("lm", "traditional", "subspace")),
    ("generic", (0, 1)),
    ("loss", ("none", "huber", "cauchy")),
    ("jacobi", (1, 0)),
    ("constant", SI.CONSTANT_SETS),
)


def allowed(row):
    solver, strategy = row[0], row[1]
    return strategy == "lm" or solver == (3, 0)   # DOGLEG needs an exact factorisation (DENSE_SCHUR)


def matrix_case(row):
    """The row in the form of test_gpu_frontend_matrix.CASES (angle-axis, no inner iterations, no evaluator form) and its constant set."""
    solver, strategy, generic, loss, jacobi, constant = row
    return constant, ("angle_axis", loss, 1.0, strategy, solver, generic, None, jacobi, None, None)


def build_table():
    """For every grouping layout, allowed rows chosen greedily until the layout has met every level of every factor.  Deterministic:
    ties go to the earlier row; each layout starts further down the list of rows, so that the layouts do not all take the same ones."""
    rows = [r for r in itertools.product(*(levels for _, levels in FACTORS)) if allowed(r)]
    table = []
    for m, name in enumerate(LAYOUTS):
        need = {(i, v) for i, (_, levels) in enumerate(FACTORS) for v in levels}
        pool = rows[m * 53:] + rows[:m * 53]
        while need:
            best = max(pool, key=lambda r: len(need & set(enumerate(r))))
            gain = need & set(enumerate(best))
            assert gain, need
            need -= gain
            table.append((name,) + matrix_case(best))
    return table


TABLE = build_table()


def si_id(entry):
    return entry[0] + "-" + entry[1] + "-" + case_id(entry[2])


def loss_of(case):
    c = dict(zip(NAMES, case))
    return None if c["loss"] == "none" else (c["loss"],) + LOSS_PARAMS[c["loss"]] + (c["scale"],)


# Edge-scene cases whose costs, radii and state are NOT compared: the restatement's own 8-iteration trajectory moves by more than a
# hundredth of the case's cost tolerance under jacobian_noise = (1e-14, seeds 1 and 2) — the rule and the method of
# test_gpu_frontend_matrix.EDGE_ILL_CONDITIONED.  The scenes below are chosen so that no case needs it
# (test_shared_intrinsics_cpu.test_every_table_case_is_well_conditioned measures every case on both scenes).
EDGE_ILL_CONDITIONED = {
}


def edge_values_compared(entry):
    c = dict(zip(NAMES, entry[2]))
    return (100.0 * EDGE_ILL_CONDITIONED.get(si_id(entry), 0.0) <= tolerances(entry[2])[0]
            and not (c["strategy"] == "lm" and c["solver"] in EDGE_INEXACT_SOLVERS))


def si_limits(entry):
    """test_gpu_frontend_matrix.limits, its edge-scene value checks decided by THIS table, as test_gpu_fixed_intrinsics.fi_limits."""
    lim = limits(entry[2])
    values = ("cost", "radius", "final_cost", "state")
    for k in values:
        lim.pop("edge_" + k, None)
    if edge_values_compared(entry):
        for k in values:
            lim["edge_" + k] = lim[k]
    lim.pop("tukey_rows", None)
    lim.pop("inner_steps", None)
    lim.pop("edge_inner_steps", None)
    for pre in ("", "edge_"):
        lim[pre + "constant_poses_changed"] = 0
        lim[pre + "groups_differ"] = 0
    return lim


# the edge scene's seed: with test_gpu_frontend_matrix's own (11) the traditional dogleg with a group per camera moves by 1.2e-6 under
# the noise — the single-observation camera's block, as there; of seeds 12 .. 17, 15 leaves every dogleg case below 3e-9
EDGE_SEED, CLEAN_SEED = 15, 5
_scenes = {}


def scenes(oracle):
    """{"clean", "edge"}: test_gpu_frontend_matrix's scenes, made once per session."""
    if not _scenes:
        _scenes["clean"] = clean_scene(oracle, seed=CLEAN_SEED)
        _scenes["edge"] = edge_scene(oracle, seed=EDGE_SEED)
    return _scenes


def ambient_state(sc):
    """[points | cameras] of a scene's BAL-order parameters."""
    nc = sc[0]
    return np.concatenate([sc[-1][9 * nc:], sc[-1][:9 * nc]])


def shared_scene(oracle, sc, groups):
    """The scene as cameras that share intrinsics see it: (scene with every pixel moved by what the group's intrinsics move its
    projection at the initial state, ambient x0 with the groups' intrinsics shared).  The residuals at x0 are then the original
    scene's own — its outliers, its far point, its initial cost — and the data fit the model: one physical camera per group.  Left as
    generated, every camera's pixels would be those of its own focal length (800 .. 1180 here) under a shared one: a large-residual
    problem whose first steps Ceres' CG rule (the Q test at eta = 1e-12) ends 1.4e-6 (one group) to 9.5e-6 (two) in cost away from the
    exact solve the restatement takes — measured with the restatement's solve replaced by that CG, and on the device; as made here
    1.1e-7 and 2.0e-7, and 4.9e-7 with a group per camera, which is the matrix scene itself (design/27_shared_intrinsics.md)."""
    nc, npts, cam, pt, obs, par = sc
    x_own = ambient_state(sc)
    x0 = SI.share(x_own, nc, npts, groups)
    zero = np.zeros((cam.shape[0], 2))
    project = lambda x: oracle.snavely_batch(x[3 * npts:].reshape(nc, 9)[cam], x[:3 * npts].reshape(npts, 3)[pt], zero)[0]
    moved = np.asarray(obs, dtype=np.float64).reshape(-1, 2) + (project(x0) - project(x_own))
    return (nc, npts, cam, pt, moved, np.concatenate([x0[3 * npts:], x0[:3 * npts]])), x0


def reference(oracle, sc, layout, constant, loss, as_generated=False):
    """(restatement, ambient x0 with the groups' intrinsics shared, compact x0, groups, constant cameras); the restatement's `scene`
    is what the device problem is made of (shared_scene; as_generated: the scene's own pixels under the shared intrinsics — the
    large-residual problem shared_scene describes, for the exact solver)."""
    groups = SI.layout(layout, sc[0])
    const = SI.constant_cameras(constant, groups)
    scene, x0 = shared_scene(oracle, sc, groups)
    if as_generated:
        scene = scene[:4] + (np.asarray(sc[4], dtype=np.float64).reshape(-1, 2),) + scene[5:]
    nc, npts, cam, pt, obs, _ = scene
    inner = F.problem(oracle.snavely_batch, 0, nc, npts, cam, pt, obs, np.argsort(pt, kind="stable"), loss)
    w = SI.Problem(inner, nc, npts, groups, const, x0)
    w.scene = scene
    return w, x0, w.compact(x0), groups, const
