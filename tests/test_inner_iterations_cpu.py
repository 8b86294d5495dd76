"""Inner iterations of the BAL front end, host side: ceres_hip_debug_inner_iteration_ordering (what a handle runs) against the numpy
restatement of CoordinateDescentMinimizer::CreateOrdering (tests/inner_reference.py), argument validation without a device, and
self-checks of the restatement's per-block loop."""
import numpy as np
import pytest

import inner_reference as IR
import robust_reference as R
from conftest import pkg


@pytest.fixture(scope="module")
def hip():
    """The binding without a device (the ordering is pure host code; the handle-less entry points only validate)."""
    hs = pkg.hip_solver
    hs.load_library()
    return hs


def random_structure(rng, nc, npts, nobs):
    cam = rng.integers(0, nc, nobs).astype(np.int32)
    pt = np.concatenate([np.arange(npts), rng.integers(0, npts, nobs - npts)]).astype(np.int32)   # every point observed
    return cam, pt


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("blocks", IR.KINDS)
def test_ordering_matches_the_restatement(hip, seed, blocks):
    rng = np.random.default_rng(seed)
    nc, npts = int(rng.integers(2, 12)), int(rng.integers(5, 60))
    cam, pt = random_structure(rng, nc, npts, int(rng.integers(npts, 4 * npts)))
    g, ng = hip.inner_iteration_ordering(nc, npts, cam, pt, blocks)
    gr, ngr = IR.ordering(nc, npts, cam, pt, blocks)
    assert ng == ngr and np.array_equal(g, gr), (ng, ngr)
    for k in range(ng):   # every group is an independent set: no observation joins two of its blocks
        assert not np.any((g[pt] == k) & (g[npts + cam] == k))


def test_ordering_of_bal_data_is_cameras_then_points(hip):
    rng = np.random.default_rng(3)
    nc, npts = 8, 400
    cam, pt = random_structure(rng, nc, npts, 2000)
    g, ng = hip.inner_iteration_ordering(nc, npts, cam, pt, "automatic")
    assert ng == 2 and np.all(g[npts:] == 0) and np.all(g[:npts] == 1)


def test_ordering_with_ties_and_low_degree_cameras(hip):
    # camera 0 sees one point (degree 1, lower than that point's 3 cameras): it is taken in the first set with the points it does not
    # touch — mixed groups; and a ring of equal degrees (every vertex degree 2): ties broken by position
    cam = np.array([0, 1, 2, 3, 1, 2, 3, 1, 3], dtype=np.int32)
    pt = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int32)
    for nc, npts, c, p in ((4, 4, cam, pt), (3, 3, np.array([0, 1, 1, 2, 2, 0], np.int32), np.array([0, 0, 1, 1, 2, 2], np.int32))):
        g, ng = hip.inner_iteration_ordering(nc, npts, c, p, "automatic")
        gr, ngr = IR.ordering(nc, npts, c, p, "automatic")
        assert ng == ngr and np.array_equal(g, gr)
    g, ng = hip.inner_iteration_ordering(4, 4, cam, pt, "automatic")
    assert len(set(g[:4]) | set(g[4:])) == ng and set(g[:4]) & set(g[4:]), g   # some group holds points and cameras


def test_explicit_kinds(hip):
    cam, pt = random_structure(np.random.default_rng(1), 5, 30, 90)
    expect = {"cameras": ([-1] * 30 + [0] * 5, 1), "points": ([0] * 30 + [-1] * 5, 1), "cameras,points": ([1] * 30 + [0] * 5, 2),
              "points,cameras": ([0] * 30 + [1] * 5, 2)}
    for kind, (grp, ng) in expect.items():
        g, n = hip.inner_iteration_ordering(5, 30, cam, pt, kind)
        assert n == ng and list(g) == grp, kind


def test_ordering_argument_validation(hip):
    lib = hip.load_library()
    cam, pt = random_structure(np.random.default_rng(2), 3, 10, 20)
    for blocks in (0, 6, -1):
        with pytest.raises(hip.HipError):
            hip.inner_iteration_ordering(3, 10, cam, pt, blocks)
    with pytest.raises(hip.HipError):
        hip.inner_iteration_ordering(3, 5, cam, pt, "automatic")   # point index out of range
    assert lib.ceres_hip_debug_inner_iteration_ordering(0, 0, 0, None, None, 1, None, None) != 0
    for name in ("ceres_hip_bal_set_inner_iterations", "ceres_hip_bal_inner_iterate", "ceres_hip_bal_inner_iteration_stats"):
        assert name in [a[0] for a in hip.ABI]
    assert lib.ceres_hip_bal_set_inner_iterations(None, 1, 1e-3) == -1
    assert b"NULL" in lib.ceres_hip_bal_last_error(None)
    assert lib.ceres_hip_bal_inner_iterate(None, None, None, None, None) != 0
    assert lib.ceres_hip_bal_inner_iteration_stats(None, None, None, None) != 0


@pytest.mark.parametrize("loss", [None, ("huber", 1.0, 1.0, 1.0), ("cauchy", 2.0, 1.0, 1.0)])
def test_restatement_pass_never_raises_a_blocks_cost(oracle, loss):
    op = oracle.BalProblem.generate(6, 120, 600, seed=4)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    x0 = op.state()
    ev = R.Evaluator(oracle.snavely_batch, op.num_cameras, op.num_points, cam, pt, obs, np.argsort(pt, kind="stable"), loss=loss)
    g, ng = IR.ordering(op.num_cameras, op.num_points, cam, pt, "automatic")
    x = x0.copy()
    for gi in range(ng):
        for cameras in (False, True):
            sel = np.flatnonzero(g[op.num_points:] == gi) if cameras else np.flatnonzero(g[:op.num_points] == gi)
            if sel.size == 0:
                continue
            grp = IR._Group(ev, cameras, sel)
            before = grp.evaluate(x, grp.get(x), False)[0]
            P, its = IR.solve_group(grp, x)
            after = grp.evaluate(x, P, False)[0]
            assert np.all(after <= before) and np.all(its >= 0)
            grp.put(x, P, np.ones(sel.size, bool))
    assert ev.cost(x) < ev.cost(x0)


def test_restatement_exact_point_takes_no_step(oracle):
    """A point whose observations the state reproduces exactly: zero residuals, zero gradient — the gradient test ends its loop before
    its first iteration."""
    op = oracle.BalProblem.generate(4, 30, 120, seed=9, pixel_noise=0.0)
    op.build_structure(True)
    cam, pt, _ = op.indices()
    x0 = op.state()
    order = np.argsort(pt, kind="stable")
    cams = x0[3 * op.num_points:].reshape(-1, 9)[cam]
    pts = x0[:3 * op.num_points].reshape(-1, 3)[pt]
    r, _, _ = oracle.snavely_batch(cams, pts, np.zeros((cam.shape[0], 2)))
    obs = r.copy()   # the projections themselves: every residual zero
    ev = R.Evaluator(oracle.snavely_batch, op.num_cameras, op.num_points, cam, pt, obs, order)
    grp = IR._Group(ev, False, np.arange(op.num_points))
    P, its = IR.solve_group(grp, x0)
    assert np.all(its == 0) and np.array_equal(P, grp.get(x0))
