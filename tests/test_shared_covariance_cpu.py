"""The reference of tests/test_gpu_shared_covariance.py held to things that do not depend on the device: the two routes of
tests/covariance_reference.py against each other on the shared-intrinsics restatement's Jacobian, the conditions the cases of
tests/shared_covariance_cases.py must meet for the rank rule (min_scaled_pivot = 1e-8, design/17_covariance.md §17.2) to be a property of
the inputs, what the pair lists cover, and the restatement against covariance_cases' 9-wide camera blocks with a group per camera.
numpy only: nothing here calls the library."""
import numpy as np
import pytest

import covariance_cases as CC
import covariance_reference as CR
import shared_covariance_cases as SC
import shared_intrinsics_reference as SI
from conftest import pkg


@pytest.mark.parametrize("name", SC.SUCCESS)
def test_the_routes_agree_and_the_pivots_are_large(oracle, name):
    """Routes (a) and (b) agree on every requested block; the smallest scaled pivots of a success case are at least 100 x above the
    default limit 1e-8; a pair with a constant pose is zeros and every block has its kind's shape."""
    c = SC.case(oracle, name)
    layout, J, a, b = SC.reference_results(oracle, name)
    assert J.shape[1] == layout.n and layout.n_f == SC.SIZES[name]
    print(f"{name}: n = {layout.n_f}, min_point_pivot = {b['min_point_pivot']:.3e}, min_schur_pivot = {b['min_schur_pivot']:.3e}")
    assert b["cov"] is not None
    assert min(b["min_point_pivot"], b["min_schur_pivot"]) >= 100.0 * 1e-8
    scales = layout.scales(np.diag(a), c.pairs)
    dev = CR.correlation_deviation(layout.blocks(b["cov"], c.pairs), layout.blocks(a, c.pairs), scales)
    print(f"{name}: route (a) against route (b): {dev:.3e}")
    # float64 on unit-diagonal matrices: n eps / pivot = 1e3 x 2.2e-16 / 1e-6 = 2e-7 at the very worst; test_covariance_cpu's own
    # limit, 2e-9, holds on these scenes (their pivots are above 1e-3) and is kept
    assert dev <= 2e-9, dev
    for (p, q), blk in zip(c.pairs, layout.blocks(b["cov"], c.pairs)):
        if layout.columns(int(p)) is None or layout.columns(int(q)) is None:
            assert not blk.any()
        assert blk.shape == (layout.size(int(p)), layout.size(int(q)))


@pytest.mark.parametrize("name", SC.FAILURE)
def test_failure_cases_have_vanishing_pivots(oracle, name):
    """A free gauge: the smallest pivot of the scaled Schur complement is at least 100 x below the limit, or not positive; the point
    stage is sound."""
    c = SC.case(oracle, name)
    layout, J, a, b = SC.reference_results(oracle, name)
    print(f"{name}: n = {layout.n_f}, min_point_pivot = {b['min_point_pivot']:.3e}, min_schur_pivot = {b['min_schur_pivot']:.3e}")
    assert c.stage == "Schur" and b["cov"] is None
    assert b["min_point_pivot"] >= 100.0 * 1e-8 and b["min_schur_pivot"] <= 1e-8 / 100.0


def test_scene_shapes(oracle):
    """The sizes the cases exist for, scene C's tracks, the groups whose cameras are all constant, the generic-kernel grouping."""
    for name, n in SC.SIZES.items():
        c = SC.case(oracle, name)
        free = c.nc - len(c.constant)
        assert 6 * free + 3 * (int(c.groups.max()) + 1) == n, name
    c = SC.case(oracle, "C-two-huber")
    counts = np.bincount(c.scene[3], minlength=c.npts)
    assert [int(counts[q]) for q in SC.TRACKS] == [32, 33, 64, 65, 2] and c.loss == CC.HUBER
    assert c.constant.tolist() == [0, 2]
    e = SC.case(oracle, "B-each")
    assert e.constant.tolist() == [0, 1] and np.array_equal(e.groups, np.arange(32))   # groups 0 and 1: constant poses only
    assert np.any(np.isin(e.scene[2], [0, 1]))                                          # rows with a group cell and no pose cell
    t = SC.case(oracle, "B-three")
    assert int(t.groups.max()) + 1 == 3 and t.constant.tolist() == [0, 3]
    s = SC.case(oracle, "A-two_single")
    assert int(np.sum(s.groups == 1)) == 1
    a = SC.case(oracle, "A-one")
    assert len(a.pairs) == (40 + 8 + 1) ** 2


@pytest.mark.parametrize("name", SC.SUCCESS)
def test_the_pairs_cover_every_kind(oracle, name):
    """Group-group own (and cross where there are two groups); pose-group with the pose in and, with two groups, out of the group;
    point-group; point-pose seen and unseen; point-point p != q; transposed and repeated pairs; pairs with a constant pose; a point a
    constant pose sees; and, where the scene has them, two points that meet in a group only."""
    c = SC.case(oracle, name)
    nc, npts, cam, pt = c.scene[0], c.scene[1], c.scene[2], c.scene[3]
    ng = int(c.groups.max()) + 1
    kind = lambda b: "point" if b < npts else "pose" if b < npts + nc else "group"
    pairs = [tuple(p) for p in c.pairs.tolist()]
    have = set(pairs)
    kinds = {(kind(a), kind(b)) for a, b in pairs}
    assert kinds == {(u, v) for u in ("point", "pose", "group") for v in ("point", "pose", "group")}
    const = set(c.constant.tolist())
    G = lambda g: npts + nc + g
    assert all((G(g), G(g)) in have for g in range(ng))
    assert ng == 1 or any(a != b for a, b in pairs if kind(a) == kind(b) == "group")
    in_group = [(a, b) for a, b in pairs if kind(a) == "pose" and kind(b) == "group" and a - npts not in const and c.groups[a - npts] == b - npts - nc]
    out_group = [(a, b) for a, b in pairs if kind(a) == "pose" and kind(b) == "group" and c.groups[a - npts] != b - npts - nc]
    assert in_group and (ng == 1 or out_group)
    sees = lambda q, cm: bool(np.any((pt == q) & (cam == cm)))
    pp = [(a, b) for a, b in pairs if kind(a) == "point" and kind(b) == "pose" and b - npts not in const]
    assert any(sees(a, b - npts) for a, b in pp) and any(not sees(a, b - npts) for a, b in pp)
    assert any(a != b for a, b in pairs if kind(a) == kind(b) == "point")
    assert any((b, a) in have for a, b in pairs if a != b) and (len(have) < len(pairs) or name == "A-one")
    assert any(kind(a) == "pose" and a - npts in const for a, b in pairs) and any(kind(b) == "pose" and b - npts in const for a, b in pairs)
    by_const = set(pt[np.isin(cam, list(const))].tolist())
    assert any(a in by_const and a == b for a, b in pairs if kind(a) == "point")
    through = SC.points_through_the_group(c.scene, c.groups)
    assert (through is None) == (name == "B-each")   # (a group per camera: two points meet in a group only through a camera)
    if through is not None:
        p, q = through
        assert (p, q) in have and (q, p) in have
        assert not set(cam[pt == p].tolist()) & set(cam[pt == q].tolist())


def test_round_boundaries_of_the_blocks_pass(oracle):
    """Scene C's point pairs put the lanes' rounds of 64 row pairs on both sides of a boundary: 65^2 = 66 full rounds and one lane, 64^2
    exactly 64 rounds, 2 x 65 two rounds and two lanes; EVERY row of a point counts, the rows of the constant poses too."""
    c = SC.case(oracle, "C-two-huber")
    counts = np.bincount(c.scene[3], minlength=c.npts)
    pairs = {tuple(p) for p in c.pairs.tolist()}
    own = {int(counts[q]) ** 2 for q in SC.TRACKS if (q, q) in pairs}
    assert {65 * 65, 64 * 64, 33 * 33, 32 * 32, 4} <= own
    assert (65 * 65) % 64 == 1 and (64 * 64) % 64 == 0
    cross = {int(counts[a]) * int(counts[b]) for a, b in pairs if a != b and a < c.npts and b < c.npts}
    assert 64 * 65 in cross and 2 * 32 in cross


def test_a_group_per_camera_is_the_nine_wide_camera(oracle):
    """With a group per camera the program's columns are those of covariance_cases' A-cameras01 (cameras 0 and 1 constant, nine columns
    per free camera) after a permutation, beside the intrinsics of cameras 0 and 1, which stay free here (a constant camera is a
    constant POSE).  The Jacobians agree column for column, and route (a) of this reference, CONDITIONED on those six columns
    (Cov_kk - Cov_kx Cov_xx^-1 Cov_xk), is route (a) of covariance_cases: pose and group blocks are the rows and columns 0 .. 5 and
    6 .. 8 of the 9-wide camera blocks — to the routes' own deviation."""
    hs = pkg.hip_solver
    nine = CC.case(oracle, "A-cameras01")
    lay9, J9, a9, _ = CC.reference_results(oracle, hs, "A-cameras01")
    A = nine.scene
    each = SC.Case("A-each", A, "each", [0, 1], None, [(0, 0)], True)
    assert np.array_equal(each.state(), nine.state(hs))   # (sharing within groups of one camera changes nothing)
    lay, J = each.reference(oracle)
    npts, nc = each.npts, each.nc
    # column of this program for every column of the nine-wide one: points, then per free camera its pose and its group
    perm = list(range(3 * npts))
    for cam in range(nc):
        if lay9.columns(npts + cam) is None:
            continue
        perm += lay.columns(npts + cam).tolist() + lay.columns(npts + nc + cam).tolist()
    perm = np.array(perm)
    extra = np.concatenate([lay.columns(npts + nc + cam) for cam in (0, 1)])
    assert sorted(perm.tolist() + extra.tolist()) == list(range(lay.n)) and perm.size == lay9.n
    assert np.array_equal(J[:, perm], J9)
    a = CR.dense_covariance(J)
    cond = a[np.ix_(perm, perm)] - a[np.ix_(perm, extra)] @ np.linalg.solve(a[np.ix_(extra, extra)], a[np.ix_(extra, perm)])
    scale = np.sqrt(np.outer(np.diag(a9), np.diag(a9)))
    dev = float(np.max(np.abs(cond - a9) / scale))
    own = float(np.max(np.abs(CR.schur_covariance(J9, lay9.e_sizes())["cov"] - a9) / scale))
    print(f"conditioned route (a) against covariance_cases' route (a): {dev:.3e}; its own routes: {own:.3e}")
    assert dev <= 2e-9, dev
    # without conditioning the blocks differ visibly: the intrinsics of cameras 0 and 1 are uncertain here
    assert float(np.max(np.abs(a[np.ix_(perm, perm)] - a9) / scale)) > 1e-3


def test_numbering_of_the_reference_layout(oracle):
    """Point q is q, the pose of camera c is num_points + c (6), group g is num_points + num_cameras + g (3); a constant pose has no
    columns, its group has."""
    c = SC.case(oracle, "B-three")
    lay = SC.reference_results(oracle, c.name)[0]
    npts, nc = c.npts, c.nc
    assert lay.num_blocks == npts + nc + 3 and lay.n == 3 * npts + 6 * (nc - 2) + 9
    assert [lay.size(b) for b in (0, npts - 1, npts, npts + nc - 1, npts + nc, npts + nc + 2)] == [3, 3, 6, 6, 3, 3]
    assert lay.columns(npts + 0) is None and lay.columns(npts + 3) is None and lay.columns(npts + 1)[0] == 3 * npts
    assert lay.columns(npts + nc)[0] == 3 * npts + 6 * (nc - 2) and lay.columns(npts + nc + 2)[-1] == lay.n - 1
    w = c.restatement(oracle)
    assert w.n == lay.n and np.array_equal(w.ccol, lay.ccol)
    assert w.groups_identical(c.state()) and np.array_equal(SI.share(c.state(), nc, npts, c.groups), c.state())
