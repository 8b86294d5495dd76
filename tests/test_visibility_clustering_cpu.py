"""The host analysis of CLUSTER_JACOBI (csrc/visibility.cc through ceres_hip_debug_cluster_cameras) against the Python restatement
(tests/visibility_reference.py): no GPU.  The restatement is first held to the known answers of the clustering unit tests the project is
modelled on (tests/golden/visibility_known_answers.json); the export must then equal it exactly — same partition, same numbering — on
every structure below, for both clustering types.  Conditions on the inputs are asserted on the RESTATEMENT's output, so that a
degenerate case cannot pass for a real one."""
import functools
import json
import os

import numpy as np
import pytest

import schur_dense_reference as R
import visibility_reference as V
from conftest import ROOT, pkg

P = pkg.problems
hs = pkg.hip_solver
TYPES = (V.CANONICAL_VIEWS, V.SINGLE_LINKAGE)


def known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "visibility_known_answers.json")) as f:
        return json.load(f)


# ---- the restatement against the reference's own unit tests ------------------------------------------------------------------------
@pytest.mark.parametrize("case", known_answers()["canonical_views"]["cases"], ids=lambda c: c["name"])
def test_restatement_canonical_views_known_answers(case):
    g = known_answers()["canonical_views"]
    nb = V.graph_from_edges(g["num_vertices"], g["edges"], self_edges=g["self_edges"])
    weights = [float("nan") if w is None else w for w in g["vertex_weights"]]
    centers, to_center, _ = V.canonical_views(nb, size_penalty=case["size_penalty_weight"], similarity_penalty=case["similarity_penalty_weight"],
                                              min_views=case["min_views"], view_score_weight=case["view_score_weight"], vertex_weights=weights)
    assert centers == case["centers"]
    if case["membership"] is not None:
        assert {str(v): c for v, c in to_center.items()} == case["membership"]


@pytest.mark.parametrize("case", known_answers()["single_linkage"]["cases"], ids=lambda c: c["name"])
def test_restatement_single_linkage_known_answers(case):
    g = known_answers()["single_linkage"]
    nb = V.graph_from_edges(g["num_vertices"], case["edges"])
    root = V.single_linkage(nb, min_similarity=g["min_similarity"])
    assert len(root) == g["num_vertices"]
    for a, b in case["same"]:
        assert root[a] == root[b], (a, b, root)
    for a, b in case["different"]:
        assert root[a] != root[b], (a, b, root)


# ---- the structures ------------------------------------------------------------------------------------------------------------------
def grouped_bal(n_groups=30, g=4, n_points=2500, groups_per_point=3, keep=0.97, seed=3):
    """30 groups of 4 cameras on a ring, every point seen by 3 neighbouring groups, each camera of a group with probability 0.97."""
    rng = np.random.default_rng(seed)
    po, co = [], []
    for pt in range(n_points):
        s = rng.integers(0, n_groups)
        gs = [(s + d) % n_groups for d in range(groups_per_point)]
        cams = [gg * g + k for gg in gs for k in range(g) if rng.random() < keep]
        if len(cams) < 2:
            cams = [gs[0] * g, gs[0] * g + 1]
        cams = sorted(set(cams))
        po += [pt] * len(cams)
        co += cams
    return P._assemble_bal(rng, n_groups * g, n_points, np.array(po, dtype=np.int64), np.array(co, dtype=np.int64), "schur", False)


CASES = {
    "banded": lambda: P.banded_bal(shape=None, num_cameras=120, num_points=3000, num_observations=15000, with_values=False),
    "synthetic": lambda: P.synthetic_bal(shape=None, num_cameras=120, num_points=3000, num_observations=15000, with_values=False),
    "libmv_problem_02": lambda: P.libmv_bal(problem=2, with_values=False),
    "libmv_structured": lambda: P.libmv_structured(problem=2, with_values=False),
    "camera_rows_with_pairs": lambda: P.add_camera_rows(P.banded_bal(shape=None, num_cameras=60, num_points=900, num_observations=4000), 50,
                                                         seed=4, pair_fraction=0.4),
    "random_schur": lambda: P.random_schur_problem(num_e_blocks=40, num_f_blocks=12, seed=5),
    "grouped": grouped_bal,
    "unobserved_cameras": lambda: R.build_case(P, "track64_239"),   # 500 cameras, most of them see nothing
}


@functools.lru_cache(maxsize=None)
def analysed(name, ctype):
    p = CASES[name]()
    nelim = int(p.num_eliminate_blocks)
    want, n_want, ties = V.cluster_cameras(p.bs, nelim, ctype, return_ties=True)
    got, n_got = hs.debug_cluster_cameras(p.bs, nelim, ctype)
    return p, want, n_want, ties, np.array(got), n_got


@pytest.mark.parametrize("ctype", TYPES, ids=["canonical_views", "single_linkage"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_export_equals_the_restatement(name, ctype):
    p, want, n_want, _, got, n_got = analysed(name, ctype)
    nf = int(p.bs.num_col_blocks) - int(p.num_eliminate_blocks)
    assert got.shape == (nf,) and want.shape == (nf,)
    assert n_got == n_want, (name, ctype, n_got, n_want)
    assert np.array_equal(got, want), (name, ctype, np.flatnonzero(got != want)[:10])
    # numbering: clusters by ascending first member, all ids used
    firsts = [int(np.flatnonzero(got == k)[0]) for k in range(n_got)]
    assert firsts == sorted(firsts)


def test_unobserved_cameras_are_in_the_case():
    p = CASES["unobserved_cameras"]()
    vis = V.visibility(p.bs, int(p.num_eliminate_blocks))
    assert sum(1 for s in vis if not s) >= 250


def test_conditions_on_the_inputs():
    """Asserted on the restatement: a non-trivial clustering per type, tied scores, one single cluster, only singletons."""
    sizes = lambda m: np.bincount(m)
    for ctype, names in ((V.CANONICAL_VIEWS, ("banded", "grouped")), (V.SINGLE_LINKAGE, ("grouped",))):
        for name in names:
            p, want, n, _, _, _ = analysed(name, ctype)
            nf = int(p.bs.num_col_blocks) - int(p.num_eliminate_blocks)
            assert 1 < n < nf and sizes(want).max() >= 3, (name, ctype, n, sizes(want).max())
    # the grouped scene: 30 clusters of 4 under single linkage, fewer and larger ones under canonical views
    _, want, n, _, _, _ = analysed("grouped", V.SINGLE_LINKAGE)
    assert n == 30 and (sizes(want) == 4).all()
    _, want, n, _, _, _ = analysed("grouped", V.CANONICAL_VIEWS)
    assert n < 30 and sizes(want).max() > 4
    # tied scores happen (the pinned order decides them)
    assert analysed("libmv_problem_02", V.CANONICAL_VIEWS)[3] > 0
    # one cluster of everything; only singletons
    p, want, n, _, _, _ = analysed("libmv_problem_02", V.SINGLE_LINKAGE)
    assert n == 1 and want.shape[0] > 100
    p, want, n, _, _, _ = analysed("synthetic", V.SINGLE_LINKAGE)
    assert n == want.shape[0] == 120


def test_block_pairs_stay_inside_clusters():
    """The restatement's block pairs (ComputeBlockPairsInPreconditioner): every (i, i), nothing across clusters, and on a structure with
    pair rows an off-diagonal pair that comes from an E-free row alone."""
    p, want, _, _, _, _ = analysed("camera_rows_with_pairs", V.CANONICAL_VIEWS)
    nelim = int(p.num_eliminate_blocks)
    pairs = V.block_pairs(p.bs, nelim, want)
    nf = int(p.bs.num_col_blocks) - nelim
    assert all((i, i) in set(pairs) for i in range(nf))
    assert all(want[i] == want[j] and i <= j for i, j in pairs)
    assert any(i != j for i, j in pairs)


# ---- option validation that needs no device -----------------------------------------------------------------------------------------
def _create(**kw):
    return hs.HipLinearSolver(hs.LinearSolverOptions(max_num_iterations=5, elimination_groups=[3], **kw))


def test_option_validation_before_device():
    assert (hs.CLUSTER_JACOBI, hs.CANONICAL_VIEWS, hs.SINGLE_LINKAGE) == (4, 0, 1)
    with pytest.raises(hs.HipError) as e:   # CGNR: refused as SCHUR_JACOBI is
        _create(type=hs.CGNR, preconditioner_type=hs.CLUSTER_JACOBI)
    assert "preconditioner_type 4 is not available for solver_type 6" in str(e.value)
    with pytest.raises(hs.HipError) as e:   # the reference CHECKs SCHUR_JACOBI there
        _create(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.CLUSTER_JACOBI, use_explicit_schur_complement=True)
    assert "Only SCHUR_JACOBI is supported with use_explicit_schur_complement" in str(e.value)
    with pytest.raises(hs.HipError) as e:
        _create(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.CLUSTER_JACOBI, visibility_clustering_type=2)
    assert "visibility_clustering_type 2" in str(e.value)
    with pytest.raises(hs.HipError) as e:   # CLUSTER_TRIDIAGONAL: still refused, with the message it always had
        _create(type=hs.ITERATIVE_SCHUR, preconditioner_type=5)
    assert "preconditioner_type 5 is not available for solver_type 5" in str(e.value)
    # the clustering type is ignored by the other preconditioners: the option is accepted and the call gets as far as the device
    if hs.device_count() == 0:
        with pytest.raises(hs.HipError) as e:
            _create(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI, visibility_clustering_type=2)
        assert "no HIP device" in str(e.value) or "no CPU fallback" in str(e.value)


def test_debug_export_refuses_bad_arguments():
    p = CASES["random_schur"]()
    with pytest.raises(hs.HipError):
        hs.debug_cluster_cameras(p.bs, int(p.num_eliminate_blocks), 2)
    with pytest.raises(hs.HipError):
        hs.debug_cluster_cameras(p.bs, 0, V.CANONICAL_VIEWS)
