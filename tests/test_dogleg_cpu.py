"""Dogleg trust region of the BAL front end, host side: ceres_hip_debug_dogleg_subspace_minimum (the subspace boundary minimum the
strategy runs) against the numpy restatement (tests/dogleg_reference.py), argument validation without a device, and self-checks of the
restatement's strategy."""
import numpy as np
import pytest

import dogleg_reference as DR
from conftest import pkg


@pytest.fixture(scope="module")
def hip():
    """The binding without a device (the boundary minimum is pure host code; the handle-less entry points only validate)."""
    hs = pkg.hip_solver
    hs.load_library()
    return hs


def random_model(rng, kind):
    """A 2x2 SPD (or near-singular) B, g and a radius that puts the Newton point outside the trust region."""
    Q, _ = np.linalg.qr(rng.standard_normal((2, 2)))
    if kind == "spd":
        ev = np.exp(rng.uniform(-3, 3, 2))
    elif kind == "near_singular":
        ev = np.array([np.exp(rng.uniform(-1, 2)), 10.0 ** rng.uniform(-8, -5)])
    else:   # indefinite: the first-order check may fail, or the roots may be all complex
        ev = np.array([np.exp(rng.uniform(-1, 2)), -np.exp(rng.uniform(-3, 1))])
    B = Q @ np.diag(ev) @ Q.T
    B = 0.5 * (B + B.T)
    g = rng.standard_normal(2) * np.exp(rng.uniform(-2, 2))
    newton = np.linalg.norm(np.linalg.lstsq(B, g, rcond=None)[0])
    # (near-singular: on the scale of the gradient step, far inside the Newton point, as a trust region is while it matters)
    scale = newton if kind == "spd" else min(newton, np.linalg.norm(g) / ev.max() * np.exp(rng.uniform(-2, 3)))
    radius = scale * rng.uniform(0.02, 0.98)
    return B, g, radius


def boundary_value(B, g, radius, x):
    xb = radius * x / np.linalg.norm(x)
    return 0.5 * xb @ B @ xb + g @ xb


@pytest.mark.parametrize("kind", ["spd", "near_singular", "indefinite"])
def test_subspace_minimum_matches_the_restatement(hip, kind):
    rng = np.random.default_rng({"spd": 1, "near_singular": 2, "indefinite": 3}[kind])
    codes = []
    for _ in range(150):
        B, g, radius = random_model(rng, kind)
        code_ref, x_ref = DR.boundary_minimum(B, g, radius)
        code, x = hip.dogleg_subspace_minimum(B, g, radius)
        codes.append(code_ref)
        assert code == code_ref, (B, g, radius, x, x_ref)
        if code_ref != 1:
            # the model's value on the boundary agrees to 1e-10 everywhere; the minimiser itself where B + yI is well conditioned at the
            # root (a nearly singular B puts the root next to -lambda_min, where any two root finders' last digits are amplified)
            f, f_ref = boundary_value(B, g, radius, x), boundary_value(B, g, radius, x_ref)
            assert abs(f - f_ref) <= 1e-10 * abs(f_ref), (B, g, radius, x, x_ref)
            tol = 1e-10 if kind == "spd" else 1e-8
            assert np.linalg.norm(x - x_ref) <= tol * np.linalg.norm(x_ref), (B, g, radius, x, x_ref)
        else:
            assert np.all(x == 0.0)
    if kind != "indefinite":
        assert codes.count(0) >= 140   # (positive definite models: the boundary minimum is found)


def test_fallback_cases_are_reported(hip):
    # g = 0 with B = I: every root gives x = 0, so no root is usable
    code, x = hip.dogleg_subspace_minimum(np.eye(2), np.zeros(2), 1.0)
    assert code == hip.DOGLEG_NO_ROOT and np.all(x == 0)
    assert DR.boundary_minimum(np.eye(2), np.zeros(2), 1.0)[0] == 1
    # a coefficient that is not finite: no roots
    code, _ = hip.dogleg_subspace_minimum(np.array([[np.inf, 0], [0, 1.0]]), np.ones(2), 1.0)
    assert code == hip.DOGLEG_NO_ROOT
    # an indefinite model whose best root violates first-order optimality somewhere in a sweep: the cosine fallback happens
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        B, g, radius = random_model(rng, "indefinite")
        code, _ = hip.dogleg_subspace_minimum(B, g, radius)
        assert code == DR.boundary_minimum(B, g, radius)[0]
        seen.add(code)
    assert 0 in seen


def test_subspace_minimum_beats_a_boundary_sweep():
    rng = np.random.default_rng(7)
    t = np.linspace(0, 2 * np.pi, 3600, endpoint=False)
    for _ in range(50):
        B, g, radius = random_model(rng, "spd")
        code, x = DR.boundary_minimum(B, g, radius)
        assert code == 0
        xb = radius * x / np.linalg.norm(x)
        best = 0.5 * xb @ B @ xb + g @ xb
        pts = radius * np.stack([np.cos(t), np.sin(t)], axis=1)
        sweep = 0.5 * np.einsum("ni,ij,nj->n", pts, B, pts) + pts @ g
        assert best <= sweep.min() + 1e-12 * max(1.0, abs(sweep.min()))


def strategy_on(rng, kind, radius, m=30, n=8):
    J = rng.standard_normal((m, n)) * np.exp(rng.uniform(-1, 1, n))
    r = rng.standard_normal(m)
    s = DR.Strategy(kind, radius, 1e-6, 1e32)
    return s, J, r


def test_traditional_step_has_the_radius_on_the_dogleg_and_cauchy_branches():
    rng = np.random.default_rng(11)
    seen = set()
    _, J, r = strategy_on(rng, "traditional", 1.0)
    for radius in np.geomspace(1e-4, 1e2, 40):
        s = DR.Strategy("traditional", radius, 1e-6, 1e32)
        status, step, solves, _ = s.compute_step(J, r)
        assert status == "ok" and solves == 1
        seen.add(s.branch)
        scaled = np.linalg.norm(step * s.diagonal)
        if s.branch == "gauss_newton":
            assert scaled <= radius * (1 + 1e-12)
        else:
            assert scaled == pytest.approx(radius, rel=1e-10)
            assert s.step_norm == pytest.approx(radius, rel=1e-10)
    assert {"gauss_newton", "cauchy"} <= seen and any(b.startswith("dogleg_c") for b in seen)


def test_subspace_step_is_no_worse_than_the_traditional_one():
    rng = np.random.default_rng(13)
    for radius in np.geomspace(1e-3, 1e1, 20):
        st, J, r = strategy_on(rng, "subspace", radius)
        tr = DR.Strategy("traditional", radius, 1e-6, 1e32)
        _, s1, _, _ = st.compute_step(J, r)
        _, s2, _, _ = tr.compute_step(J, r)
        model = lambda s: -(J @ s) @ (r + J @ s / 2)   # noqa: E731  (the model cost change: larger is better)
        assert model(s1) >= model(s2) - 1e-10 * abs(model(s2))


def test_reused_step_runs_no_solve_and_keeps_the_vectors():
    rng = np.random.default_rng(17)
    s, J, r = strategy_on(rng, "traditional", 1e-2)
    _, a, solves, lsi = s.compute_step(J, r)
    assert solves == 1 and lsi == 1
    s.rejected()
    _, b, solves, lsi = s.compute_step(J, r)
    assert solves == 0 and lsi == 0
    assert np.linalg.norm(b * s.diagonal) == pytest.approx(0.5e-2, rel=1e-10)
    s.invalid()
    assert not s.reuse and s.radius == 0.5e-2 and s.mu == pytest.approx(1e-7)


def test_mu_retry_sequence_stops_at_one():
    rng = np.random.default_rng(19)
    s, J, r = strategy_on(rng, "traditional", 1.0)
    J[:, 3] = np.nan   # every factorisation fails
    status, step, solves, _ = s.compute_step(J, r)
    assert status == "failure" and step is None
    assert solves == 8 and s.mu >= 1.0   # 1e-8, 1e-7, ..., 1e-1
    s.invalid()
    status, _, solves, lsi = s.compute_step(J, r)
    assert status == "failure" and solves == 0 and lsi == 0
    s2, J2, r2 = strategy_on(np.random.default_rng(19), "traditional", 1.0)
    s2.accepted(0.5)
    assert s2.mu == DR.MIN_MU and not s2.reuse


def test_near_parallel_columns_count_as_one_dimensional():
    rng = np.random.default_rng(23)
    g = rng.standard_normal(50)
    for angle, rank in ((0.0, 1), (1e-12, 1), (1e-8, 1), (1e-6, 2), (1e-2, 2)):
        w = rng.standard_normal(50)
        w -= (w @ g) / (g @ g) * g
        gn = -3.0 * (np.cos(angle) * g / np.linalg.norm(g) + np.sin(angle) * w / np.linalg.norm(w))
        assert DR.pivoted_basis(g, gn)[0] == rank, angle
    assert DR.pivoted_basis(np.zeros(5), np.zeros(5))[0] == 0
    # the strategy takes the 1-D step (the gradient truncated to the radius) for such a basis
    J = rng.standard_normal((40, 6))
    r = J @ rng.standard_normal(6)   # consistent: the Gauss-Newton step and the gradient are not parallel in general
    s = DR.Strategy("subspace", 1e-3, 1e-6, 1e32)
    s.compute_step(J, r)
    assert not s.one_dim and s.branch == "subspace_boundary"


def test_argument_validation(hip):
    lib = hip.load_library()
    assert lib.ceres_hip_bal_set_trust_region_strategy(None, hip.DOGLEG, hip.SUBSPACE_DOGLEG) == -1
    assert b"NULL" in lib.ceres_hip_bal_last_error(None)
    assert lib.ceres_hip_debug_dogleg_subspace_minimum(None, None, 1.0, None) == -1
    assert lib.ceres_hip_op_jacobian_gram(None, None, None, None) == -1
