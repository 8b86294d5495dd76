"""The numpy restatement of the robust losses and the Corrector (tests/robust_reference.py) pinned on its own: values at 0, derivatives
against finite differences on every branch, hand-computed values, and the identities the Corrector exists for.  No GPU."""
import numpy as np
import pytest

import robust_reference as R

# (kind, a, b) of the tests below; Tolerant twice (a > 0 and a = 0)
PARAMS = [("trivial", 1.0, 1.0), ("huber", 1.0, 1.0), ("huber", 2.5, 1.0), ("soft_l_one", 1.5, 1.0), ("cauchy", 2.0, 1.0),
          ("arctan", 3.0, 1.0), ("tolerant", 4.0, 1.0), ("tolerant", 0.0, 2.0), ("tukey", 2.0, 1.0)]


@pytest.mark.parametrize("kind,a,b", [p for p in PARAMS if p[0] != "tolerant"])
def test_unscaled_losses_are_the_squared_loss_at_zero(kind, a, b):
    r0, r1, _ = R.rho(kind, np.array([0.0]), a, b)
    assert r0[0] == 0.0 and r1[0] == 1.0


@pytest.mark.parametrize("a,b", [(4.0, 1.0), (0.0, 2.0), (1.0, 0.5)])
def test_tolerant_is_zero_at_zero(a, b):
    # (its slope there is the logistic e^x / (1 + e^x) at x = -a / b, not 1)
    r0, r1, _ = R.rho("tolerant", np.array([0.0]), a, b)
    assert abs(r0[0]) <= 1e-15 * max(1.0, b)
    assert r1[0] == pytest.approx(1.0 / (1.0 + np.exp(a / b)), rel=1e-14)


def central(f, s, h):
    return (f(s + h) - f(s - h)) / (2.0 * h)


@pytest.mark.parametrize("kind,a,b,s", [
    ("huber", 1.0, 1.0, 0.5), ("huber", 1.0, 1.0, 4.0), ("huber", 2.5, 1.0, 3.0), ("huber", 2.5, 1.0, 40.0),
    ("soft_l_one", 1.5, 1.0, 0.3), ("soft_l_one", 1.5, 1.0, 90.0),
    ("cauchy", 2.0, 1.0, 0.7), ("cauchy", 2.0, 1.0, 250.0),
    ("arctan", 3.0, 1.0, 0.4), ("arctan", 3.0, 1.0, 7.0),
    ("tolerant", 4.0, 1.0, 2.0), ("tolerant", 4.0, 1.0, 6.0), ("tolerant", 4.0, 1.0, 30.0), ("tolerant", 4.0, 1.0, 50.0),
    ("tolerant", 0.0, 2.0, 1.0),
    ("tukey", 2.0, 1.0, 1.0), ("tukey", 2.0, 1.0, 3.5), ("tukey", 2.0, 1.0, 9.0),
])
@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_derivatives_against_finite_differences(kind, a, b, s, scale):
    h = 1e-5 * max(1.0, s)
    f = lambda t: R.rho(kind, np.array([t]), a, b, scale)
    d1 = central(lambda t: f(t)[0][0], s, h)
    d2 = central(lambda t: f(t)[1][0], s, h)
    r0, r1, r2 = f(s)
    assert r1[0] == pytest.approx(d1, rel=1e-7, abs=1e-10)
    assert r2[0] == pytest.approx(d2, rel=1e-5, abs=1e-9)
    if kind == "tolerant":   # which side of x = 36.7 (ln 2^53) this is
        x = (s - a) / b
        assert (r2[0] == 0.0) == (x > 36.7)


def test_hand_computed_values():
    r = lambda *args: tuple(v[0] for v in R.rho(*args))
    assert r("huber", np.array([4.0]), 1.0) == (3.0, 0.5, -1.0 / 16.0)
    assert r("huber", np.array([0.25]), 1.0) == (0.25, 1.0, 0.0)
    assert r("cauchy", np.array([1.0]), 1.0) == pytest.approx((np.log(2.0), 0.5, -0.25), rel=1e-15)
    assert r("soft_l_one", np.array([3.0]), 1.0) == pytest.approx((2.0, 0.5, -1.0 / 16.0), rel=1e-15)
    assert r("arctan", np.array([1.0]), 1.0) == pytest.approx((np.pi / 4.0, 0.5, -0.5), rel=1e-15)
    assert r("tukey", np.array([0.5]), 1.0) == pytest.approx((7.0 / 24.0, 0.25, -1.0), rel=1e-15)
    assert r("tukey", np.array([1.5]), 1.0) == pytest.approx((1.0 / 3.0, 0.0, 0.0))
    assert r("trivial", np.array([5.0]), 1.0, 1.0, 3.0) == (15.0, 3.0, 0.0)
    # Tolerant(a, b) = b ln(1 + e^((s - a) / b)) - b ln(1 + e^(-a / b)); far right: s - a - c
    c = 2.0 * np.log(1.0 + np.exp(-1.0))
    assert r("tolerant", np.array([2.0]), 2.0, 2.0)[0] == pytest.approx(2.0 * np.log(2.0) - c, rel=1e-15)
    assert r("tolerant", np.array([100.0]), 2.0, 2.0)[0] == pytest.approx(98.0 - c, rel=1e-15)
    # the rho' floor: Cauchy far out still has a positive slope
    assert R.rho("cauchy", np.array([1e310 / 1e10]), 1e-150)[1][0] >= R.DBL_MIN


def test_no_loss_produces_nan_or_inf():
    s = np.array([0.0, 1e-300, 1e-8, 0.5, 1.0, 4.0, 36.0, 1e4, 1e8, 1e12])
    for kind, a, b in PARAMS:
        for scale in (1.0, 0.25):
            rhos = R.rho(kind, s, a, b, scale)
            assert all(np.all(np.isfinite(v)) for v in rhos), kind
            r = np.sqrt(s)[:, None] * np.array([[0.6, -0.8]])
            J = np.ones((s.shape[0], 2, 12))
            rt, Jt = R.correct(r, J, rhos)
            assert np.all(np.isfinite(rt)) and np.all(np.isfinite(Jt)), kind
    # beyond Tukey's cut-off the block vanishes: rho' = 0 gives zero rows, not 0 / 0
    rt, Jt = R.correct(np.array([[3.0, 4.0]]), np.ones((1, 2, 12)), R.rho("tukey", np.array([25.0]), 2.0))
    assert np.all(rt == 0.0) and np.all(Jt == 0.0)


@pytest.mark.parametrize("kind,a,b", PARAMS)
@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_corrector_identities(kind, a, b, scale):
    """J~^T r~ = rho' J^T r always; J~^T J~ = rho' J^T J + 2 rho'' J^T r r^T J where rho'' > 0 (the Triggs correction), and
    rho' J^T J where the Corrector clamps it (rho'' <= 0: first order only)."""
    rng = np.random.default_rng(11)
    n = 64
    r = rng.standard_normal((n, 2)) * rng.choice([0.3, 1.0, 3.0, 30.0], size=(n, 1))
    J = rng.standard_normal((n, 2, 12))
    s = np.sum(r * r, axis=1)
    rhos = R.rho(kind, s, a, b, scale)
    rt, Jt = R.correct(r, J, rhos)
    g = np.einsum("nkm,nk->nm", Jt, rt)
    assert np.allclose(g, rhos[1][:, None] * np.einsum("nkm,nk->nm", J, r), rtol=1e-12, atol=1e-12)
    H = np.einsum("nkm,nkl->nml", Jt, Jt)
    rtj = np.einsum("nk,nkm->nm", r, J)
    full = rhos[2] > 0.0
    want = rhos[1][:, None, None] * np.einsum("nkm,nkl->nml", J, J) + \
        np.where(full, 2.0 * rhos[2], 0.0)[:, None, None] * np.einsum("nm,nl->nml", rtj, rtj)
    assert np.allclose(H, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    if kind == "tolerant":
        assert full.any()   # the only loss here whose rho'' > 0 (left of x = 36.7): the whole Corrector is reached
    # cost of the corrected linear model near 0 agrees with rho to second order (Triggs): rho(|r + J d|^2) ~ rho + 2 g.d + d^T H d
    d = 1e-4 * rng.standard_normal(12)
    exact = R.rho(kind, np.sum((r + np.einsum("nkm,m->nk", J, d)) ** 2, axis=1), a, b, scale)[0] - rhos[0]
    model = 2.0 * g @ d + np.einsum("m,nml,l->n", d, H, d)
    ok = full | (rhos[2] == 0.0)
    assert np.allclose(exact[ok], model[ok], rtol=1e-4, atol=1e-9)


def test_squared_loss_evaluator_layout():
    """Evaluator lays values out as the solver does: E cells at 6 r, F cells at 6 n_rows + 18 r, rows in the given order."""
    def snavely_linear(cams, pts, obs):   # a stand-in residual that is linear in camera and point: r = A_c cam + B p - obs
        n = cams.shape[0]
        jc = np.broadcast_to(np.arange(18.0).reshape(2, 9) / 10.0, (n, 2, 9)).copy()
        jp = np.broadcast_to(np.arange(6.0).reshape(2, 3) / 7.0 + 1.0, (n, 2, 3)).copy()
        r = np.einsum("nkm,nm->nk", jc, cams) + np.einsum("nkm,nm->nk", jp, pts) - obs
        return r, jc, jp
    rng = np.random.default_rng(2)
    cam = np.array([0, 1, 0, 1, 1], dtype=np.int32)
    pt = np.array([2, 0, 1, 0, 2], dtype=np.int32)
    obs = rng.standard_normal((5, 2))
    order = np.argsort(pt, kind="stable")
    ev = R.Evaluator(snavely_linear, 2, 3, cam, pt, obs, order)
    x = rng.standard_normal(ev.n)
    cost, res, vals, g = ev.evaluate(x)
    J = ev.dense_jacobian(vals)
    assert np.allclose(J @ x - obs[order].reshape(-1), res)
    assert np.allclose(J.T @ res, g) and cost == pytest.approx(0.5 * res @ res)
    ev.loss = ("huber", 0.5, 1.0, 1.0)
    cost_h, res_h, vals_h, g_h, g_plain = ev.evaluate(x, corrector_free_gradient=True)
    assert np.allclose(ev.dense_jacobian(vals_h).T @ res_h, g_h) and np.allclose(g_h, g_plain)
    assert cost_h < cost
