"""The composed restatement of ceres_hip_bal_minimize (tests/frontend_reference.py) against each per-feature restatement within that
one's own domain: the same flags, and costs, radii and states to 1e-13.  The composed loop then rests on the references the per-feature
GPU tests already trust.  No GPU."""
import numpy as np
import pytest

import dogleg_reference as DR
import frontend_reference as F
import inner_reference as IR
import quaternion_reference as Q
import robust_reference as R

LOSSES = [None, ("trivial", 1.0, 1.0, 2.5), ("huber", 2.0, 1.0, 1.0), ("soft_l_one", 2.0, 1.0, 2.5), ("cauchy", 2.0, 1.0, 1.0),
          ("arctan", 3.0, 1.0, 2.5), ("tolerant", 4.0, 1.0, 1.0), ("tukey", 6.0, 1.0, 2.5)]
LOSS_IDS = ["squared"] + [f"{l[0]}-{l[3]}" for l in LOSSES[1:]]
TOL = 1e-13


def small_scene(seed=5, nc=6, npts=60, nobs=320, outliers=0.05):
    """quaternion_reference.synthetic_scene with `outliers` of its observations 5-30 px off: (cam, pt, obs, BAL-order parameters)."""
    cam, pt, obs, cams, pts = Q.synthetic_scene(nc, npts, nobs, seed)
    rng = np.random.default_rng(seed + 77)
    out = rng.random(nobs) < outliers
    ang, mag = rng.uniform(0, 2 * np.pi, out.sum()), rng.uniform(5.0, 30.0, out.sum())
    obs = obs.copy()
    obs[out, 0] += mag * np.cos(ang)
    obs[out, 1] += mag * np.sin(ang)
    return cam, pt, obs, cams, pts


def angle_axis(oracle, sc, loss=None):
    cam, pt, obs, cams, pts = sc
    order = np.argsort(pt, kind="stable")
    ev = R.Evaluator(oracle.snavely_batch, cams.shape[0], pts.shape[0], cam, pt, obs, order, loss=loss)
    return ev, np.concatenate([pts.reshape(-1), cams.reshape(-1)])


def quaternion(model, sc, loss=None):
    cam, pt, obs, cams, pts = sc
    order = np.argsort(pt, kind="stable")
    ev = Q.Evaluator(model, cams.shape[0], pts.shape[0], cam, pt, obs, order, loss=loss)
    qc = np.concatenate([Q.angle_axis_to_quaternion(cams[:, :3]), cams[:, 3:]], axis=1)
    return ev, np.concatenate([pts.reshape(-1), qc.reshape(-1)])


def same(x, S, xr, Sr, fields=("step_is_successful", "step_is_valid")):
    its, itr = S["iterations"], Sr["iterations"]
    assert len(its) == len(itr) >= 3
    for i, (a, b) in enumerate(zip(its, itr)):
        assert all(a[f] == b[f] for f in fields), (i, a, b)
        assert abs(a["cost"] - b["cost"]) <= TOL * abs(b["cost"]), (i, a["cost"], b["cost"])
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= TOL * b["trust_region_radius"], i
    assert S["termination_type"] == Sr["termination_type"]
    assert abs(S["final_cost"] - Sr["final_cost"]) <= TOL * Sr["final_cost"]
    assert np.max(np.abs(x - xr)) <= TOL * np.max(np.abs(xr))


@pytest.mark.parametrize("jacobi_scaling", [1, 0])
@pytest.mark.parametrize("loss", LOSSES, ids=LOSS_IDS)
def test_levenberg_marquardt_is_robust_reference(oracle, loss, jacobi_scaling):
    ev, x0 = angle_axis(oracle, small_scene(), loss)
    xr, Sr = R.minimize(ev, x0, max_num_iterations=8, jacobi_scaling=jacobi_scaling)
    x, S = F.minimize(F.Problem(ev), x0, "lm", max_num_iterations=8, jacobi_scaling=jacobi_scaling)
    same(x, S, xr, Sr)
    assert S["num_linear_solves"] == len(S["iterations"]) - 1 and S["num_inner_iteration_steps"] == 0


@pytest.mark.parametrize("loss", [None, ("cauchy", 2.0, 1.0, 2.5)], ids=["squared", "cauchy"])
@pytest.mark.parametrize("model", [Q.QUATERNION, Q.QUATERNION_MANIFOLD])
def test_levenberg_marquardt_is_quaternion_reference(model, loss):
    ev, x0 = quaternion(model, small_scene(seed=6), loss)
    xr, Sr = Q.minimize(ev, x0, max_num_iterations=8)
    x, S = F.minimize(F.Problem(ev), x0, "lm", max_num_iterations=8)
    same(x, S, xr, Sr)
    if model == Q.QUATERNION_MANIFOLD:
        qn = lambda v: np.linalg.norm(v[3 * ev.np_:].reshape(-1, 10)[:, :4], axis=1)
        assert np.max(np.abs(qn(x) - qn(x0))) <= 1e-14


@pytest.mark.parametrize("inner", [False, True], ids=["plain", "inner"])
@pytest.mark.parametrize("jacobi_scaling", [1, 0])
@pytest.mark.parametrize("kind", ["traditional", "subspace"])
def test_dogleg_is_dogleg_reference(oracle, kind, jacobi_scaling, inner):
    sc = small_scene(seed=7)
    loss = ("huber", 2.0, 1.0, 1.0)
    ev, x0 = angle_axis(oracle, sc, loss)
    grp = IR.ordering(sc[3].shape[0], sc[4].shape[0], sc[0], sc[1], "automatic") if inner else None
    kw = dict(max_num_iterations=8, jacobi_scaling=jacobi_scaling, initial_trust_region_radius=10.0)
    xr, Sr = DR.minimize(ev, x0, kind, inner=grp, **kw)
    x, S = F.minimize(F.Problem(ev), x0, kind, inner=grp, **kw)
    same(x, S, xr, Sr, fields=("step_is_successful", "step_is_valid", "branch", "solves", "linear_solver_iterations"))
    assert S["num_linear_solves"] == Sr["num_linear_solves"]
    assert (S["num_inner_iteration_steps"] > 0) == inner


@pytest.mark.parametrize("blocks,tol", [("automatic", 1e-3), ("cameras,points", 1e-3), ("points", 0.2)])
def test_inner_iterations_are_inner_reference(oracle, blocks, tol):
    sc = small_scene(seed=8)
    ev, x0 = angle_axis(oracle, sc, ("cauchy", 2.0, 1.0, 1.0))
    group, ng = IR.ordering(sc[3].shape[0], sc[4].shape[0], sc[0], sc[1], blocks)
    xr, Sr = IR.minimize(ev, x0, group, ng, inner_iteration_tolerance=tol, max_num_iterations=8)
    x, S = F.minimize(F.Problem(ev), x0, "lm", inner=(group, ng), inner_iteration_tolerance=tol, max_num_iterations=8)
    same(x, S, xr, Sr)
    assert S["num_inner_iteration_steps"] == Sr["num_inner_iteration_steps"] >= 1
    assert S["inner_enabled_at_end"] == Sr["inner_enabled_at_end"]
    assert sum(it["inner_step"] for it in S["iterations"]) == S["num_inner_iteration_steps"]


def test_quaternion_dogleg_descends_to_the_angle_axis_minimum(oracle):
    """The composition no single restatement covers: dogleg on both quaternion models reaches the minimum angle-axis LM reaches."""
    sc = small_scene(seed=9, outliers=0.0)
    tight = dict(max_num_iterations=60, function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14)
    ev, x0 = angle_axis(oracle, sc)
    _, Sa = F.minimize(F.Problem(ev), x0, "lm", **tight)
    for model in (Q.QUATERNION, Q.QUATERNION_MANIFOLD):
        evq, xq = quaternion(model, sc)
        for kind in ("traditional", "subspace"):
            _, S = F.minimize(F.Problem(evq), xq, kind, **tight)
            assert S["final_cost"] == pytest.approx(Sa["final_cost"], rel=1e-8), (model, kind)


def test_inner_iterations_refuse_quaternion_cameras():
    ev, x0 = quaternion(Q.QUATERNION_MANIFOLD, small_scene())
    with pytest.raises(AssertionError):
        F.minimize(F.Problem(ev), x0, "lm", inner=(np.zeros(1, np.int64), 1))
