"""Quaternion cameras in the BAL front end (ceres_hip_bal_create_with_camera): bundle_adjuster --use_quaternions (Euclidean Plus on all ten
camera parameters) and --use_quaternions --use_manifolds (QuaternionManifold on the rotation).  The device evaluator, Plus, the gradient
norm and ceres_hip_bal_minimize against the numpy restatement (tests/quaternion_reference.py: complex-step Jacobians of the literal
formula) and against the angle-axis handle at the converted state."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import quaternion_reference as Q
from conftest import ROOT
from test_gpu_operators import rel

pytestmark = pytest.mark.gpu

MODELS = ["quaternion", "quaternion_manifold"]
LOSSES = [None, ("huber", 1.0, 1.0, 1.0), ("cauchy", 1.0, 1.0, 1.0)]


def scene(nc, npts, nobs, seed):
    """(camera_index, point_index, observations, BAL-order parameters) of a synthetic scene."""
    cam, pt, obs, cams, pts = Q.synthetic_scene(nc, npts, nobs, seed)
    return cam, pt, obs, np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def problem(hip, model, nc, npts, cam, pt, obs, solver_type=5, pre=2):
    o = hip.LinearSolverOptions(type=solver_type, preconditioner_type=pre, min_num_iterations=0, max_num_iterations=500)
    return hip.BalProblem(o, nc, npts, cam, pt, obs, camera_model=model)


def reference(gp, cam, pt, obs, loss=None):
    model = Q.QUATERNION if gp.camera_model == 1 else Q.QUATERNION_MANIFOLD
    return Q.Evaluator(model, gp.num_cameras, gp.num_points, cam, pt, obs, gp.row_order(), loss=loss)


@pytest.mark.parametrize("model", MODELS)
def test_sizes_and_evaluation_match_the_angle_axis_handle(hip, model):
    nc, npts, nobs = 20, 700, 4000
    cam, pt, obs, par = scene(nc, npts, nobs, seed=4)
    ga = problem(hip, "angle_axis", nc, npts, cam, pt, obs)
    gq = problem(hip, model, nc, npts, cam, pt, obs)
    cw = 10 if model == "quaternion" else 9
    assert gq.num_parameters == 3 * npts + 10 * nc
    assert gq.num_effective_parameters == 3 * npts + cw * nc
    assert gq.num_jacobian_values == (6 + 2 * cw) * nobs and gq.num_residuals == 2 * nobs
    assert ga.num_effective_parameters == ga.num_parameters
    np.testing.assert_array_equal(gq.row_order(), ga.row_order())
    xa, xq = ga.state_from_bal(par), gq.state_from_bal(par)
    np.testing.assert_allclose(gq.state_to_bal(xq), par, rtol=0, atol=1e-14)
    ca, ra, _, _ = ga.evaluate(xa, residuals=True)
    cq, rq, _, _ = gq.evaluate(xq, residuals=True)
    assert abs(cq - ca) <= 1e-13 * ca
    assert rel(rq, ra) <= 1e-13
    ga.close()
    gq.close()


@pytest.mark.parametrize("seed,nc,npts,nobs", [(3, 6, 80, 400), (4, 20, 700, 4000), (5, 40, 3000, 14000)])
@pytest.mark.parametrize("loss", LOSSES, ids=["squared", "huber", "cauchy"])
@pytest.mark.parametrize("model", MODELS)
def test_jacobian_matches_the_complex_step_reference(hip, model, loss, seed, nc, npts, nobs):
    cam, pt, obs, par = scene(nc, npts, nobs, seed)
    gp = problem(hip, model, nc, npts, cam, pt, obs)
    if loss:
        gp.set_loss(loss[0], loss[1])
    ev = reference(gp, cam, pt, obs, loss)
    x = gp.state_from_bal(par)
    cost_r, res_r, vals_r, g_r = ev.evaluate(x)
    cost, res, grad, vals = gp.evaluate(x, residuals=True, gradient=True, jacobian=True)
    assert abs(cost - cost_r) <= 1e-13 * cost_r
    assert rel(res, res_r) <= 1e-13
    assert rel(vals, vals_r) <= 1e-12
    assert rel(grad, ev.dense_jacobian(vals).T @ res) <= 1e-12
    assert rel(grad, g_r) <= 1e-12
    gp.close()


def test_non_unit_quaternions_and_the_identity_rotation(hip):
    nc, npts, nobs = 6, 80, 400
    cam, pt, obs, par = scene(nc, npts, nobs, seed=9)
    par[9:12] = 0.0   # camera 1: angle-axis exactly zero -> q = (1, 0, 0, 0)
    for model in MODELS:
        gp = problem(hip, model, nc, npts, cam, pt, obs)
        ev = reference(gp, cam, pt, obs)
        x = gp.state_from_bal(par)
        np.testing.assert_array_equal(x[3 * npts + 10:3 * npts + 14], [1.0, 0.0, 0.0, 0.0])
        c0, r0, _, v0 = gp.evaluate(x, residuals=True, jacobian=True)
        assert rel(v0, ev.evaluate(x)[2]) <= 1e-12
        if model == "quaternion":   # QuaternionRotatePoint normalises: q x 3.7 is the same rotation, its Jacobian 1 / 3.7 on q
            x2 = x.copy()
            x2[3 * npts:].reshape(-1, 10)[:, :4] *= 3.7
            c2, r2, _, v2 = gp.evaluate(x2, residuals=True, jacobian=True)
            assert abs(c2 - c0) <= 1e-13 * c0 and rel(r2, r0) <= 1e-13
            assert rel(v2, ev.evaluate(x2)[2]) <= 1e-12
        gp.close()


def check_loop(S, Sr, tol):
    its = Sr["iterations"]
    assert S.num_iterations_logged == len(its)
    for i, it in enumerate(its):
        d = S.iterations[i]
        assert (d.step_is_successful, d.step_is_valid) == (it["step_is_successful"], it["step_is_valid"]), i
        assert abs(d.cost - it["cost"]) <= tol * abs(it["cost"]), (i, d.cost, it["cost"])
        assert abs(d.trust_region_radius - it["trust_region_radius"]) <= tol * it["trust_region_radius"], i
    assert S.termination_type == Sr["termination_type"]


@pytest.mark.parametrize("solver_type,pre", [(5, 2), (6, 1), (3, 0)])
@pytest.mark.parametrize("model", MODELS)
def test_minimize_follows_the_reference_loop(hip, model, solver_type, pre):
    nc, npts, nobs = 10, 200, 1200
    cam, pt, obs, par = scene(nc, npts, nobs, seed=5)
    gp = problem(hip, model, nc, npts, cam, pt, obs, solver_type, pre)
    ev = reference(gp, cam, pt, obs)
    x0 = gp.state_from_bal(par)
    xr, Sr = Q.minimize(ev, x0, max_num_iterations=8)
    x, S = gp.minimize(x0, max_num_iterations=8, eta=1e-12)
    assert S.initial_cost == pytest.approx(Sr["initial_cost"], rel=1e-12)
    assert S.iterations[0].gradient_max_norm == pytest.approx(Sr["iterations"][0]["gradient_max_norm"], rel=1e-8)
    assert S.num_iterations_logged >= 5   # (this scene converges in four steps: function tolerance)
    check_loop(S, Sr, 1e-6)
    assert S.final_cost < 0.5 * S.initial_cost
    assert gp.evaluate(x)[0] == pytest.approx(S.final_cost, rel=1e-12)
    if model == "quaternion_manifold":   # Plus on the manifold keeps |q|
        qn0 = np.linalg.norm(x0[3 * npts:].reshape(-1, 10)[:, :4], axis=1)
        qn1 = np.linalg.norm(x[3 * npts:].reshape(-1, 10)[:, :4], axis=1)
        assert np.max(np.abs(qn1 - qn0)) <= 1e-14
    gp.close()


def test_plus_with_an_exactly_zero_rotation_step(hip):
    """A camera whose only point sits at the origin: its rotation columns are exactly zero at the start (-2 [R 0]x = 0), so the
    gradient norm's Plus(q, -g) and the first step's Plus(q, delta) see a rotation delta of exactly 0 — QuaternionPlus returns q (no
    sin(0) / 0)."""
    nc, npts, nobs = 6, 80, 400
    cam, pt, obs, par = scene(nc, npts, nobs, seed=12)
    # camera nc and point npts: the point at the origin, seen by the new camera and by camera 0
    cam = np.concatenate([cam, [nc, 0]]).astype(np.int32)
    pt = np.concatenate([pt, [npts, npts]]).astype(np.int32)
    newcam = np.array([0.0, 0.0, 0.0, 0.1, -0.2, -10.0, 500.0, 0.0, 0.0])
    par = np.concatenate([par[:9 * nc], newcam, par[9 * nc:], np.zeros(3)])
    obs = np.concatenate([obs, [[-4.0, 9.0], [3.0, -2.0]]])
    nc, npts = nc + 1, npts + 1
    gp = problem(hip, "quaternion_manifold", nc, npts, cam, pt, obs, 3, 0)
    ev = reference(gp, cam, pt, obs)
    x0 = gp.state_from_bal(par)
    _, _, g, _ = gp.evaluate(x0, gradient=True)
    assert np.all(g[3 * npts + 9 * (nc - 1):3 * npts + 9 * (nc - 1) + 3] == 0.0)
    xr, Sr = Q.minimize(ev, x0, max_num_iterations=3)
    x, S = gp.minimize(x0, max_num_iterations=3)
    assert np.all(np.isfinite(x)) and np.isfinite(S.final_cost)
    assert S.iterations[0].gradient_max_norm == pytest.approx(Sr["iterations"][0]["gradient_max_norm"], rel=1e-8)
    check_loop(S, Sr, 1e-6)
    gp.close()


@pytest.mark.parametrize("kind", ["traditional", "subspace"])
def test_dogleg_converges_to_the_angle_axis_minimum(hip, kind):
    nc, npts, nobs = 8, 150, 900
    cam, pt, obs, par = scene(nc, npts, nobs, seed=6)
    tight = dict(max_num_iterations=100, function_tolerance=1e-14, gradient_tolerance=1e-14, parameter_tolerance=1e-14)
    finals = {}
    for model in ("angle_axis", "quaternion_manifold"):
        gp = problem(hip, model, nc, npts, cam, pt, obs, 3, 0)
        gp.set_trust_region_strategy("dogleg", kind)
        x, S = gp.minimize(gp.state_from_bal(par), **tight)
        assert S.final_cost < 0.5 * S.initial_cost
        finals[model] = S.final_cost
        gp.close()
    assert finals["quaternion_manifold"] == pytest.approx(finals["angle_axis"], rel=1e-6)


def test_the_tile_path_is_not_taken(hip, monkeypatch):
    nc, npts, nobs = 12, 800, 3600
    cam, pt, obs, par = scene(nc, npts, nobs, seed=7)

    def run():
        gp = problem(hip, "quaternion_manifold", nc, npts, cam, pt, obs)
        x, S = gp.minimize(gp.state_from_bal(par), max_num_iterations=6)
        gp.close()
        return x, [(it.cost, it.trust_region_radius, it.gradient_max_norm) for it in S.iterations[:S.num_iterations_logged]]

    monkeypatch.delenv("CERES_HIP_EVAL_TILES", raising=False)
    xa, ta = run()
    monkeypatch.setenv("CERES_HIP_EVAL_TILES", "0")
    xb, tb = run()
    np.testing.assert_array_equal(xa, xb)
    assert ta == tb


def test_model_zero_is_ceres_hip_bal_create(hip, monkeypatch):
    nc, npts, nobs = 12, 800, 3600
    cam, pt, obs, par = scene(nc, npts, nobs, seed=8)
    ga = problem(hip, "angle_axis", nc, npts, cam, pt, obs)
    gb = problem(hip, "angle_axis", nc, npts, cam, pt, obs)
    lib = hip.load_library()
    op = ga.options   # (the options BalProblem passes to ceres_hip_bal_create)
    o = hip.COptions(op.type, op.preconditioner_type, op.min_num_iterations, op.max_num_iterations, op.residual_reset_period, npts, op.device,
                     int(op.force_generic_path), op.cg_check_interval, op.jacobian_storage, op.max_num_spse_iterations,
                     int(op.use_spse_initialization), op.spse_tolerance, int(op.use_explicit_schur_complement))
    i32 = ctypes.POINTER(ctypes.c_int32)
    h = lib.ceres_hip_bal_create_with_camera(ctypes.byref(o), 0, nc, npts, nobs, cam.ctypes.data_as(i32), pt.ctypes.data_as(i32),
                                             np.ascontiguousarray(obs).ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert h, lib.ceres_hip_bal_last_error(None).decode()
    lib.ceres_hip_bal_destroy(gb._h)
    gb._h = h
    x0 = ga.state_from_bal(par)
    ea = ga.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    eb = gb.evaluate(x0, residuals=True, gradient=True, jacobian=True)
    assert ea[0] == eb[0]
    for u, v in zip(ea[1:], eb[1:]):
        np.testing.assert_array_equal(u, v)
    xa, Sa = ga.minimize(x0, max_num_iterations=6)
    xb, Sb = gb.minimize(x0, max_num_iterations=6)
    np.testing.assert_array_equal(xa, xb)
    fields = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_successful")
    assert Sa.num_iterations_logged == Sb.num_iterations_logged
    for i in range(Sa.num_iterations_logged):
        assert all(getattr(Sa.iterations[i], f) == getattr(Sb.iterations[i], f) for f in fields), i
    ga.close()
    gb.close()


@pytest.mark.parametrize("model", MODELS)
def test_refusals(hip, model):
    nc, npts, nobs = 6, 80, 400
    cam, pt, obs, par = scene(nc, npts, nobs, seed=3)
    gp = problem(hip, model, nc, npts, cam, pt, obs)
    x = gp.state_from_bal(par)
    for call in (lambda: gp.set_inner_iterations("automatic"), lambda: gp.inner_iterate(x), lambda: gp.evaluate_tiles_timing(x)):
        with pytest.raises(hip.HipError) as e:
            call()
        assert "error -2" in str(e.value), str(e.value)
    gp.set_inner_iterations(None)   # (NONE stays allowed)
    assert np.isfinite(gp.minimize(x, max_num_iterations=2)[1].final_cost)
    gp.close()


@pytest.mark.parametrize("model", MODELS)
def test_cpp_host_mirror_in_quaternion_mode(hip, model, tmp_path):
    nc, npts, nobs = 8, 250, 1200
    cam, pt, obs, par = scene(nc, npts, nobs, seed=17)
    f = str(tmp_path / "problem.txt")
    from ceres_solver_amd import problems
    problems.write_bal(f, nc, npts, cam, pt, obs, par)
    exe = os.path.join(ROOT, "ceres-solver_amd", "host", "host_driver")
    r = subprocess.run([exe, f, "6", model], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(re.findall(r"(\w+)=([^ ]+)", [l for l in r.stdout.splitlines() if l.startswith("bal ")][0]))
    kq = dict(re.findall(r"(\w+)=([^ ]+)", [l for l in r.stdout.splitlines() if l.startswith("quaternion ")][0]))
    o = hip.LinearSolverOptions(type=hip.ITERATIVE_SCHUR, preconditioner_type=hip.SCHUR_JACOBI, min_num_iterations=0, max_num_iterations=500)
    gp, x0 = hip.BalProblem.from_file(o, f, camera_model=model)
    x, S = gp.minimize(x0, max_num_iterations=6)
    ga, xa = hip.BalProblem.from_file(o, f)
    assert ga.evaluate(xa)[0] == pytest.approx(gp.evaluate(x0)[0], rel=1e-13)
    ga.close()
    gp.close()
    assert int(kv["parameters"]) == gp.num_parameters and int(kq["effective_parameters"]) == gp.num_effective_parameters
    assert float(kv["initial_cost"]) == pytest.approx(S.initial_cost, rel=1e-13)
    assert float(kv["final_cost"]) == pytest.approx(S.final_cost, rel=1e-9)
    assert float(kq["angle_axis_final"]) == pytest.approx(float(kv["final_cost"]), rel=1e-9)
    assert int(kv["successful"]) == S.num_successful_steps and S.final_cost < 0.5 * S.initial_cost
