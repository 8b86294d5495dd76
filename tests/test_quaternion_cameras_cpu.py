"""The numpy restatement of the quaternion cameras (tests/quaternion_reference.py) checked on its own, and the camera-model refusal of
ceres_hip_bal_create_with_camera, which comes before any device call.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import quaternion_reference as Q
from conftest import pkg


def scene_rows(n=40, seed=3):
    cam, pt, obs, cams, pts = Q.synthetic_scene(5, 30, n, seed)
    q = np.concatenate([Q.angle_axis_to_quaternion(cams[:, :3]), cams[:, 3:]], axis=1)
    return q[cam], pts[pt], obs, cams[cam]


def test_complex_step_matches_central_differences():
    cams, X, obs, _ = scene_rows()
    jc, jp = Q.ambient_jacobian(cams, X, obs)
    for j in range(10):
        h = 1e-6 * max(1.0, float(np.max(np.abs(cams[:, j]))))
        cp, cm = cams.copy(), cams.copy()
        cp[:, j] += h
        cm[:, j] -= h
        fd = (Q.residual(cp, X, obs) - Q.residual(cm, X, obs)) / (2 * h)
        assert np.max(np.abs(fd - jc[:, :, j])) <= 1e-6 * max(1.0, np.max(np.abs(jc[:, :, j]))), j
    for j in range(3):
        xp, xm = X.copy(), X.copy()
        xp[:, j] += 1e-6
        xm[:, j] -= 1e-6
        fd = (Q.residual(cams, xp, obs) - Q.residual(cams, xm, obs)) / 2e-6
        assert np.max(np.abs(fd - jp[:, :, j])) <= 1e-6 * max(1.0, np.max(np.abs(jp[:, :, j]))), j


def test_quaternion_residual_is_the_angle_axis_residual():
    cams, X, obs, cams_aa = scene_rows()
    p = Q.angle_axis_rotate_point(cams_aa[:, :3], X) + cams_aa[:, 3:6]
    xp, yp = -p[:, 0] / p[:, 2], -p[:, 1] / p[:, 2]
    r2 = xp * xp + yp * yp
    d = 1.0 + r2 * (cams_aa[:, 7] + cams_aa[:, 8] * r2)
    r_aa = np.stack([cams_aa[:, 6] * d * xp - obs[:, 0], cams_aa[:, 6] * d * yp - obs[:, 1]], axis=1)
    r_q = Q.residual(cams, X, obs)
    assert np.max(np.abs(r_q - r_aa)) <= 1e-12 * np.max(np.abs(r_aa))
    # QuaternionRotatePoint does not assume |q| = 1
    c2 = cams.copy()
    c2[:, :4] *= 3.7
    assert np.max(np.abs(Q.residual(c2, X, obs) - r_q)) <= 1e-12 * np.max(np.abs(r_q))


def test_angle_axis_quaternion_round_trip():
    rng = np.random.default_rng(11)
    a = rng.normal(0.0, 1.0, (200, 3))
    a *= (rng.uniform(0.0, np.pi * 0.999, 200) / np.linalg.norm(a, axis=1))[:, None]
    a[0] = 0.0
    q = Q.angle_axis_to_quaternion(a)
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(Q.quaternion_to_angle_axis(q), a, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(q[0], [1.0, 0.0, 0.0, 0.0])
    # -q is the same rotation: QuaternionToAngleAxis still returns the angle within [-pi, pi]
    np.testing.assert_allclose(Q.quaternion_to_angle_axis(-q), a, rtol=0, atol=1e-14)
    # the product's conversions agree with the restatement
    hs = pkg.hip_solver
    np.testing.assert_array_equal(hs.angle_axis_to_quaternion(a), q)
    np.testing.assert_array_equal(hs.quaternion_to_angle_axis(q), Q.quaternion_to_angle_axis(q))


def test_plus_preserves_the_norm_and_is_exact_at_zero():
    rng = np.random.default_rng(5)
    q = rng.normal(0.0, 1.0, (100, 4))
    d = rng.normal(0.0, 0.5, (100, 3))
    d[0] = 0.0
    out = Q.quaternion_plus(q, d)
    np.testing.assert_allclose(np.linalg.norm(out, axis=1), np.linalg.norm(q, axis=1), rtol=1e-15)
    np.testing.assert_array_equal(out[0], q[0])
    # PlusJacobian is the derivative of Plus at delta = 0, and its columns are orthogonal to q
    P = Q.plus_jacobian(q)
    for j in range(3):
        e = np.zeros((100, 3))
        e[:, j] = 1e-7
        fd = (Q.quaternion_plus(q, e) - Q.quaternion_plus(q, -e)) / 2e-7
        np.testing.assert_allclose(fd, P[:, :, j], rtol=0, atol=1e-8 * np.max(np.abs(q)))
    assert np.max(np.abs(np.einsum("nk,nkj->nj", q, P))) <= 1e-15 * np.max(np.abs(q)) ** 2


@pytest.mark.parametrize("qscale", [1.0, 3.7, 0.2])
def test_manifold_jacobian_closed_form(qscale):
    # J_ambient x PlusJacobian on the rotation = J_proj (-2 [R(q / |q|) X]x), whatever |q| is (the device kernel's form)
    cams, X, obs, _ = scene_rows(seed=7)
    cams[:, :4] *= qscale
    jc, _ = Q.ambient_jacobian(cams, X, obs)
    local = Q.local_camera_jacobian(jc, cams[:, :4], Q.QUATERNION_MANIFOLD)
    Y = Q.quaternion_rotate_point(cams[:, :4], X)
    # the projection's derivative d res / d p is the translation block of the ambient Jacobian (p = Y + t)
    Jproj = jc[:, :, 4:7]
    closed = np.einsum("nkm,nmj->nkj", Jproj, -2.0 * Q.cross_matrix(Y))
    assert np.max(np.abs(local[:, :, :3] - closed)) <= 1e-12 * np.max(np.abs(closed))
    assert local.shape[2] == 9
    np.testing.assert_array_equal(local[:, :, 3:], jc[:, :, 4:])


def test_reference_loop_descends_on_both_models():
    cam, pt, obs, cams, pts = Q.synthetic_scene(4, 25, 120, seed=2)
    order = np.lexsort((np.arange(cam.shape[0]), pt))
    for model in (Q.QUATERNION, Q.QUATERNION_MANIFOLD):
        ev = Q.Evaluator(model, 4, 25, cam, pt, obs, order)
        x0 = np.concatenate([pts.reshape(-1), np.concatenate([Q.angle_axis_to_quaternion(cams[:, :3]), cams[:, 3:]], axis=1).reshape(-1)])
        c0, r, vals, g = ev.evaluate(x0)
        J = ev.dense_jacobian(vals)
        np.testing.assert_allclose(g, J.T @ r, rtol=0, atol=1e-12 * np.max(np.abs(g)))
        x, S = Q.minimize(ev, x0, max_num_iterations=6)
        assert S["final_cost"] < 0.5 * S["initial_cost"]
        qn0 = np.linalg.norm(x0[75:].reshape(-1, 10)[:, :4], axis=1)
        qn1 = np.linalg.norm(x[75:].reshape(-1, 10)[:, :4], axis=1)
        if model == Q.QUATERNION_MANIFOLD:
            np.testing.assert_allclose(qn1, qn0, rtol=1e-14)


def test_create_with_an_unknown_camera_model_fails_before_the_device():
    hs = pkg.hip_solver
    lib = hs.load_library()
    o = hs.COptions()
    o.solver_type, o.preconditioner_type, o.max_num_iterations = hs.ITERATIVE_SCHUR, hs.SCHUR_JACOBI, 10
    cam = np.array([0, 1, 0], dtype=np.int32)
    pt = np.array([0, 1, 2], dtype=np.int32)
    obs = np.zeros(6)
    h = lib.ceres_hip_bal_create_with_camera(ctypes.byref(o), 7, 2, 3, 3, cam.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             pt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), obs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert not h
    msg = lib.ceres_hip_bal_last_error(None).decode()
    assert "camera_model" in msg and "7" in msg, msg
    with pytest.raises(ValueError):
        hs.BalProblem(hs.LinearSolverOptions(type=hs.ITERATIVE_SCHUR, preconditioner_type=hs.SCHUR_JACOBI), 2, 3, cam, pt, obs,
                      camera_model="rodrigues")
