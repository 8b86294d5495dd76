"""The (scene, options) pairs on which the device line search minimizer is compared with tests/line_search_reference.py
(tests/test_gpu_line_search.py), shared with the CPU test that holds the restatement's runs on them to be non-degenerate
(tests/test_line_search_cpu.py): decisions with a margin, a zoom phase, an expansion or a first-sample accept, a circular-buffer
overwrite at rank 3, a cost that falls — and one run that ends on a step of zero."""
import numpy as np

import constant_blocks_reference as CB
import line_search_reference as LS

MODELS = {"angle_axis": 0, "quaternion": 1, "quaternion_manifold": 2}
COMPARED_ITERATIONS = 10


def small_scene(oracle, seed):
    """6 cameras, 40 points, about 200 observations, the pixels and the state perturbed: cheap for the numpy evaluators."""
    op = oracle.BalProblem.generate(6, 40, 200, seed=seed)
    op.build_structure(True)
    cam, pt, obs = op.indices()
    return op.num_cameras, op.num_points, cam, pt, obs, op.state()


# name: (seed, camera, loss, constant cameras, constant points, options, what the scene offers the line search).  "expansion": a Wolfe
# run with an iteration of more than one bracketing step; "first_sample": a Wolfe run on a scene that offers no expansion — the first
# sample is accepted or brackets at once, zoom follows; "armijo": an Armijo run (no bracketing, no zoom): a contraction instead.
CASES = {
    "lbfgs_default": (3, "angle_axis", None, None, None, dict(), "first_sample"),
    "lbfgs_rank3_scaling": (3, "angle_axis", None, None, None, dict(max_lbfgs_rank=3, use_approximate_eigenvalue_bfgs_scaling=1), "first_sample"),
    "lbfgs_manifold_huber": (5, "quaternion_manifold", ("huber", 1.0, 1.0, 1.0), None, None, dict(), "first_sample"),
    "lbfgs_constant_blocks": (3, "angle_axis", ("cauchy", 1.0, 1.0, 1.0), [0], [0, 1, 2], dict(line_search_interpolation_type=LS.QUADRATIC),
                              "first_sample"),
    "ncg_polak_ribiere": (3, "quaternion", None, None, None,
                          dict(line_search_direction_type=LS.NONLINEAR_CONJUGATE_GRADIENT, nonlinear_conjugate_gradient_type=LS.POLAK_RIBIERE), "expansion"),
    "ncg_hestenes_stiefel_armijo": (3, "angle_axis", None, None, None,
                                    dict(line_search_direction_type=LS.NONLINEAR_CONJUGATE_GRADIENT, nonlinear_conjugate_gradient_type=LS.HESTENES_STIEFEL,
                                         line_search_type=LS.ARMIJO, line_search_interpolation_type=LS.QUADRATIC), "armijo"),
    "steepest_armijo": (3, "angle_axis", None, None, None,
                        dict(line_search_direction_type=LS.STEEPEST_DESCENT, line_search_type=LS.ARMIJO, line_search_interpolation_type=LS.QUADRATIC),
                        "armijo"),
}

# A run whose line search hands the initial position back: with ONE step-size iteration allowed, the first sample (step 1 / |g|_inf along
# -g) violates the Armijo condition, the bracket is [0, t] and the zoom phase has no iteration left — its best Armijo point so far is the
# initial position.  The step is zero, the position's gradient is evaluated again (the only evaluation the minimizer adds: 3 function and
# 3 gradient evaluations in all) and the parameter tolerance ends the run after its first iteration.
ZERO_STEP_CASES = {
    "lbfgs_zero_step": (5, "quaternion_manifold", None, [0], [0, 1, 2], dict(max_num_line_search_step_size_iterations=1), "zero_step"),
}
ALL_CASES = dict(CASES, **ZERO_STEP_CASES)


def reference_problem(oracle, sc, camera, loss, cc, cp):
    nc, npts, cam, pt, obs, _ = sc
    return CB.Problem(oracle.snavely_batch, MODELS[camera], nc, npts, cam, pt, obs, cc, cp, loss)


def initial_state(sc, camera):
    """The scene's angle-axis state in the camera model's layout (quaternion_reference's conversion)."""
    import quaternion_reference as Q
    nc, npts, _, _, _, st = sc
    if camera == "angle_axis":
        return np.array(st, dtype=np.float64)
    cams = st[3 * npts:].reshape(nc, 9)
    q = Q.angle_axis_to_quaternion(cams[:, :3])
    return np.concatenate([st[:3 * npts], np.concatenate([q, cams[:, 3:]], axis=1).reshape(-1)])


def run_reference(oracle, name):
    seed, camera, loss, cc, cp, opts, _ = ALL_CASES[name]
    sc = small_scene(oracle, seed)
    pr = reference_problem(oracle, sc, camera, loss, cc, cp)
    x0 = initial_state(sc, camera)
    return sc, pr, x0, LS.minimize(pr, x0, max_num_iterations=COMPARED_ITERATIONS, **opts)
