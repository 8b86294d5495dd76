"""The cases on which ceres_hip_bal_minimize with bound constraints is compared with tests/bounds_reference.py
(tests/test_gpu_bounds.py), shared with the CPU test that holds the restatement's runs on them to be decided nowhere by rounding
(tests/test_bounds_cpu.py).  The scene is test_gpu_frontend_matrix.clean_scene (10 cameras, 200 points, 1200 observations), the initial
state line_search_cases.initial_state, and the box is built from the scene alone: with x8 the state after eight UNBOUNDED iterations of
frontend_reference.minimize on the case's own camera, loss and constants,

  every free camera     f in [0.998 f0, 1.002 f0];  k1 in [min(k1_0, m) - 1e-12, max(k1_0, m) + 1e-12], m = (k1_0 + k1_8) / 2
  every free point q = 0, 3, 6, ...   z >= (z_0 + z_8) / 2, no upper bound

(f is camera coordinate cs - 3, k1 is cs - 2) and everything else unbounded: the unbounded trajectory leaves the box, so bounds bind."""
import numpy as np

import frontend_reference as F
import line_search_cases as LC
import line_search_reference as LS

# name: camera, loss (set_loss arguments or None), constant cameras, constant points, strategy, the search's options, iterations, the
# device's (linear solver, preconditioner), force_generic_path
CASES = {
    "cubic_default": ("angle_axis", None, None, None, "lm", dict(), 8, (5, 2), 0),
    "huber_first_sample": ("angle_axis", ("huber", 2.0, 1.0, 1.0), None, None, "lm", dict(), 8, (6, 1), 0),
    "quadratic": ("angle_axis", None, None, None, "lm", dict(line_search_interpolation_type=LS.QUADRATIC), 8, (5, 2), 1),
    "one_iteration": ("angle_axis", None, None, None, "lm", dict(max_num_line_search_step_size_iterations=1), 8, (3, 0), 0),
    "quaternion_constant": ("quaternion", None, [0], [0, 1, 2], "lm", dict(), 8, (5, 2), 0),
    "quaternion_quadratic": ("quaternion", None, None, None, "lm", dict(line_search_interpolation_type=LS.QUADRATIC), 8, (3, 0), 0),
    "dogleg": ("angle_axis", None, None, None, "traditional", dict(), 4, (3, 0), 0),
}
NOISE_SEEDS = (1, 2)


def matrix_case(name):
    """The row of test_gpu_frontend_matrix's table this case corresponds to (for its `tolerances`)."""
    camera, loss, _, _, strategy, _, _, solver, generic = CASES[name]
    return (camera, loss[0] if loss else "none", 1.0, strategy, solver, generic, None, 1, None, None)


def scene(oracle):
    """clean_scene with its parameters in STATE order (points, then cameras): what line_search_cases.initial_state takes."""
    from test_gpu_frontend_matrix import clean_scene
    nc, npts, cam, pt, obs, par = clean_scene(oracle)
    return nc, npts, cam, pt, obs, np.concatenate([par[9 * nc:], par[:9 * nc]])


def setup(oracle, name, sc=None):
    """(scene, reference problem, x0, lower, upper) of a case."""
    camera, loss, cc, cp, _, _, _, _, _ = CASES[name]
    sc = sc if sc is not None else scene(oracle)
    pr = LC.reference_problem(oracle, sc, camera, loss, cc, cp)
    x0 = LC.initial_state(sc, camera)
    lower, upper = box(pr, sc, x0, cc, cp)
    return sc, pr, x0, lower, upper


def box(pr, sc, x0, cc, cp):
    nc, npts = sc[0], sc[1]
    cs = pr.cs
    x8, _ = F.minimize(pr, x0, max_num_iterations=8)
    lower, upper = np.full(x0.size, -np.inf), np.full(x0.size, np.inf)
    const_c, const_p = set(cc or []), set(cp or [])
    for c in range(nc):
        if c in const_c:
            continue
        f, k1 = 3 * npts + cs * c + cs - 3, 3 * npts + cs * c + cs - 2
        assert x0[f] > 0.0
        lower[f], upper[f] = 0.998 * x0[f], 1.002 * x0[f]
        m = 0.5 * (x0[k1] + x8[k1])
        lower[k1], upper[k1] = min(x0[k1], m) - 1e-12, max(x0[k1], m) + 1e-12
    for q in range(0, npts, 3):
        if q in const_p:
            continue
        lower[3 * q + 2] = 0.5 * (x0[3 * q + 2] + x8[3 * q + 2])
    return lower, upper


def run_reference(pr, x0, lower, upper, name, jacobian_noise=None):
    import bounds_reference as B
    _, _, _, _, strategy, lso, iters, _, _ = CASES[name]
    return B.minimize(pr, x0, lower, upper, strategy=strategy, jacobian_noise=jacobian_noise, line_search_options=lso, max_num_iterations=iters)


_REFERENCE = {}


def reference(oracle, name):
    """dict(sc, pr, x0, lower, upper, x, S) of a case: computed once per session, shared by every test that needs it, never changed."""
    if name not in _REFERENCE:
        if "scene" not in _REFERENCE:
            _REFERENCE["scene"] = scene(oracle)
        sc, pr, x0, lower, upper = setup(oracle, name, _REFERENCE["scene"])
        x, S = run_reference(pr, x0, lower, upper, name)
        for a in (x0, lower, upper, x):
            a.setflags(write=False)
        _REFERENCE[name] = dict(sc=sc, pr=pr, x0=x0, lower=lower, upper=upper, x=x, S=S)
    return _REFERENCE[name]
