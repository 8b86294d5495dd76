"""A numpy restatement of the quaternion cameras of the BAL front end (ceres_hip_bal_create_with_camera): what the device evaluator
(csrc/snavely.h snavely_quat, csrc/bal_evaluate.h), the Plus and gradient-norm kernels (csrc/kernels_quaternion.hip) and
ceres_hip_bal_minimize (csrc/bal_frontend.inc) are checked against.  It imports nothing from the product.

  AngleAxisToQuaternion, QuaternionToAngleAxis,
  QuaternionRotatePoint, UnitQuaternionRotatePoint   include/ceres/rotation.h
  the residual                                       examples/snavely_reprojection_error.h (SnavelyReprojectionErrorWithQuaternions)
  QuaternionPlus, QuaternionPlusJacobian             internal/ceres/manifold.cc (QuaternionPlusImpl, QuaternionPlusJacobianImpl)
  the local Jacobian                                 internal/ceres/residual_block.cc: ambient J x PlusJacobian, then the Corrector
  gradient_max_norm                                  internal/ceres/trust_region_minimizer.cc: |x - Plus(x, -g)|_inf

The Jacobian is the complex-step derivative of the literal formula: independent of the analytic one, and exact to rounding.  Camera
models: 0 angle-axis (not restated here), 1 quaternion with Euclidean Plus (10 tangent columns), 2 quaternion manifold (9)."""
import numpy as np

from robust_reference import correct, rho

QUATERNION, QUATERNION_MANIFOLD = 1, 2
STEP = 1e-30   # complex step: f(x + i h) = f(x) + i h f'(x) + O(h^2)


def angle_axis_to_quaternion(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    theta = np.sqrt(np.sum(a * a, axis=1))
    nz = theta != 0.0
    th = np.where(nz, theta, 1.0)
    k = np.where(nz, np.sin(0.5 * th) / th, 0.5)
    return np.concatenate([np.where(nz, np.cos(0.5 * th), 1.0)[:, None], a * k[:, None]], axis=1)


def quaternion_to_angle_axis(q):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    s = np.sqrt(np.sum(q[:, 1:] ** 2, axis=1))
    nz = s != 0.0
    sign = np.copysign(1.0, q[:, 0])
    k = np.where(nz, 2.0 * np.arctan2(sign * s, sign * q[:, 0]) / np.where(nz, s, 1.0), 2.0)
    return q[:, 1:] * k[:, None]


def angle_axis_rotate_point(a, X):
    """Rodrigues' formula, rows (n, 3) (for tests that compare the two camera models)."""
    a, X = np.asarray(a, dtype=np.float64), np.asarray(X, dtype=np.float64)
    theta = np.sqrt(np.sum(a * a, axis=1))[:, None]
    w = a / np.where(theta == 0.0, 1.0, theta)
    c, s = np.cos(theta), np.sin(theta)
    return X * c + np.cross(w, X) * s + w * np.sum(w * X, axis=1, keepdims=True) * (1.0 - c)


def quaternion_rotate_point(q, X):
    """QuaternionRotatePoint: u = q / |q|, then UnitQuaternionRotatePoint, statement by statement; rows, real or complex."""
    scale = 1.0 / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    w, x, y, z = (scale * q[:, k] for k in range(4))
    uv0 = y * X[:, 2] - z * X[:, 1]
    uv1 = z * X[:, 0] - x * X[:, 2]
    uv2 = x * X[:, 1] - y * X[:, 0]
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    r0 = X[:, 0] + w * uv0 + (y * uv2 - z * uv1)
    r1 = X[:, 1] + w * uv1 + (z * uv0 - x * uv2)
    r2 = X[:, 2] + w * uv2 + (x * uv1 - y * uv0)
    return np.stack([r0, r1, r2], axis=1)


def residual(cams, X, obs):
    """SnavelyReprojectionErrorWithQuaternions on rows: cams (n, 10) = [q(4) t(3) f k1 k2], X (n, 3), obs (n, 2)."""
    p = quaternion_rotate_point(cams[:, :4], X) + cams[:, 4:7]
    xp, yp = -p[:, 0] / p[:, 2], -p[:, 1] / p[:, 2]
    r2 = xp * xp + yp * yp
    dist = 1.0 + r2 * (cams[:, 8] + cams[:, 9] * r2)
    return np.stack([cams[:, 7] * dist * xp - obs[:, 0], cams[:, 7] * dist * yp - obs[:, 1]], axis=1)


def ambient_jacobian(cams, X, obs):
    """(d res / d cam (n, 2, 10), d res / d X (n, 2, 3)) by complex step."""
    cams, X = np.asarray(cams, dtype=np.float64), np.asarray(X, dtype=np.float64)
    jc = np.empty((cams.shape[0], 2, 10))
    jp = np.empty((cams.shape[0], 2, 3))
    for j in range(10):
        c = cams.astype(np.complex128)
        c[:, j] += 1j * STEP
        jc[:, :, j] = residual(c, X, obs).imag / STEP
    for j in range(3):
        x = X.astype(np.complex128)
        x[:, j] += 1j * STEP
        jp[:, :, j] = residual(cams, x, obs).imag / STEP
    return jc, jp


def quaternion_plus(q, d):
    """QuaternionPlusImpl on rows: [cos |d|, sin |d| / |d| d] (x) q, and q where |d| is exactly 0."""
    q, d = np.asarray(q, dtype=np.float64).reshape(-1, 4), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    nd = np.sqrt(np.sum(d * d, axis=1))
    zero = nd == 0.0
    n1 = np.where(zero, 1.0, nd)
    s = np.sin(n1) / n1
    z = np.concatenate([np.cos(n1)[:, None], s[:, None] * d], axis=1)
    out = np.stack([z[:, 0] * q[:, 0] - z[:, 1] * q[:, 1] - z[:, 2] * q[:, 2] - z[:, 3] * q[:, 3],
                    z[:, 0] * q[:, 1] + z[:, 1] * q[:, 0] + z[:, 2] * q[:, 3] - z[:, 3] * q[:, 2],
                    z[:, 0] * q[:, 2] - z[:, 1] * q[:, 3] + z[:, 2] * q[:, 0] + z[:, 3] * q[:, 1],
                    z[:, 0] * q[:, 3] + z[:, 1] * q[:, 2] - z[:, 2] * q[:, 1] + z[:, 3] * q[:, 0]], axis=1)
    return np.where(zero[:, None], q, out)


def plus_jacobian(q):
    """QuaternionPlusJacobianImpl on rows: (n, 4, 3)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([-x, -y, -z], axis=1), np.stack([w, z, -y], axis=1),
                     np.stack([-z, w, x], axis=1), np.stack([y, -x, w], axis=1)], axis=1)


def local_camera_jacobian(jc, q, model):
    """The camera block of the local Jacobian: jc (n, 2, 10) as it is (model 1), or with its rotation columns times PlusJacobian (2)."""
    if model == QUATERNION:
        return jc
    return np.concatenate([np.einsum("nkj,njm->nkm", jc[:, :, :4], plus_jacobian(q)), jc[:, :, 4:]], axis=2)


def cross_matrix(v):
    """[v]x on rows: (n, 3, 3)."""
    o = np.zeros(v.shape[0])
    return np.stack([np.stack([o, -v[:, 2], v[:, 1]], axis=1), np.stack([v[:, 2], o, -v[:, 0]], axis=1),
                     np.stack([-v[:, 1], v[:, 0], o], axis=1)], axis=1)


class Evaluator:
    """Cost, residuals, local Jacobian values and gradient of a BAL problem with quaternion cameras, in the layout of
    ceres_hip_bal_evaluate: rows in `row_order`, E cell of row r at 6 r, F cell at 6 n_rows + 2 cw r (row-major 2 x cw);
    state = [3 per point | 10 per camera] (ambient), gradient 3 n_p + cw n_c (tangent)."""

    def __init__(self, model, num_cameras, num_points, camera_index, point_index, observations, row_order, loss=None):
        self.model = model
        self.cw = 10 if model == QUATERNION else 9
        self.nc, self.np_ = int(num_cameras), int(num_points)
        order = np.asarray(row_order)
        self.cam = np.asarray(camera_index)[order].astype(np.int64)
        self.pt = np.asarray(point_index)[order].astype(np.int64)
        self.obs = np.asarray(observations, dtype=np.float64).reshape(-1, 2)[order]
        self.n_rows = self.cam.shape[0]
        self.n_a = 3 * self.np_ + 10 * self.nc
        self.n_t = 3 * self.np_ + self.cw * self.nc
        self.loss = loss   # None: the squared loss; else (kind, a, b, scale)

    def _rows(self, x):
        x = np.asarray(x, dtype=np.float64)
        return x[3 * self.np_:].reshape(-1, 10)[self.cam], x[:3 * self.np_].reshape(-1, 3)[self.pt]

    def cost(self, x):
        r = residual(*self._rows(x), self.obs)
        s = np.sum(r * r, axis=1)
        return 0.5 * float(np.sum(s if self.loss is None else rho(self.loss[0], s, *self.loss[1:])[0]))

    def evaluate(self, x):
        """(cost, residuals, values, gradient)."""
        cams, X = self._rows(x)
        r = residual(cams, X, self.obs)
        jc, jp = ambient_jacobian(cams, X, self.obs)
        jc = local_camera_jacobian(jc, cams[:, :4], self.model)
        s = np.sum(r * r, axis=1)
        if self.loss is None:
            cost = 0.5 * float(np.sum(s))
        else:
            rhos = rho(self.loss[0], s, *self.loss[1:])
            cost = 0.5 * float(np.sum(rhos[0]))
            r, J = correct(r, np.concatenate([jp, jc], axis=2), rhos, s)
            jp, jc = J[:, :, :3], J[:, :, 3:]
        vals = np.concatenate([jp.reshape(-1), jc.reshape(-1)])
        g = np.zeros(self.n_t)
        np.add.at(g[:3 * self.np_].reshape(-1, 3), self.pt, np.einsum("nkm,nk->nm", jp, r))
        np.add.at(g[3 * self.np_:].reshape(-1, self.cw), self.cam, np.einsum("nkm,nk->nm", jc, r))
        return cost, r.reshape(-1), vals, g

    def dense_jacobian(self, vals):
        J = np.zeros((2 * self.n_rows, self.n_t))
        jp = vals[:6 * self.n_rows].reshape(-1, 2, 3)
        jc = vals[6 * self.n_rows:].reshape(-1, 2, self.cw)
        rows = np.arange(self.n_rows)
        for k in range(2):
            for m in range(3):
                J[2 * rows + k, 3 * self.pt + m] = jp[:, k, m]
            for m in range(self.cw):
                J[2 * rows + k, 3 * self.np_ + self.cw * self.cam + m] = jc[:, k, m]
        return J

    def plus(self, x, delta):
        """Evaluator::Plus: x ambient, delta tangent."""
        if self.model == QUATERNION:
            return x + delta
        out = np.array(x, dtype=np.float64)
        out[:3 * self.np_] += delta[:3 * self.np_]
        c = out[3 * self.np_:].reshape(-1, 10)
        d = delta[3 * self.np_:].reshape(-1, 9)
        c[:, :4] = quaternion_plus(c[:, :4], d[:, :3])
        c[:, 4:] += d[:, 3:]
        return out

    def gradient_max_norm(self, x, g):
        """|x - Plus(x, -g)|_inf in ambient coordinates; |g_i| where Plus is Euclidean (as the device computes it)."""
        if self.model == QUATERNION:
            return float(np.max(np.abs(g)))
        gc = g[3 * self.np_:].reshape(-1, 9)
        q = np.asarray(x[3 * self.np_:]).reshape(-1, 10)[:, :4]
        dq = np.abs(q - quaternion_plus(q, -gc[:, :3]))
        return float(max(np.max(np.abs(g[:3 * self.np_])), np.max(np.abs(gc[:, 3:])), np.max(dq)))


DEFAULTS = dict(max_num_iterations=50, jacobi_scaling=1, max_consecutive_invalid_steps=5, initial_trust_region_radius=1e4,
                max_trust_region_radius=1e16, min_trust_region_radius=1e-32, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


def minimize(ev: Evaluator, x0, **opts):
    """TrustRegionMinimizer::Minimize, LEVENBERG_MARQUARDT, monotonic, with the Evaluator's Plus and the manifold's gradient norm; the
    linear solve dense and exact.  Returns (x, summary dict: initial_cost, final_cost, termination_type, iterations: [dict(cost,
    step_is_successful, step_is_valid, trust_region_radius, gradient_max_norm)])."""
    o = dict(DEFAULTS)
    o.update(opts)
    x = np.array(x0, dtype=np.float64)
    radius, decrease_factor = o["initial_trust_region_radius"], 2.0
    reuse_diagonal, one_success, invalid_run, iteration = False, False, 0, 0
    scale = np.ones(ev.n_t)
    st = {}

    def eval_jacobian():
        cost, r, vals, g = ev.evaluate(x)
        J = ev.dense_jacobian(vals)
        if o["jacobi_scaling"] and iteration == 0:
            scale[:] = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        st.update(cost=cost, r=r, Js=J * scale[None, :] if o["jacobi_scaling"] else J, grad_max=ev.gradient_max_norm(x, g))

    eval_jacobian()
    S = dict(initial_cost=st["cost"], termination_type=NO_CONVERGENCE)
    its = [dict(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius, step_is_valid=1, step_is_successful=1)]
    diag = None
    while True:
        if iteration >= o["max_num_iterations"]:
            S["termination_type"] = NO_CONVERGENCE
            break
        if st["grad_max"] <= o["gradient_tolerance"] or radius <= o["min_trust_region_radius"]:
            S["termination_type"] = CONVERGENCE
            break
        iteration += 1
        it = dict(step_is_valid=0, step_is_successful=0)
        Js, r = st["Js"], st["r"]
        if not reuse_diagonal:
            diag = np.clip(np.sum(Js * Js, axis=0), o["min_lm_diagonal"], o["max_lm_diagonal"])
        step = -np.linalg.solve(Js.T @ Js + np.diag(diag / radius), Js.T @ r)
        reuse_diagonal = True
        model = Js @ step
        mcc = -float(np.sum(model * (r + model / 2.0)))
        valid = bool(np.all(np.isfinite(step))) and mcc > 0.0
        it["step_is_valid"] = int(valid)
        if not valid:
            invalid_run += 1
            if invalid_run >= o["max_consecutive_invalid_steps"]:
                S["termination_type"] = FAILURE
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            it.update(cost=st["cost"], gradient_max_norm=st["grad_max"], trust_region_radius=radius)
            its.append(it)
            continue
        invalid_run = 0
        delta = step * scale if o["jacobi_scaling"] else step
        cand = ev.plus(x, delta)
        cand_cost = ev.cost(cand)
        step_norm = float(np.linalg.norm(delta))   # tangent |delta|, ambient |x|
        if one_success and step_norm <= o["parameter_tolerance"] * (float(np.linalg.norm(x)) + o["parameter_tolerance"]):
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        if abs(st["cost"] - cand_cost) <= o["function_tolerance"] * st["cost"]:
            S["termination_type"] = CONVERGENCE
            it.update(cost=st["cost"], trust_region_radius=radius)
            its.append(it)
            break
        rel_dec = (st["cost"] - cand_cost) / mcc
        if rel_dec > o["min_relative_decrease"]:
            x = cand
            one_success = True
            eval_jacobian()
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rel_dec - 1.0) ** 3))
            decrease_factor = 2.0
            reuse_diagonal = False
            it["step_is_successful"] = 1
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
        it.update(cost=st["cost"] if it["step_is_successful"] else cand_cost, gradient_max_norm=st["grad_max"], trust_region_radius=radius)
        its.append(it)
    S["final_cost"] = st["cost"]
    S["iterations"] = its
    return x, S


def synthetic_scene(num_cameras, num_points, num_observations, seed, pixel_noise=0.5, param_noise=0.02):
    """A small BAL-like scene in angle-axis form: (camera_index, point_index, observations (n, 2), cameras (nc, 9), points (np, 3)) —
    cameras looking down -z at points near the origin (every point in front of every camera), observed with pixel noise, the
    parameters then perturbed so that there is something to minimise."""
    rng = np.random.default_rng(seed)
    cams = np.zeros((num_cameras, 9))
    cams[:, :3] = rng.normal(0.0, 0.15, (num_cameras, 3))
    cams[:, 3:5] = rng.normal(0.0, 0.3, (num_cameras, 2))
    cams[:, 5] = -rng.uniform(8.0, 12.0, num_cameras)
    cams[:, 6] = rng.uniform(400.0, 600.0, num_cameras)
    cams[:, 7] = rng.normal(0.0, 1e-2, num_cameras)
    cams[:, 8] = rng.normal(0.0, 1e-3, num_cameras)
    pts = rng.normal(0.0, 1.0, (num_points, 3))
    cam = np.concatenate([np.arange(num_cameras), rng.integers(0, num_cameras, num_observations - num_cameras)]).astype(np.int32)
    pt = np.concatenate([rng.permutation(num_points)[:min(num_points, num_observations)],
                         rng.integers(0, num_points, max(0, num_observations - num_points))])[:num_observations].astype(np.int32)
    q = np.concatenate([angle_axis_to_quaternion(cams[:, :3]), cams[:, 3:]], axis=1)
    obs = residual(q[cam], pts[pt], np.zeros((num_observations, 2))) + rng.normal(0.0, pixel_noise, (num_observations, 2))
    cams_n = cams * (1.0 + rng.normal(0.0, param_noise, cams.shape))
    pts_n = pts + rng.normal(0.0, param_noise, pts.shape)
    return cam, pt, obs, cams_n, pts_n
