// snavely.h — the Snavely reprojection residual and its analytic Jacobian for one observation, shared by the
// evaluator kernels (kernels_evaluator.hip) and the camera-major preconditioner pass that evaluates its F cells on the fly
// (kernels_bal.inc, <2,3,9> shape).  Formula: examples/snavely_reprojection_error.h:53-105 with AngleAxisRotatePoint,
// include/ceres/rotation.h:864-905; the oracle differentiates the same formula with dual numbers (oracle/bal_harness.cc).
#pragma once
#include <hip/hip_runtime.h>

namespace chip {

// Residual (and, JAC, the Jacobian) of one observation.  cam = [angle-axis(3) t(3) f k1 k2].
// jc = d res / d cam (2x9 row-major), jp = d res / d point (2x3 row-major).
template <bool JAC>
__device__ __forceinline__ void snavely(const double (&cam)[9], const double (&X)[3], double ox, double oy,
                                        double (&res)[2], double (&jc)[18], double (&jp)[6]) {
  const double a0 = cam[0], a1 = cam[1], a2 = cam[2];
  const double theta2 = a0 * a0 + a1 * a1 + a2 * a2;
  double P[3];
  double R[9];      // d P / d X
  double dPa[9];    // d P / d angle-axis, column j = derivative w.r.t. a_j, stored [row * 3 + j]
  if (theta2 != 0.0) {
    // Rodrigues: P = X cos + (w x X) sin + w (w.X)(1 - cos), w = a / theta   (include/ceres/rotation.h:864-905)
    const double theta = sqrt(theta2);
    const double c = cos(theta), s = sin(theta), inv = 1.0 / theta;
    const double w[3] = {a0 * inv, a1 * inv, a2 * inv};
    const double wxX[3] = {w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]};
    const double wdX = w[0] * X[0] + w[1] * X[1] + w[2] * X[2];
    const double omc = 1.0 - c;
    const double tmp = wdX * omc;
#pragma unroll
    for (int i = 0; i < 3; ++i) P[i] = X[i] * c + wxX[i] * s + w[i] * tmp;
    if constexpr (JAC) {
      // R = c I + s [w]x + (1 - c) w w^T
      R[0] = c + omc * w[0] * w[0];         R[1] = -s * w[2] + omc * w[0] * w[1];  R[2] = s * w[1] + omc * w[0] * w[2];
      R[3] = s * w[2] + omc * w[1] * w[0];  R[4] = c + omc * w[1] * w[1];          R[5] = -s * w[0] + omc * w[1] * w[2];
      R[6] = -s * w[1] + omc * w[2] * w[0]; R[7] = s * w[0] + omc * w[2] * w[1];   R[8] = c + omc * w[2] * w[2];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // d theta / d a_j = w_j ;  d w / d a_j = (e_j - w w_j) / theta
        const double wj = w[j];
        double dw[3] = {-w[0] * wj * inv, -w[1] * wj * inv, -w[2] * wj * inv};
        dw[j] += inv;
        const double dwxX[3] = {dw[1] * X[2] - dw[2] * X[1], dw[2] * X[0] - dw[0] * X[2], dw[0] * X[1] - dw[1] * X[0]};
        const double dwdX = dw[0] * X[0] + dw[1] * X[1] + dw[2] * X[2];
        const double dtmp = dwdX * omc + wdX * s * wj;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          dPa[i * 3 + j] = -X[i] * s * wj + dwxX[i] * s + wxX[i] * c * wj + dw[i] * tmp + w[i] * dtmp;
      }
    }
  } else {
    // first-order Taylor branch: P = X + a x X
    P[0] = X[0] + (a1 * X[2] - a2 * X[1]);
    P[1] = X[1] + (a2 * X[0] - a0 * X[2]);
    P[2] = X[2] + (a0 * X[1] - a1 * X[0]);
    if constexpr (JAC) {
      R[0] = 1.0; R[1] = -a2; R[2] = a1;
      R[3] = a2;  R[4] = 1.0; R[5] = -a0;
      R[6] = -a1; R[7] = a0;  R[8] = 1.0;
      // d (a x X) / d a_j = e_j x X
      dPa[0] = 0.0;   dPa[1] = X[2];  dPa[2] = -X[1];
      dPa[3] = -X[2]; dPa[4] = 0.0;   dPa[5] = X[0];
      dPa[6] = X[1];  dPa[7] = -X[0]; dPa[8] = 0.0;
    }
  }
  const double p0 = P[0] + cam[3], p1 = P[1] + cam[4], p2 = P[2] + cam[5];
  const double iz = 1.0 / p2;
  const double xp = -p0 * iz, yp = -p1 * iz;
  const double f = cam[6], k1 = cam[7], k2 = cam[8];
  const double r2 = xp * xp + yp * yp;
  const double dist = 1.0 + r2 * (k1 + k2 * r2);
  res[0] = f * dist * xp - ox;
  res[1] = f * dist * yp - oy;
  if constexpr (JAC) {
    const double g = k1 + 2.0 * k2 * r2;  // d dist / d r2
    // A = d res / d (xp, yp)
    const double A00 = f * (dist + 2.0 * g * xp * xp), A01 = f * 2.0 * g * xp * yp;
    const double A10 = A01, A11 = f * (dist + 2.0 * g * yp * yp);
    // d (xp, yp) / d p = [-1/z 0 x/z^2 ; 0 -1/z y/z^2] = [-iz 0 -xp iz ; 0 -iz -yp iz]
    const double J00 = -A00 * iz, J01 = -A01 * iz, J02 = -(A00 * xp + A01 * yp) * iz;
    const double J10 = -A10 * iz, J11 = -A11 * iz, J12 = -(A10 * xp + A11 * yp) * iz;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      jp[j] = J00 * R[j] + J01 * R[3 + j] + J02 * R[6 + j];
      jp[3 + j] = J10 * R[j] + J11 * R[3 + j] + J12 * R[6 + j];
      jc[j] = J00 * dPa[j] + J01 * dPa[3 + j] + J02 * dPa[6 + j];
      jc[9 + j] = J10 * dPa[j] + J11 * dPa[3 + j] + J12 * dPa[6 + j];
    }
    jc[3] = J00; jc[4] = J01; jc[5] = J02;
    jc[12] = J10; jc[13] = J11; jc[14] = J12;
    jc[6] = dist * xp;          jc[15] = dist * yp;
    jc[7] = f * r2 * xp;        jc[16] = f * r2 * yp;
    jc[8] = f * r2 * r2 * xp;   jc[17] = f * r2 * r2 * yp;
  }
}

// The same residual with a quaternion camera, cam = [q_w q_x q_y q_z | t(3) | f k1 k2] (SnavelyReprojectionErrorWithQuaternions,
// examples/snavely_reprojection_error.h:110-160): QuaternionRotatePoint — u = q / |q|, then UnitQuaternionRotatePoint's
// P = X + 2 w (v x X) + v x (2 v x X), v = (u_x, u_y, u_z) (include/ceres/rotation.h:787-824) — and the projection above.
// !MANIFOLD: jc = d res / d cam, 2 x 10 (Euclidean Plus on all ten).  MANIFOLD: jc = (d res / d cam) x PlusJacobian, 2 x 9 — with
// ProductManifold<QuaternionManifold, EuclideanManifold<6>> (I/manifold.cc QuaternionPlusJacobianImpl on q, identity on the rest).
// The columns of QuaternionPlusJacobian(q) = |q| QuaternionPlusJacobian(u) are orthogonal to u, and d P / d q = (d P / d u)(I - u u^T) / |q|,
// so the product is d P / d u along the tangent of the unit sphere: d R(exp(delta) u) X / d delta = -2 [R(u) X]x, whatever |q| is.
template <bool JAC, bool MANIFOLD>
__device__ __forceinline__ void snavely_quat(const double (&cam)[10], const double (&X)[3], double ox, double oy, double (&res)[2],
                                             double (&jc)[MANIFOLD ? 18 : 20], double (&jp)[6]) {
  constexpr int W = MANIFOLD ? 9 : 10;   // Jacobian columns per camera
  const double scale = 1.0 / sqrt(cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2] + cam[3] * cam[3]);
  const double w = scale * cam[0], v[3] = {scale * cam[1], scale * cam[2], scale * cam[3]};
  double uv[3] = {v[1] * X[2] - v[2] * X[1], v[2] * X[0] - v[0] * X[2], v[0] * X[1] - v[1] * X[0]};
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  double P[3] = {X[0] + w * uv[0], X[1] + w * uv[1], X[2] + w * uv[2]};
  P[0] += v[1] * uv[2] - v[2] * uv[1];
  P[1] += v[2] * uv[0] - v[0] * uv[2];
  P[2] += v[0] * uv[1] - v[1] * uv[0];
  const double p0 = P[0] + cam[4], p1 = P[1] + cam[5], p2 = P[2] + cam[6];
  const double iz = 1.0 / p2;
  const double xp = -p0 * iz, yp = -p1 * iz;
  const double f = cam[7], k1 = cam[8], k2 = cam[9];
  const double r2 = xp * xp + yp * yp;
  const double dist = 1.0 + r2 * (k1 + k2 * r2);
  res[0] = f * dist * xp - ox;
  res[1] = f * dist * yp - oy;
  if constexpr (JAC) {
    const double g = k1 + 2.0 * k2 * r2;
    const double A00 = f * (dist + 2.0 * g * xp * xp), A01 = f * 2.0 * g * xp * yp;
    const double A10 = A01, A11 = f * (dist + 2.0 * g * yp * yp);
    const double J[2][3] = {{-A00 * iz, -A01 * iz, -(A00 * xp + A01 * yp) * iz}, {-A10 * iz, -A11 * iz, -(A10 * xp + A11 * yp) * iz}};
    // d P / d X of the formula: I + 2 w [v]x + 2 [v]x^2 = (1 - 2 |v|^2) I + 2 w [v]x + 2 v v^T
    const double d = 1.0 - 2.0 * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double R[9] = {d + 2.0 * v[0] * v[0],      2.0 * (v[0] * v[1] - w * v[2]), 2.0 * (v[0] * v[2] + w * v[1]),
                         2.0 * (v[1] * v[0] + w * v[2]), d + 2.0 * v[1] * v[1],      2.0 * (v[1] * v[2] - w * v[0]),
                         2.0 * (v[2] * v[0] - w * v[1]), 2.0 * (v[2] * v[1] + w * v[0]), d + 2.0 * v[2] * v[2]};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int j = 0; j < 3; ++j) jp[3 * k + j] = J[k][0] * R[j] + J[k][1] * R[3 + j] + J[k][2] * R[6 + j];
      if constexpr (MANIFOLD) {
        // J_k (-2 [P]x), P the rotated point: column j is J_k . (-2 P x e_j) = 2 (P x J_k)_j
        jc[W * k + 0] = 2.0 * (P[1] * J[k][2] - P[2] * J[k][1]);
        jc[W * k + 1] = 2.0 * (P[2] * J[k][0] - P[0] * J[k][2]);
        jc[W * k + 2] = 2.0 * (P[0] * J[k][1] - P[1] * J[k][0]);
      } else {
        // G = d P / d u: d/dw = 2 v x X = uv; d/dv = -2 w [X]x + 2 (v.X) I + 2 v X^T - 4 X v^T.  Row k of d res / d q is then
        // (a - (a.u) u^T) scale with a = J_k G (a 4-vector); (J_k [X]x)_m = J_k . (X x e_m) = (J_k x X)_m.
        const double vX = v[0] * X[0] + v[1] * X[1] + v[2] * X[2];
        const double jX = J[k][0] * X[0] + J[k][1] * X[1] + J[k][2] * X[2];
        const double jv = J[k][0] * v[0] + J[k][1] * v[1] + J[k][2] * v[2];
        const double jxX[3] = {J[k][1] * X[2] - J[k][2] * X[1], J[k][2] * X[0] - J[k][0] * X[2], J[k][0] * X[1] - J[k][1] * X[0]};
        double a[4];
        a[0] = J[k][0] * uv[0] + J[k][1] * uv[1] + J[k][2] * uv[2];
#pragma unroll
        for (int m = 0; m < 3; ++m) a[1 + m] = -2.0 * w * jxX[m] + 2.0 * vX * J[k][m] + 2.0 * jv * X[m] - 4.0 * jX * v[m];
        const double au = a[0] * w + a[1] * v[0] + a[2] * v[1] + a[3] * v[2];
        jc[W * k + 0] = (a[0] - au * w) * scale;
#pragma unroll
        for (int m = 0; m < 3; ++m) jc[W * k + 1 + m] = (a[1 + m] - au * v[m]) * scale;
      }
      constexpr int o = MANIFOLD ? 3 : 4;   // translation, then f k1 k2
#pragma unroll
      for (int j = 0; j < 3; ++j) jc[W * k + o + j] = J[k][j];
      const double pk = k == 0 ? xp : yp;
      jc[W * k + o + 3] = dist * pk;
      jc[W * k + o + 4] = f * r2 * pk;
      jc[W * k + o + 5] = f * r2 * r2 * pk;
    }
  }
}

}  // namespace chip
