// robust_loss.h — the robust losses of the BAL front end and the Corrector that applies one to a 2-row residual block, on the device
// (SURVEY.md §8 f4).  Shared by the evaluator kernels (kernels_evaluator.hip) and the camera-major pass that evaluates its F cells
// (kernels_bal.inc, <2,3,9> shape), so that every place a Jacobian value of the problem is produced applies the same statements.
//
//   rho(s), rho'(s), rho''(s) of s = |r|^2          include/ceres/loss_function.h:131-330, I/loss_function.cc:46-175
//   cost = rho(s) / 2; J corrected before r, with the uncorrected r    I/residual_block.cc:161-195
//   the Corrector (Triggs correction)                                  I/corrector.cc:41-135
//
// The loss type is a kernel argument: wave-uniform, so the selection below is a scalar branch.  Whether a loss is set at all is a
// template parameter of the kernels (their squared-loss instantiations are unchanged).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device.h"

namespace chip {

// rho[0..2] at s >= 0.  L's constants are the ones the reference's constructors derive (LossParams, device.h).
__device__ __forceinline__ void robust_rho(const LossParams& L, double s, double (&rho)[3]) {
  switch (L.type) {
    case kLossHuber:   // a, b = a^2
      if (s > L.b) {
        const double r = sqrt(s);
        rho[0] = 2.0 * L.a * r - L.b;
        rho[1] = fmax(DBL_MIN, L.a / r);
        rho[2] = -rho[1] / (2.0 * s);
      } else {
        rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
      }
      break;
    case kLossSoftLOne: {   // b = a^2, c = 1 / b
      const double sum = 1.0 + s * L.c;
      const double tmp = sqrt(sum);
      rho[0] = 2.0 * L.b * (tmp - 1.0);
      rho[1] = fmax(DBL_MIN, 1.0 / tmp);
      rho[2] = -(L.c * rho[1]) / (2.0 * sum);
      break;
    }
    case kLossCauchy: {   // b = a^2, c = 1 / b
      const double sum = 1.0 + s * L.c;
      const double inv = 1.0 / sum;
      rho[0] = L.b * log(sum);
      rho[1] = fmax(DBL_MIN, inv);
      rho[2] = -L.c * (inv * inv);
      break;
    }
    case kLossArctan: {   // a, b = 1 / a^2
      const double sum = 1.0 + s * s * L.b;
      const double inv = 1.0 / sum;
      rho[0] = L.a * atan2(s, L.a);
      rho[1] = fmax(DBL_MIN, inv);
      rho[2] = -2.0 * s * L.b * (inv * inv);
      break;
    }
    case kLossTolerant: {   // a, b, c = b ln(1 + e^(-a / b))
      const double x = (s - L.a) / L.b;
      if (x > 36.7) {   // ln(2^53): 1 + e^x == e^x in doubles, and e^x may overflow
        rho[0] = s - L.a - L.c; rho[1] = 1.0; rho[2] = 0.0;
      } else {
        const double e_x = exp(x);
        rho[0] = L.b * log(1.0 + e_x) - L.c;
        rho[1] = fmax(DBL_MIN, e_x / (1.0 + e_x));
        rho[2] = 0.5 / (L.b * (1.0 + cosh(x)));
      }
      break;
    }
    case kLossTukey:   // b = a^2
      if (s <= L.b) {
        const double v = 1.0 - s / L.b, v2 = v * v;
        rho[0] = L.b / 3.0 * (1.0 - v2 * v);
        rho[1] = v2;
        rho[2] = -2.0 / L.b * v;
      } else {
        rho[0] = L.b / 3.0; rho[1] = 0.0; rho[2] = 0.0;
      }
      break;
    default:   // kLossTrivial
      rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
      break;
  }
  // ScaledLoss
  rho[0] *= L.k; rho[1] *= L.k; rho[2] *= L.k;
}

// The Corrector of one residual block at s = |r|^2.  s == 0 or rho'' <= 0: J and r are only scaled by sqrt(rho'); otherwise
// alpha = 1 - sqrt(1 + 2 s rho'' / rho'), r~ = sqrt(rho') / (1 - alpha) r, J~ = sqrt(rho') (J - (alpha / s) r (r^T J)).
struct RobustCorrector {
  double sqrt_rho1, residual_scaling, alpha_sq_norm;
};
__device__ __forceinline__ RobustCorrector robust_corrector(double s, const double (&rho)[3]) {
  RobustCorrector C;
  C.sqrt_rho1 = sqrt(rho[1]);
  if (s == 0.0 || rho[2] <= 0.0) {
    C.residual_scaling = C.sqrt_rho1;
    C.alpha_sq_norm = 0.0;
  } else {
    const double alpha = 1.0 - sqrt(1.0 + 2.0 * s * rho[2] / rho[1]);
    C.residual_scaling = C.sqrt_rho1 / (1.0 - alpha);
    C.alpha_sq_norm = alpha / s;
  }
  return C;
}

// J~ of a 2 x N block stored row-major (j[0 .. N) row 0, j[N .. 2N) row 1), from the UNCORRECTED residual (r0, r1).  With
// alpha_sq_norm == 0 this is exactly the plain scaling by sqrt(rho'): the subtracted term is a signed zero.
template <int N>
__device__ __forceinline__ void robust_correct_jacobian(const RobustCorrector& C, double r0, double r1, double (&j)[2 * N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double rtj = r0 * j[k] + r1 * j[N + k];
    j[k] = C.sqrt_rho1 * (j[k] - C.alpha_sq_norm * r0 * rtj);
    j[N + k] = C.sqrt_rho1 * (j[N + k] - C.alpha_sq_norm * r1 * rtj);
  }
}

}  // namespace chip
