// QuaternionManifold's Plus as a device function, shared by every kernel that moves a quaternion camera along a tangent step: the
// trust-region loop's candidate and gradient-norm kernels (kernels_quaternion.hip, kernels_constant.hip) and the line search minimizer's
// trial point (kernels_line_search.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace chip {

// QuaternionPlusImpl (I/manifold.cc): [cos |d|, sin |d| / |d| d] (x) q, the product of include/ceres/rotation.h's QuaternionProduct;
// q itself when |d| is exactly zero
__device__ __forceinline__ void quaternion_plus(const double (&q)[4], double d0, double d1, double d2, double (&out)[4]) {
  const double nd = norm3d(d0, d1, d2);
  if (nd == 0.0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = q[k];
    return;
  }
  const double s = sin(nd) / nd;
  const double z[4] = {cos(nd), s * d0, s * d1, s * d2};
  out[0] = z[0] * q[0] - z[1] * q[1] - z[2] * q[2] - z[3] * q[3];
  out[1] = z[0] * q[1] + z[1] * q[0] + z[2] * q[3] - z[3] * q[2];
  out[2] = z[0] * q[2] - z[1] * q[3] + z[2] * q[0] + z[3] * q[1];
  out[3] = z[0] * q[3] + z[1] * q[2] - z[2] * q[1] + z[3] * q[0];
}

}  // namespace chip
