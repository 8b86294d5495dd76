// The trust-region loop's vector kernels for quaternion-manifold cameras (ceres_hip_bal_create_with_camera,
// CERES_HIP_CAMERA_QUATERNION_MANIFOLD): the state is ambient — [3 per point | q(4) t(3) f k1 k2 per camera] — and the step, the scale and
// the gradient are tangent — 9 per camera — so that Plus and the gradient's max norm are no longer element-wise (bal_candidate_kernel and
// bal_gradient_max_kernel of kernels_evaluator.hip serve the other two camera models).  A translation unit of its own: the sin / cos
// of QuaternionPlus next to the evaluator's kernels changed the register allocation of its robust tile-order instantiations.
#include <hip/hip_runtime.h>

#include "bal_evaluate.h"
#include "device.h"
#include "reduce.h"
#include "quaternion_plus.h"

namespace chip {

namespace {

// bal_candidate_kernel for quaternion-manifold cameras: delta = step .* scale (tangent: 9 per camera), candidate = Plus(x, delta)
// (ambient: 10 per camera, QuaternionManifold on q, Euclidean on the rest).  One item per point coordinate, then one per camera: each
// thread's sums run in a fixed order, so the partials — |x|^2 (ambient) at [b], |delta|^2 (tangent) at [grid + b] — are repeatable.
__global__ __launch_bounds__(kVecBlock) void bal_candidate_quat_kernel(const double* x, const double* step, const double* scale,
                                                                       double* delta, double* cand, int64_t n_points, int64_t n_cameras,
                                                                       double* partials) {
  __shared__ double sh[8];
  double xn = 0, dn = 0;
  const int64_t n_pt = 3 * n_points;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n_pt + n_cameras; i += int64_t(gridDim.x) * kVecBlock) {
    if (i < n_pt) {
      const double d = scale ? step[i] * scale[i] : step[i];
      const double xi = x[i];
      delta[i] = d;
      cand[i] = xi + d;
      xn += xi * xi;
      dn += d * d;
      continue;
    }
    const int64_t t = n_pt + 9 * (i - n_pt), a = n_pt + 10 * (i - n_pt);
    double d[9], q[4], qp[4];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      d[j] = scale ? step[t + j] * scale[t + j] : step[t + j];
      delta[t + j] = d[j];
      dn += d[j] * d[j];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = x[a + k]; xn += q[k] * q[k]; }
    quaternion_plus(q, d[0], d[1], d[2], qp);
#pragma unroll
    for (int k = 0; k < 4; ++k) cand[a + k] = qp[k];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double xi = x[a + 4 + j];
      cand[a + 4 + j] = xi + d[3 + j];
      xn += xi * xi;
    }
  }
  xn = wave_sum(xn); dn = wave_sum(dn);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = xn; sh[4 + (threadIdx.x >> 6)] = dn; }   // (one branch for both: two wave_to_lds change the code)
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = lds_sum4(sh);
    partials[gridDim.x + blockIdx.x] = lds_sum4(sh + 4);
  }
}

// Ceres' gradient_max_norm with quaternion-manifold cameras: |x - Plus(x, -g)|_inf in ambient coordinates (I/trust_region_minimizer.cc:
// 285-302), g = J^T f / scale the gradient of the unscaled problem (tangent).  |g_i| on points, translations and intrinsics; on a
// camera's rotation the four components of q - Plus(q, -g_rot).
__global__ __launch_bounds__(kVecBlock) void bal_gradient_max_quat_kernel(const double* g, const double* scale, const double* x,
                                                                          int64_t n_points, int64_t n_cameras, double* partials) {
  __shared__ double sh[4];
  double m = 0;
  const int64_t n_pt = 3 * n_points;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n_pt + n_cameras; i += int64_t(gridDim.x) * kVecBlock) {
    if (i < n_pt) {
      m = fmax(m, fabs(scale ? g[i] / scale[i] : g[i]));
      continue;
    }
    const int64_t t = n_pt + 9 * (i - n_pt), a = n_pt + 10 * (i - n_pt);
    double gt[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) gt[j] = scale ? g[t + j] / scale[t + j] : g[t + j];
    double q[4], qp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = x[a + k];
    quaternion_plus(q, -gt[0], -gt[1], -gt[2], qp);
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmax(m, fabs(q[k] - qp[k]));
#pragma unroll
    for (int j = 3; j < 9; ++j) m = fmax(m, fabs(gt[j]));
  }
  m = wave_max(m);
  wave_to_lds(m, sh);
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = lds_max4(sh);
}

}  // namespace

hipError_t LaunchBalCandidateQuat(const double* x, const double* step, const double* scale, double* delta, double* cand, int64_t n_points,
                                  int64_t n_cameras, double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(3 * n_points + n_cameras, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(bal_candidate_quat_kernel, dim3(grid), dim3(kVecBlock), 0, stream, x, step, scale, delta, cand, n_points, n_cameras,
                     partials);
  return hipGetLastError();
}

hipError_t LaunchBalGradientMaxQuat(const double* g, const double* scale, const double* x, int64_t n_points, int64_t n_cameras,
                                    double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(3 * n_points + n_cameras, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(bal_gradient_max_quat_kernel, dim3(grid), dim3(kVecBlock), 0, stream, g, scale, x, n_points, n_cameras, partials);
  return hipGetLastError();
}

hipError_t LaunchBalEvaluateQuat(const BalEvalArgs& A, bool jacobian, int grid, hipStream_t stream, int camera_model) {
  const bool robust = A.loss.type != kLossNone;
#define EVAL_QUAT_CASE(CM)                                                                                                        \
  case CM:                                                                                                                        \
    if (jacobian && robust) hipLaunchKernelGGL((bal_evaluate_kernel<true, true, CM>), dim3(grid), dim3(kVecBlock), 0, stream, A);    \
    else if (jacobian) hipLaunchKernelGGL((bal_evaluate_kernel<true, false, CM>), dim3(grid), dim3(kVecBlock), 0, stream, A);       \
    else if (robust) hipLaunchKernelGGL((bal_evaluate_kernel<false, true, CM>), dim3(grid), dim3(kVecBlock), 0, stream, A);         \
    else hipLaunchKernelGGL((bal_evaluate_kernel<false, false, CM>), dim3(grid), dim3(kVecBlock), 0, stream, A);                    \
    return hipGetLastError();
  switch (camera_model) {
    EVAL_QUAT_CASE(kCamQuaternion)
    EVAL_QUAT_CASE(kCamQuaternionManifold)
    default: return hipErrorInvalidValue;
  }
#undef EVAL_QUAT_CASE
}

hipError_t LaunchBalEvaluateConstQuat(const BalEvalConstArgs& A, int grid, hipStream_t stream, int camera_model) {
  const bool robust = A.loss.type != kLossNone;
#define EVAL_QUAT_CONST_CASE(CM)                                                                                                        \
  case CM:                                                                                                                              \
    if (robust) hipLaunchKernelGGL((bal_evaluate_kernel<true, true, CM, true>), dim3(grid), dim3(kVecBlock), 0, stream, A);              \
    else hipLaunchKernelGGL((bal_evaluate_kernel<true, false, CM, true>), dim3(grid), dim3(kVecBlock), 0, stream, A);                    \
    return hipGetLastError();
  switch (camera_model) {
    EVAL_QUAT_CONST_CASE(kCamQuaternion)
    EVAL_QUAT_CONST_CASE(kCamQuaternionManifold)
    default: return hipErrorInvalidValue;
  }
#undef EVAL_QUAT_CONST_CASE
}

}  // namespace chip
