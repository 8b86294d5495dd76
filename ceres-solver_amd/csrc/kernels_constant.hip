// The trust-region loop's vector kernels on a REDUCED program (ceres_hip_bal_create_with_constant_blocks: Problem::SetParameterBlockConstant,
// Program::RemoveFixedBlocks — I/program.cc:309-410).  The state stays ambient and full — [3 per point | cs per camera], constant blocks
// included, read and never written — while the step, the scale, delta and the gradient are the reduced program's tangent vectors:
// [3 per free point | cw per free camera].  So Plus scatters: one work item per FREE block (its first double in the full state comes
// from a list), each thread's sums in a fixed order — the partials are repeatable, as in bal_candidate_kernel / bal_candidate_quat_kernel.
// |x|^2 runs over the free blocks only: Ceres' x_norm is the reduced program's state (I/trust_region_minimizer.cc:127-140).
#include <hip/hip_runtime.h>

#include "device.h"
#include "reduce.h"
#include "quaternion_plus.h"

namespace chip {

namespace {

// CM: the camera model — SW state doubles, CW tangent entries per camera; the manifold's Plus on q, x + delta everywhere else
template <int CM>
__global__ __launch_bounds__(kVecBlock) void bal_candidate_free_kernel(BalFreeBlocks B, const double* x, const double* step, const double* scale,
                                                                       double* delta, double* cand, double* partials) {
  constexpr int SW = CM == kCamAngleAxis ? 9 : 10;
  constexpr int CW = CM == kCamQuaternion ? 10 : 9;
  __shared__ double sh[8];
  double xn = 0, dn = 0;
  const int64_t nfp = B.n_free_points, n = nfp + B.n_free_cameras;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    const int64_t a = B.block[i];
    if (i < nfp) {
      const int64_t t = 3 * i;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double d = scale ? step[t + j] * scale[t + j] : step[t + j];
        const double xi = x[a + j];
        delta[t + j] = d;
        cand[a + j] = xi + d;
        xn += xi * xi;
        dn += d * d;
      }
      continue;
    }
    const int64_t t = 3 * nfp + CW * (i - nfp);
    double d[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) {
      d[j] = scale ? step[t + j] * scale[t + j] : step[t + j];
      delta[t + j] = d[j];
      dn += d[j] * d[j];
    }
    if constexpr (CM == kCamQuaternionManifold) {
      double q[4], qp[4];
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
    } else {
      static_assert(CM == kCamQuaternionManifold || SW == CW, "Euclidean cameras: tangent = ambient");
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        const double xi = x[a + j];
        cand[a + j] = xi + d[j];
        xn += xi * xi;
      }
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

// bal_gradient_max_quat_kernel over the free blocks
__global__ __launch_bounds__(kVecBlock) void bal_gradient_max_quat_free_kernel(BalFreeBlocks B, const double* g, const double* scale, const double* x,
                                                                               double* partials) {
  __shared__ double sh[4];
  double m = 0;
  const int64_t nfp = B.n_free_points, n = nfp + B.n_free_cameras;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    if (i < nfp) {
#pragma unroll
      for (int j = 0; j < 3; ++j) m = fmax(m, fabs(scale ? g[3 * i + j] / scale[3 * i + j] : g[3 * i + j]));
      continue;
    }
    const int64_t t = 3 * nfp + 9 * (i - nfp), a = B.block[i];
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

hipError_t LaunchBalCandidateFree(const BalFreeBlocks& B, int camera_model, const double* x, const double* step, const double* scale,
                                  double* delta, double* cand, double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(B.n_free_points + B.n_free_cameras, kMaxVecGrid);
  *nparts = grid;
  switch (camera_model) {
    case kCamAngleAxis:
      hipLaunchKernelGGL((bal_candidate_free_kernel<kCamAngleAxis>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, step, scale, delta, cand, partials);
      break;
    case kCamQuaternion:
      hipLaunchKernelGGL((bal_candidate_free_kernel<kCamQuaternion>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, step, scale, delta, cand, partials);
      break;
    case kCamQuaternionManifold:
      hipLaunchKernelGGL((bal_candidate_free_kernel<kCamQuaternionManifold>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, step, scale, delta, cand,
                         partials);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchBalGradientMaxQuatFree(const BalFreeBlocks& B, const double* g, const double* scale, const double* x, double* partials,
                                        int* nparts, hipStream_t stream) {
  const int grid = vec_grid(B.n_free_points + B.n_free_cameras, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(bal_gradient_max_quat_free_kernel, dim3(grid), dim3(kVecBlock), 0, stream, B, g, scale, x, partials);
  return hipGetLastError();
}

}  // namespace chip
