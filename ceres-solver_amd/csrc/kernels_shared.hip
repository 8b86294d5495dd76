// Shared camera intrinsics of the BAL front end (ceres_hip_bal_create_with_shared_intrinsics: one 3-wide parameter block f, k1, k2 per
// group of cameras beside a 6-wide pose block per camera — examples/libmv_bundle_adjuster.cc:697-728).  The state stays ambient, nine
// doubles per angle-axis camera, the intrinsics of a group bit-identical in all its cameras; the step, the scale, delta and the gradient
// are tangent: [points | free cameras' poses | groups].
//
// The evaluator is bal_evaluate_subset_kernel (kernels_subset.hip: the reduced-program form, one thread per row, grid-strided, the same
// cost partials in the same order) with the corrected 2 x 9 camera Jacobian split: columns 0 .. 5 to the pose cell, 6 .. 8 to the group
// cell, each scaled by its own entries of the tangent scale vector.  The intrinsics are read from the row's own camera.  A translation
// unit of its own because instantiations added to an existing unit change the register allocation of the kernels already there
// (bal_evaluate.h).  The cost-only evaluation has no cell to split: it stays LaunchBalEvaluate's.
#include <hip/hip_runtime.h>

#include "device.h"
#include "reduce.h"
#include "robust_loss.h"
#include "snavely.h"

namespace chip {

namespace {

// ROBUST: as bal_evaluate_kernel's (always with Jacobian)
template <bool ROBUST>
__global__ __launch_bounds__(kVecBlock) void bal_evaluate_shared_kernel(BalEvalSharedArgs A) {
  __shared__ double sh[4];
  double cost = 0.0;
  for (int64_t r = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; r < A.n_rows; r += int64_t(gridDim.x) * kVecBlock) {
    const int c = A.row_cam[r], p = A.row_pt[r];
    const double2 o = A.row_obs[r];
    double cam[9], X[3], res[2], jc[18], jp[6];
    const double* cs = A.state + A.cam_base + 9 * int64_t(c);
    const double* ps = A.state + 3 * int64_t(p);
#pragma unroll
    for (int i = 0; i < 9; ++i) cam[i] = cs[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = ps[i];
    snavely<true>(cam, X, o.x, o.y, res, jc, jp);
    if constexpr (ROBUST) {
      const double sq = res[0] * res[0] + res[1] * res[1];
      double rho[3];
      robust_rho(A.loss, sq, rho);
      cost += 0.5 * rho[0];
      const RobustCorrector C = robust_corrector(sq, rho);
      robust_correct_jacobian<9>(C, res[0], res[1], jc);
      robust_correct_jacobian<3>(C, res[0], res[1], jp);
      res[0] *= C.residual_scaling; res[1] *= C.residual_scaling;
    } else {
      cost += 0.5 * (res[0] * res[0] + res[1] * res[1]);
    }
    if (A.residuals) reinterpret_cast<double2*>(A.residuals)[r] = make_double2(res[0], res[1]);
    const int fpos = A.row_fpos[r], gpos = A.row_gpos[r], scam = A.row_scam[r], sgrp = A.row_sgrp[r], spt = A.row_spt[r];
    if (spt >= 0) {
      if (A.scale) {
        const double* sp = A.scale + spt;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double v = sp[j]; jp[j] *= v; jp[3 + j] *= v; }
      }
      double2* e = reinterpret_cast<double2*>(A.values + 6 * r);   // (every row has an E cell: its place is the row's)
#pragma unroll
      for (int j = 0; j < 3; ++j) e[j] = make_double2(jp[2 * j], jp[2 * j + 1]);
    }
    // the split: every index below is a constant in the unrolled body (jc is 2 x 9 row-major)
    if (fpos >= 0) {   // the pose cell, 2 x 6 row-major: 96 B, 16-byte aligned
      double f[12];
#pragma unroll
      for (int j = 0; j < 6; ++j) { f[j] = jc[j]; f[6 + j] = jc[9 + j]; }
      if (A.scale) {
        const double* sc = A.scale + scam;
#pragma unroll
        for (int j = 0; j < 6; ++j) { const double v = sc[j]; f[j] *= v; f[6 + j] *= v; }
      }
      double2* fo = reinterpret_cast<double2*>(A.values + fpos);
#pragma unroll
      for (int j = 0; j < 6; ++j) fo[j] = make_double2(f[2 * j], f[2 * j + 1]);
    }
    {   // the group cell, 2 x 3 row-major: 48 B, 16-byte aligned
      double g[6];
#pragma unroll
      for (int j = 0; j < 3; ++j) { g[j] = jc[6 + j]; g[3 + j] = jc[15 + j]; }
      if (A.scale) {
        const double* sg = A.scale + sgrp;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double v = sg[j]; g[j] *= v; g[3 + j] *= v; }
      }
      double2* go = reinterpret_cast<double2*>(A.values + gpos);
#pragma unroll
      for (int j = 0; j < 3; ++j) go[j] = make_double2(g[2 * j], g[2 * j + 1]);
    }
  }
  cost = wave_sum(cost);
  wave_to_lds(cost, sh);
  __syncthreads();
  if (threadIdx.x == 0) A.partials[blockIdx.x] = lds_sum4(sh);
}

// delta = step .* scale (tangent), cand = Plus(x, delta); one work item per block — n_points points, then n_cameras cameras — each
// thread's sums in a fixed order (bal_candidate_free_kernel's scheme and partials: |x|^2 at [b], |delta|^2 at [grid + b]).  The product
// is rounded before it is added (no contraction): delta holds exactly what every member of a group adds, and all members of a group add
// the same double to the same bits.  A group's |x|^2 and |delta|^2 terms come from its first camera alone, a constant pose adds nothing.
__global__ __launch_bounds__(kVecBlock) void bal_candidate_shared_kernel(BalSharedCameras B, const double* x, const double* step, const double* scale,
                                                                         double* delta, double* cand, double* partials) {
  __shared__ double sh[8];
  double xn = 0, dn = 0;
  const int64_t n = B.n_points + B.n_cameras;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    if (i < B.n_points) {
      const int64_t t = 3 * i;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double d = scale ? __dmul_rn(step[t + j], scale[t + j]) : step[t + j];
        const double xi = x[t + j];
        delta[t + j] = d;
        cand[t + j] = __dadd_rn(xi, d);
        xn += xi * xi;
        dn += d * d;
      }
      continue;
    }
    const int64_t c = i - B.n_points, a = 3 * B.n_points + 9 * c;
    const int tp = B.cam_pose[c], tg = B.cam_group[c];
    const bool first = B.cam_first[c] != 0;
    if (tp >= 0) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double d = scale ? __dmul_rn(step[tp + j], scale[tp + j]) : step[tp + j];
        const double xi = x[a + j];
        delta[tp + j] = d;
        cand[a + j] = __dadd_rn(xi, d);
        xn += xi * xi;
        dn += d * d;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) cand[a + j] = x[a + j];   // (the caller's bits, a -0.0 included)
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double d = scale ? __dmul_rn(step[tg + j], scale[tg + j]) : step[tg + j];
      const double xi = x[a + 6 + j];
      cand[a + 6 + j] = __dadd_rn(xi, d);
      if (first) {
        delta[tg + j] = d;
        xn += xi * xi;
        dn += d * d;
      }
    }
  }
  xn = wave_sum(xn); dn = wave_sum(dn);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = xn; sh[4 + (threadIdx.x >> 6)] = dn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = lds_sum4(sh);
    partials[gridDim.x + blockIdx.x] = lds_sum4(sh + 4);
  }
}

}  // namespace

hipError_t LaunchBalEvaluateShared(const BalEvalSharedArgs& A, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(A.n_rows, kMaxEvalGrid);
  *nparts = grid;
  if (!A.row_fpos || !A.row_gpos || !A.row_scam || !A.row_sgrp || !A.row_spt || !A.values) return hipErrorInvalidValue;
  if (A.loss.type != kLossNone) hipLaunchKernelGGL(bal_evaluate_shared_kernel<true>, dim3(grid), dim3(kVecBlock), 0, stream, A);
  else hipLaunchKernelGGL(bal_evaluate_shared_kernel<false>, dim3(grid), dim3(kVecBlock), 0, stream, A);
  return hipGetLastError();
}

hipError_t LaunchBalCandidateShared(const BalSharedCameras& B, const double* x, const double* step, const double* scale, double* delta,
                                    double* cand, double* partials, int* nparts, hipStream_t stream) {
  if (!B.cam_pose || !B.cam_group || !B.cam_first) return hipErrorInvalidValue;
  const int grid = vec_grid(B.n_points + B.n_cameras, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(bal_candidate_shared_kernel, dim3(grid), dim3(kVecBlock), 0, stream, B, x, step, scale, delta, cand, partials);
  return hipGetLastError();
}

}  // namespace chip
