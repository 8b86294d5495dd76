// Fixed camera intrinsics of the BAL front end (ceres_hip_bal_create_with_fixed_intrinsics: SubsetManifold(9, {6, 7, 8} or a subset) on
// every camera block — include/ceres/manifold.h; I/residual_block.cc:161-195).  The state stays ambient, nine doubles per angle-axis
// camera; the step, the scale, delta and the gradient are tangent: the camera's free coordinates in ascending index, CW = 6, 7 or 8 of
// them.  PlusJacobian is a selection, so the local Jacobian is the ambient one with the marked columns removed — after the Corrector
// (it acts per column), before the Jacobi scale (the scale vector is tangent).
//
// The evaluator is bal_evaluate_kernel (bal_evaluate.h: one thread per observation, grid-strided, the same cost partials in the same
// order) with the F cell narrowed; a translation unit of its own because instantiations added to an existing unit change the register
// allocation of the kernels already there (bal_evaluate.h).  MASK is a template parameter — bit k: coordinate 6 + k is constant — so
// every register index is static: seven masks x {squared loss, robust}.  Only the reduced-program form exists (BalEvalConstArgs: a
// row's cells and scale entries come from row_fpos / row_scam / row_spt); a handle without constant blocks runs it on the identity
// reduction.  The form that derives those positions from the row's camera and point holds both across the projection and allocates
// 126 / 186 VGPRs, two more than bal_evaluate_kernel<true, ., kCamAngleAxis, false>; this one 120 / 180, what the CONST instantiations
// use — at 12 more bytes read per row beside the 160 to 192 it writes.  The cost-only evaluation has no columns to remove: it stays
// LaunchBalEvaluate's.
#include <hip/hip_runtime.h>

#include "device.h"
#include "reduce.h"
#include "robust_loss.h"
#include "snavely.h"

namespace chip {

namespace {

constexpr bool subset_is_free(int mask, int j) { return j < 6 || !((mask >> (j - 6)) & 1); }
constexpr int subset_width(int mask) { return 9 - (mask & 1) - ((mask >> 1) & 1) - ((mask >> 2) & 1); }

// ROBUST: as bal_evaluate_kernel's (always with Jacobian, always CONST)
template <bool ROBUST, int MASK>
__global__ __launch_bounds__(kVecBlock) void bal_evaluate_subset_kernel(BalEvalConstArgs A) {
  constexpr int CW = subset_width(MASK);
  static_assert(MASK >= 1 && MASK <= 7, "a non-empty subset of the three intrinsics");
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
    // the column removal: fully unrolled, k is a constant in every copy of the body
    double f[2 * CW];
    {
      int k = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        if (subset_is_free(MASK, j)) { f[k] = jc[j]; f[CW + k] = jc[9 + j]; ++k; }
      }
    }
    const int fpos = A.row_fpos[r], scam = A.row_scam[r], spt = A.row_spt[r];
    if (spt >= 0) {
      if (A.scale) {
        const double* sp = A.scale + spt;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double v = sp[j]; jp[j] *= v; jp[3 + j] *= v; }
      }
      double2* e = reinterpret_cast<double2*>(A.values + 6 * r);   // (rows with an E cell come first: its place is the row's)
#pragma unroll
      for (int j = 0; j < 3; ++j) e[j] = make_double2(jp[2 * j], jp[2 * j + 1]);
    }
    if (fpos >= 0) {
      if (A.scale) {
        const double* sc = A.scale + scam;
#pragma unroll
        for (int j = 0; j < CW; ++j) { const double v = sc[j]; f[j] *= v; f[CW + j] *= v; }
      }
      double2* fo = reinterpret_cast<double2*>(A.values + fpos);   // 96, 112 or 128 B per cell, 16-byte aligned
#pragma unroll
      for (int j = 0; j < CW; ++j) fo[j] = make_double2(f[2 * j], f[2 * j + 1]);
    }
  }
  cost = wave_sum(cost);
  wave_to_lds(cost, sh);
  __syncthreads();
  if (threadIdx.x == 0) A.partials[blockIdx.x] = lds_sum4(sh);
}

// delta = step .* scale (tangent), cand = x with delta added on the free coordinates, the marked ones copied; one work item per free
// block, each thread's sums in a fixed order (bal_candidate_free_kernel's scheme and partials: |x|^2 over the ambient doubles of the
// free blocks — marked coordinates included: the block stays in the program with all nine — at [b], |delta|^2 at [grid + b]).
// LIST: the free blocks come from B.block (a reduced program); !LIST: every block is free, block i starts where it always did.
template <bool LIST>
__global__ __launch_bounds__(kVecBlock) void bal_candidate_subset_kernel(BalFreeBlocks B, int mask, int cw, int64_t n_points, const double* x,
                                                                         const double* step, const double* scale, double* delta, double* cand,
                                                                         double* partials) {
  __shared__ double sh[8];
  double xn = 0, dn = 0;
  const int64_t nfp = B.n_free_points, n = nfp + B.n_free_cameras;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    if (i < nfp) {
      const int64_t a = LIST ? B.block[i] : 3 * i, t = 3 * i;
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
    const int64_t a = LIST ? B.block[i] : 3 * n_points + 9 * (i - nfp);
    int64_t t = 3 * nfp + cw * (i - nfp);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const double xi = x[a + j];
      xn += xi * xi;
      if (j >= 6 && ((mask >> (j - 6)) & 1)) { cand[a + j] = xi; continue; }
      const double d = scale ? step[t] * scale[t] : step[t];
      delta[t] = d;
      cand[a + j] = xi + d;
      dn += d * d;
      ++t;
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

template <int MASK>
void launch_subset(const BalEvalConstArgs& A, int grid, hipStream_t stream) {
  if (A.loss.type != kLossNone) hipLaunchKernelGGL((bal_evaluate_subset_kernel<true, MASK>), dim3(grid), dim3(kVecBlock), 0, stream, A);
  else hipLaunchKernelGGL((bal_evaluate_subset_kernel<false, MASK>), dim3(grid), dim3(kVecBlock), 0, stream, A);
}

}  // namespace

hipError_t LaunchBalEvaluateSubset(const BalEvalConstArgs& A, int mask, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(A.n_rows, kMaxEvalGrid);
  *nparts = grid;
  if (!A.row_fpos || !A.row_scam || !A.row_spt || !A.values) return hipErrorInvalidValue;
  switch (mask) {
    case 1: launch_subset<1>(A, grid, stream); break;
    case 2: launch_subset<2>(A, grid, stream); break;
    case 3: launch_subset<3>(A, grid, stream); break;
    case 4: launch_subset<4>(A, grid, stream); break;
    case 5: launch_subset<5>(A, grid, stream); break;
    case 6: launch_subset<6>(A, grid, stream); break;
    case 7: launch_subset<7>(A, grid, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchBalCandidateSubset(const BalFreeBlocks& B, int mask, int64_t n_points, const double* x, const double* step, const double* scale,
                                    double* delta, double* cand, double* partials, int* nparts, hipStream_t stream) {
  if (mask < 1 || mask > 7) return hipErrorInvalidValue;
  const int64_t n = B.n_free_points + B.n_free_cameras;
  const int grid = vec_grid(n, kMaxVecGrid);
  *nparts = grid;
  const int cw = subset_width(mask);
  if (B.block) hipLaunchKernelGGL(bal_candidate_subset_kernel<true>, dim3(grid), dim3(kVecBlock), 0, stream, B, mask, cw, n_points, x, step, scale, delta, cand, partials);
  else hipLaunchKernelGGL(bal_candidate_subset_kernel<false>, dim3(grid), dim3(kVecBlock), 0, stream, B, mask, cw, n_points, x, step, scale, delta, cand, partials);
  return hipGetLastError();
}

}  // namespace chip
