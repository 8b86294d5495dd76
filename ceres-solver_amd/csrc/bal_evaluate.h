// bal_evaluate.h — the caller-layout evaluator kernel (one thread per observation: residual, Snavely Jacobian, loss, Jacobi scaling), a
// template on the camera model.  kernels_evaluator.hip instantiates the angle-axis camera, kernels_quaternion.hip the two quaternion
// cameras: in one translation unit the quaternion instantiations changed the register allocation of the tile-order evaluator's robust
// instantiations (the inliner's choices for the loss functions they share).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device.h"
#include "reduce.h"
#include "robust_loss.h"
#include "snavely.h"

namespace chip {

namespace {

// ROBUST: A.loss applies (robust_loss.h) — cost rho / 2, the Jacobian corrected with the uncorrected residual, then the residual; the
// Jacobi column scaling comes after the correction.  !ROBUST: the squared loss, as this kernel was before losses existed.
// CM: the camera model (kCam*, device.h) — state doubles per camera SW, Jacobian columns per camera CW (the scale vector and the F cells
// are in the tangent space: 9 for the angle-axis and the quaternion-manifold camera, 10 for the Euclidean quaternion).
// CONST: a reduced program (BalEvalConstArgs: row_fpos / row_scam / row_spt): a cell of a constant block is neither scaled nor stored,
// the Corrector still uses the whole residual.  A template flag: the !CONST instantiations are the kernel as it was, arguments included.
template <bool JAC, bool ROBUST, int CM = kCamAngleAxis, bool CONST = false>
__global__ __launch_bounds__(kVecBlock) void bal_evaluate_kernel(typename std::conditional<CONST, BalEvalConstArgs, BalEvalArgs>::type A) {
  constexpr int SW = CM == kCamAngleAxis ? 9 : 10;
  constexpr int CW = CM == kCamQuaternion ? 10 : 9;
  __shared__ double sh[4];
  double cost = 0.0;
  for (int64_t r = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; r < A.n_rows; r += int64_t(gridDim.x) * kVecBlock) {
    const int c = A.row_cam[r], p = A.row_pt[r];
    const double2 o = A.row_obs[r];
    double cam[SW], X[3], res[2], jc[2 * CW], jp[6];
    const double* cs = A.state + A.cam_base + SW * int64_t(c);
    const double* ps = A.state + 3 * int64_t(p);
#pragma unroll
    for (int i = 0; i < SW; ++i) cam[i] = cs[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = ps[i];
    if constexpr (CM == kCamAngleAxis) snavely<JAC>(cam, X, o.x, o.y, res, jc, jp);
    else snavely_quat<JAC, CM == kCamQuaternionManifold>(cam, X, o.x, o.y, res, jc, jp);
    if constexpr (ROBUST) {
      const double sq = res[0] * res[0] + res[1] * res[1];
      double rho[3];
      robust_rho(A.loss, sq, rho);
      cost += 0.5 * rho[0];
      if (JAC || A.residuals) {   // (cost only: no Corrector, I/residual_block.cc:175-178)
        const RobustCorrector C = robust_corrector(sq, rho);
        if constexpr (JAC) {
          robust_correct_jacobian<CW>(C, res[0], res[1], jc);
          robust_correct_jacobian<3>(C, res[0], res[1], jp);
        }
        res[0] *= C.residual_scaling; res[1] *= C.residual_scaling;
      }
    } else {
      cost += 0.5 * (res[0] * res[0] + res[1] * res[1]);
    }
    if (A.residuals) reinterpret_cast<double2*>(A.residuals)[r] = make_double2(res[0], res[1]);
    if constexpr (JAC && CONST) {
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
          for (int j = 0; j < CW; ++j) { const double v = sc[j]; jc[j] *= v; jc[CW + j] *= v; }
        }
        double2* fo = reinterpret_cast<double2*>(A.values + fpos);
#pragma unroll
        for (int j = 0; j < CW; ++j) fo[j] = make_double2(jc[2 * j], jc[2 * j + 1]);
      }
    } else if constexpr (JAC) {
      if (A.scale) {
        const double* sc = A.scale + A.cam_base + CW * int64_t(c);
        const double* sp = A.scale + 3 * int64_t(p);
#pragma unroll
        for (int j = 0; j < CW; ++j) { const double v = sc[j]; jc[j] *= v; jc[CW + j] *= v; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double v = sp[j]; jp[j] *= v; jp[3 + j] *= v; }
      }
      double2* e = reinterpret_cast<double2*>(A.values + 6 * r);                // 48 B per row, 16-byte aligned
      double2* fo = reinterpret_cast<double2*>(A.values + 6 * A.n_rows + 2 * CW * r);  // 144 (160) B per row
#pragma unroll
      for (int j = 0; j < 3; ++j) e[j] = make_double2(jp[2 * j], jp[2 * j + 1]);
#pragma unroll
      for (int j = 0; j < CW; ++j) fo[j] = make_double2(jc[2 * j], jc[2 * j + 1]);
    }
  }
  cost = wave_sum(cost);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cost;   // (inline: wave_to_lds here renumbers the blocks of kernels_quaternion.hip)
  __syncthreads();
  if (threadIdx.x == 0) A.partials[blockIdx.x] = lds_sum4(sh);
}

}  // namespace

}  // namespace chip
