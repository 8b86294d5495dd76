// Inner iterations of the BAL front end (ceres_hip_bal_inner_iterate, and ceres_hip_bal_minimize with inner iterations set): one
// coordinate-descent pass is, per group of the ordering, an independent small Levenberg-Marquardt solve per parameter block with every
// other block held fixed.  Ceres runs them on a CPU thread pool, one TrustRegionMinimizer per block; here one launch runs the whole
// group, each block's loop on the device from its first evaluation to its termination.
//
//   one pass                 CoordinateDescentMinimizer::Minimize   I/coordinate_descent_minimizer.cc:130-211
//   one block                CoordinateDescentMinimizer::Solve      I/coordinate_descent_minimizer.cc:213-240: a fresh TrustRegionMinimizer
//                            with DEFAULT options (Minimizer::Options() = Solver::Options defaults, TrustRegionStrategy::Options
//                            defaults: I/trust_region_strategy.h:61-72; note max_radius 1e32), LEVENBERG_MARQUARDT, DENSE_QR
//   the loop                 I/trust_region_minimizer.cc (Init, ComputeTrustRegionStep :381-461, HandleInvalidStep :466-497,
//                            ParameterToleranceReached :726-748, FunctionToleranceReached :751-771, IsStepSuccessful :801-825,
//                            HandleSuccessfulStep :829-845), the LM step of I/levenberg_marquardt_strategy.cc:69-157
//
// The linear solve: Ceres' DENSE_QR solves [J S; D] delta ~ [-f; 0].  Here the 3x3 / 9x9 normal equations (S J^T J S + D^2) delta =
// -S J^T f are factored by Cholesky: the same step up to rounding.  A non-positive pivot is a failed solve (an invalid step), which QR
// would not report — D^2 = diag / radius > 0 keeps the matrix positive definite unless radius has grown past ~1e16 times the
// conditioning, where QR's answer is rounding noise too.  The model cost change -(m^T f + |m|^2 / 2) with m = J S step is taken
// from the same normal equations: -(step . g + step^T H step / 2).
//
// Kernel forms (the host picks per block size, bal_frontend.inc): a TEAM of T lanes solves one block, T = 1 (a lane per short point)
// or 64 (a wave per long point, and per camera).  The team strides over the block's observations and sums its 3 + 6 + 1 (point) or
// 9 + 45 + 1 (camera) accumulators with a fixed-order butterfly: every lane of the team holds the bit-identical sums, so every lane
// runs the same loop (team-uniform control flow) and nothing is summed with atomics — a pass is bit-for-bit reproducible.
// A workgroup per camera (four waves summed through LDS) was tried: at 256 VGPRs + 256 AGPRs it still spilled 560 bytes per lane, the
// wave form none; cameras take a wave whatever their size.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device.h"
#include "reduce.h"
#include "robust_loss.h"
#include "snavely.h"

namespace chip {

namespace {

constexpr int kInnerBlock = 256;   // threads per workgroup of every form

template <int NP>
struct InnerSizes {
  static constexpr int kH = NP * (NP + 1) / 2;   // upper triangle of J^T J, row-major
  static constexpr int kAcc = kH + NP + 1;       // [H | g | cost]
};

// upper-triangle index of (i, j), i <= j
template <int NP>
__device__ constexpr int tri(int i, int j) { return i * NP - i * (i - 1) / 2 + (j - i); }

// Sum acc[0 .. N) over the team (T = 64: a fixed-order butterfly); afterwards every lane of the team holds the same bits.
template <int T, int N>
__device__ __forceinline__ void team_sum(double (&acc)[N]) {
  if constexpr (T == 64) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = wave_sum(acc[k]);
  }
}

// One observation of block x: its residual block (corrected by the loss) and, JAC, the block's 2 x NP Jacobian (corrected).  Returns
// false when the residual is not finite (the evaluation fails: ResidualBlock::Evaluate's IsEvaluationValid).
template <int NP, bool JAC>
__device__ __forceinline__ bool inner_observation(const InnerArgs& A, const double (&x)[NP], int64_t k, double& cost, double (&r)[2],
                                                  double (&j)[2 * NP]) {
  const int o = A.other[k];
  const double2 ob = A.obs[k];
  double cam[9], X[3];
  if constexpr (NP == 3) {
    const double* c = A.state + A.cam_base + 9 * int64_t(o);
#pragma unroll
    for (int i = 0; i < 9; ++i) cam[i] = c[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = x[i];
  } else {
    const double* p = A.state + 3 * int64_t(o);
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = p[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) cam[i] = x[i];
  }
  double jc[18], jp[6];
  snavely<JAC>(cam, X, ob.x, ob.y, r, jc, jp);   // (the half of the Jacobian this block does not need is dead code)
  const bool finite = isfinite(r[0]) && isfinite(r[1]);
  const double s = r[0] * r[0] + r[1] * r[1];
  if constexpr (JAC) {
#pragma unroll
    for (int i = 0; i < 2 * NP; ++i) j[i] = NP == 3 ? jp[i % 6] : jc[i % 18];
  }
  if (A.loss.type == kLossNone) {
    cost = 0.5 * s;
  } else {
    double rho[3];
    robust_rho(A.loss, s, rho);
    cost = 0.5 * rho[0];
    if constexpr (JAC) {
      const RobustCorrector C = robust_corrector(s, rho);
      robust_correct_jacobian<NP>(C, r[0], r[1], j);   // (J first, with the uncorrected residual: I/residual_block.cc:161-195)
      r[0] *= C.residual_scaling;
      r[1] *= C.residual_scaling;
    }
  }
  return finite;
}

// Cost (and, JAC, H = J^T J and g = J^T f, unscaled) of block x over its entries [b, e), summed over the team.  A non-finite residual
// anywhere makes the cost NaN.
template <int NP, int T, bool JAC>
__device__ __forceinline__ void inner_evaluate(const InnerArgs& A, const double (&x)[NP], int64_t b, int64_t e, int lane,
                                               double (&acc)[InnerSizes<NP>::kAcc]) {
  constexpr int kH = InnerSizes<NP>::kH, kAcc = InnerSizes<NP>::kAcc;
  double bad = 0.0;
  if constexpr (JAC) {
#pragma unroll
    for (int i = 0; i < kAcc; ++i) acc[i] = 0.0;
  } else {
    acc[kAcc - 1] = 0.0;
  }
#pragma unroll 1
  for (int64_t k = b + lane; k < e; k += T) {
    double c, r[2], j[2 * NP];
    if (!inner_observation<NP, JAC>(A, x, k, c, r, j)) bad = 1.0;
    acc[kAcc - 1] += c;
    if constexpr (JAC) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int q = p; q < NP; ++q) acc[tri<NP>(p, q)] += j[p] * j[q] + j[NP + p] * j[NP + q];
        acc[kH + p] += j[p] * r[0] + j[NP + p] * r[1];
      }
    }
  }
  if constexpr (JAC) {
    team_sum<T, kAcc>(acc);
  } else {
    double one[1] = {acc[kAcc - 1]};
    team_sum<T, 1>(one);
    acc[kAcc - 1] = one[0];
  }
  double flag[1] = {bad};
  team_sum<T, 1>(flag);
  if (flag[0] != 0.0) acc[kAcc - 1] = __builtin_nan("");
}

// x = -(M)^-1 g by Cholesky of M (upper triangle, row-major); false if a pivot is not positive and finite.
template <int NP>
__device__ __forceinline__ bool inner_cholesky_solve(double (&M)[InnerSizes<NP>::kH], const double (&g)[NP], double (&x)[NP]) {
  // M = U^T U, U upper, stored over M
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double d = M[tri<NP>(i, i)];
#pragma unroll
    for (int k = 0; k < i; ++k) d -= M[tri<NP>(k, i)] * M[tri<NP>(k, i)];
    if (!(d > 0.0) || !isfinite(d)) return false;
    const double u = sqrt(d), inv = 1.0 / u;
    M[tri<NP>(i, i)] = u;
#pragma unroll
    for (int j = i + 1; j < NP; ++j) {
      double v = M[tri<NP>(i, j)];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= M[tri<NP>(k, i)] * M[tri<NP>(k, j)];
      M[tri<NP>(i, j)] = v * inv;
    }
  }
  double y[NP];   // U^T y = -g
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= M[tri<NP>(k, i)] * y[k];
    y[i] = v / M[tri<NP>(i, i)];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {   // U x = y
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < NP; ++k) v -= M[tri<NP>(i, k)] * x[k];
    x[i] = v / M[tri<NP>(i, i)];
  }
  return true;
}

// TrustRegionMinimizer::Options defaults (the inner minimizer's; the caller's options do not reach it)
constexpr int kInnerMaxIterations = 50, kInnerMaxInvalid = 5;
constexpr double kInnerInitialRadius = 1e4, kInnerMaxRadius = 1e32, kInnerMinRadius = 1e-32, kInnerMinDiag = 1e-6, kInnerMaxDiag = 1e32,
                 kInnerMinRelativeDecrease = 1e-3, kInnerFunctionTolerance = 1e-6, kInnerGradientTolerance = 1e-10,
                 kInnerParameterTolerance = 1e-8;

template <int NP, int T>
__global__ __launch_bounds__(kInnerBlock) void inner_blocks_kernel(InnerArgs A) {
  constexpr int kH = InnerSizes<NP>::kH, kAcc = InnerSizes<NP>::kAcc;
  constexpr int kTeams = kInnerBlock / T, kState = kH + 2 * NP;
  // LDS, per team: the loop's J^T J (scaled), LM diagonal and Jacobi scaling, which live through the whole loop but are read only in
  // the step's solve (in registers they would spill the camera form: 45 + 18 doubles beside the 55 accumulators of an evaluation).
  // Every lane of the team writes the same bits, so no lane waits for another.
  __shared__ double team_state[kTeams * kState];
  const int64_t team = (int64_t(blockIdx.x) * kInnerBlock + threadIdx.x) / T;
  const int lane = int(threadIdx.x % T);
  if (team >= A.n_blocks) return;   // (T = 64: whole waves; T = 1: single lanes)
  double* Hs = team_state + (threadIdx.x / T) * kState;
  double* diag = Hs + kH;
  double* scale = diag + NP;
  const int blk = A.blocks[team];
  double* xp = NP == 3 ? A.state + 3 * int64_t(blk) : A.state + A.cam_base + 9 * int64_t(blk);
  const int64_t b = A.ptr[blk], e = A.ptr[blk + 1];
  double x[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) x[i] = xp[i];

  // Init + EvaluateGradientAndJacobian at iteration 0: the scaling from the block's own first (corrected) Jacobian
  double acc[kAcc];
  inner_evaluate<NP, T, true>(A, x, b, e, lane, acc);
  double x_cost = acc[kAcc - 1];
  int iteration = 0;
  if (isfinite(x_cost)) {
#pragma unroll
    for (int i = 0; i < NP; ++i) scale[i] = 1.0 / (1.0 + sqrt(acc[tri<NP>(i, i)]));
    double g[NP], grad_max = 0.0;
    bool fresh = true;   // acc holds a new evaluation at x: load H = S J^T J S, g = S J^T f and the unscaled gradient's max norm
    double radius = kInnerInitialRadius, decrease_factor = 2.0;
    bool reuse_diagonal = false, one_success = false;
    int invalid_run = 0;
#pragma unroll 1
    while (true) {
      if (fresh) {
        grad_max = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const double sp = scale[p];
#pragma unroll
          for (int q = p; q < NP; ++q) Hs[tri<NP>(p, q)] = acc[tri<NP>(p, q)] * sp * scale[q];
          g[p] = acc[kH + p] * sp;
          grad_max = fmax(grad_max, fabs(acc[kH + p]));
        }
        fresh = false;
      }
      // FinalizeIterationAndCheckIfMinimizerCanContinue
      if (iteration >= kInnerMaxIterations || grad_max <= kInnerGradientTolerance || radius <= kInnerMinRadius) break;
      ++iteration;
      if (!reuse_diagonal) {
#pragma unroll
        for (int i = 0; i < NP; ++i) diag[i] = fmin(fmax(Hs[tri<NP>(i, i)], kInnerMinDiag), kInnerMaxDiag);
      }
      reuse_diagonal = true;
      double step[NP], model_cost_change = 0.0;
      bool valid;
      {
        double M[kH];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
          for (int q = p; q < NP; ++q) M[tri<NP>(p, q)] = Hs[tri<NP>(p, q)];
          M[tri<NP>(p, p)] += diag[p] / radius;   // D^2, D = sqrt(diag / radius)
        }
        valid = inner_cholesky_solve<NP>(M, g, step);
      }
      if (valid) {
        double sg = 0.0, sHs = 0.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          valid = valid && isfinite(step[p]);
          double hp = 0.0;
#pragma unroll
          for (int q = 0; q < NP; ++q) hp += Hs[p <= q ? tri<NP>(p, q) : tri<NP>(q, p)] * step[q];
          sg += step[p] * g[p];
          sHs += step[p] * hp;
        }
        model_cost_change = -(sg + 0.5 * sHs);
        valid = valid && model_cost_change > 0.0;
      }
      if (!valid) {   // HandleInvalidStep
        if (++invalid_run >= kInnerMaxInvalid) break;
        radius /= decrease_factor;
        decrease_factor *= 2.0;
        continue;
      }
      invalid_run = 0;
      double cand[NP], dn = 0.0, xn = 0.0;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        cand[i] = x[i] + step[i] * scale[i];
        const double d = x[i] - cand[i];   // (ParameterToleranceReached: |x - candidate|)
        dn += d * d;
        xn += x[i] * x[i];
      }
      inner_evaluate<NP, T, false>(A, cand, b, e, lane, acc);
      double cand_cost = acc[kAcc - 1];
      if (!isfinite(cand_cost)) cand_cost = DBL_MAX;   // a failed evaluation: a point of very high cost
      if (one_success && sqrt(dn) <= kInnerParameterTolerance * (sqrt(xn) + kInnerParameterTolerance)) break;
      if (fabs(x_cost - cand_cost) <= kInnerFunctionTolerance * x_cost) break;
      const double relative_decrease = (x_cost - cand_cost) / model_cost_change;
      if (relative_decrease > kInnerMinRelativeDecrease) {   // HandleSuccessfulStep
        inner_evaluate<NP, T, true>(A, cand, b, e, lane, acc);
        if (!isfinite(acc[kAcc - 1])) break;   // (the Jacobian's evaluation failed: Ceres stops, at the last accepted point)
#pragma unroll
        for (int i = 0; i < NP; ++i) x[i] = cand[i];
        x_cost = acc[kAcc - 1];
        fresh = true;
        one_success = true;
        const double t = 2.0 * relative_decrease - 1.0;
        radius = fmin(kInnerMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
        decrease_factor = 2.0;
        reuse_diagonal = false;
      } else {
        radius /= decrease_factor;
        decrease_factor *= 2.0;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NP; ++i) xp[i] = x[i];
    if (A.iterations) A.iterations[blk] = iteration;
  }
}

__global__ __launch_bounds__(kVecBlock) void bal_diff_norm_kernel(const double* a, const double* b, int64_t n, double* partials) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    const double d = a[i] - b[i];
    s += d * d;
  }
  s = wave_sum(s);
  wave_to_lds(s, sh);
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = lds_sum4(sh);
}

}  // namespace

hipError_t LaunchInnerBlocks(const InnerArgs& A, int form, hipStream_t stream) {
  if (A.n_blocks <= 0) return hipSuccess;
  const int64_t n = A.n_blocks;
  switch (form) {
    case kInnerPointLane:
      hipLaunchKernelGGL((inner_blocks_kernel<3, 1>), dim3(unsigned((n + kInnerBlock - 1) / kInnerBlock)), dim3(kInnerBlock), 0, stream, A);
      break;
    case kInnerPointWave:
      hipLaunchKernelGGL((inner_blocks_kernel<3, 64>), dim3(unsigned((n + 3) / 4)), dim3(kInnerBlock), 0, stream, A);
      break;
    case kInnerCameraWave:
      hipLaunchKernelGGL((inner_blocks_kernel<9, 64>), dim3(unsigned((n + 3) / 4)), dim3(kInnerBlock), 0, stream, A);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchBalDiffNorm(const double* a, const double* b, int64_t n, double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(n, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(bal_diff_norm_kernel, dim3(grid), dim3(kVecBlock), 0, stream, a, b, n, partials);
  return hipGetLastError();
}

}  // namespace chip
