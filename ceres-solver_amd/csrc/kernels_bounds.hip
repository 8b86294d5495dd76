// Bound constraints of the BAL front end (ceres_hip_bal_set_bounds; bounds.inc): the vector kernels of the trust-region loop on a
// CONSTRAINED handle.  ParameterBlock::Plus clamps every coordinate of x_plus_delta to [lower, upper] (I/parameter_block.h:227-255);
// TrustRegionMinimizer projects the initial point (Plus(x, 0), I/trust_region_minimizer.cc:210-220), measures the gradient as
// |x - Plus(x, -g)| (:281-302), searches along clamp(x + a delta) (DoLineSearch, :596-641) and takes |x - candidate| as the step norm
// (:726-748).  Three kernels — the projection in place with an exact count of what it moved, the bounded trial point with its four
// partial sums in one pass, the projected gradient max norm — each in two forms: PLAIN (every block free: ambient index = tangent
// index, one work item per double) and FREE (a BalFreeBlocks list: one work item per free block of 3, 9 or 10 doubles; constant blocks
// are neither read nor written).  Only handles whose Plus is x + delta take bounds (angle-axis and Euclidean quaternion cameras), so
// inside a block the ambient and the tangent offset coincide.
// A unit of its own for the reason bal_evaluate.h records: no instantiation is added to an existing unit.  Sums in a fixed order, no
// floating-point atomics: two launches at one state give the same bits.  Every product and sum is rounded on its own (no contraction
// into fma), so the trial point is the restatement's clamp(x + a * delta) to the bit.
#include <hip/hip_runtime.h>

#include "device.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace chip {

namespace {

// std::max(v, lower) then std::min(., upper), as ParameterBlock::Plus writes them (a NaN passes through; no bound: -inf / +inf)
__device__ __forceinline__ double clamp_b(double v, double lo, double hi) {
  v = v < lo ? lo : v;
  return hi < v ? hi : v;
}

// Walks the coordinates a thread owns and hands f(ambient index, tangent index) each of them.  W == 0: the plain form, n doubles;
// W == 9 | 10: the free-block form, n_free_points blocks of 3 then n_free_cameras blocks of W.
template <int W, class F>
__device__ __forceinline__ void for_each_coordinate(const BalFreeBlocks& B, F f) {
  const int64_t first = int64_t(blockIdx.x) * kVecBlock + threadIdx.x, stride = int64_t(gridDim.x) * kVecBlock;
  if constexpr (W == 0) {
    for (int64_t i = first; i < B.n_free_points; i += stride) f(i, i);
  } else {
    const int64_t nfp = B.n_free_points, n = nfp + B.n_free_cameras;
    for (int64_t i = first; i < n; i += stride) {
      const int64_t a = B.block[i];
      if (i < nfp) {
#pragma unroll
        for (int j = 0; j < 3; ++j) f(a + j, 3 * i + j);
      } else {
        const int64_t t = 3 * nfp + W * (i - nfp);
#pragma unroll
        for (int j = 0; j < W; ++j) f(a + j, t + j);
      }
    }
  }
}

template <int W>
__global__ __launch_bounds__(kVecBlock) void bounds_project_kernel(BalFreeBlocks B, const double* lower, const double* upper, double* x,
                                                                   unsigned long long* counts) {
  __shared__ unsigned sh[4];
  unsigned moved = 0;   // (a thread owns at most 2^31 / (kMaxVecGrid kVecBlock) blocks of at most 10 doubles)
  for_each_coordinate<W>(B, [&](int64_t a, int64_t) {
    const double v = x[a], c = clamp_b(v, lower[a], upper[a]);
    if (c != v) { x[a] = c; ++moved; }
  });
  moved = wave_sum(moved);
  wave_to_lds(moved, sh);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned long long)(sh[0]) + sh[1] + sh[2] + sh[3];
}

template <int W>
__global__ __launch_bounds__(kVecBlock) void bounds_trial_kernel(BalFreeBlocks B, const double* lower, const double* upper, const double* x,
                                                                 const double* step, const double* scale, const double* grad, double t, int fold,
                                                                 double* delta, double* out, double* partials) {
  __shared__ double sh[16];
  double xn = 0, sn = 0, dm = 0, gd = 0;
  for_each_coordinate<W>(B, [&](int64_t a, int64_t k) {
    const double sc = scale ? scale[k] : 1.0;
    double d = scale ? step[k] * sc : step[k];
    double move = t * d;
    if (fold) d = move;
    const double xi = x[a];
    const double o = clamp_b(xi + move, lower[a], upper[a]);
    delta[k] = d;
    out[a] = o;
    const double diff = o - xi;
    xn += xi * xi;
    sn += diff * diff;
    dm = fmax(dm, fabs(d));
    if (grad) gd += (scale ? grad[k] / sc : grad[k]) * d;
  });
  xn = wave_sum(xn); sn = wave_sum(sn); dm = wave_max(dm); gd = wave_sum(gd);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh[w] = xn; sh[4 + w] = sn; sh[8 + w] = dm; sh[12 + w] = gd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int g = gridDim.x;
    partials[blockIdx.x] = lds_sum4(sh);
    partials[g + blockIdx.x] = lds_sum4(sh + 4);
    partials[2 * g + blockIdx.x] = lds_max4(sh + 8);
    partials[3 * g + blockIdx.x] = lds_sum4(sh + 12);
  }
}

template <int W>
__global__ __launch_bounds__(kVecBlock) void bounds_gradient_max_kernel(BalFreeBlocks B, const double* lower, const double* upper, const double* x,
                                                                        const double* g, const double* scale, double* partials) {
  __shared__ double sh[4];
  double m = 0;
  for_each_coordinate<W>(B, [&](int64_t a, int64_t k) {
    const double gi = scale ? g[k] / scale[k] : g[k];
    const double xi = x[a];
    m = fmax(m, fabs(xi - clamp_b(xi - gi, lower[a], upper[a])));
  });
  m = wave_max(m);
  wave_to_lds(m, sh);
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = lds_max4(sh);
}

// work items: doubles in the plain form, free blocks in the other
int bounds_grid(const BalBounds& K) {
  return vec_grid(K.B.block ? K.B.n_free_points + K.B.n_free_cameras : K.B.n_free_points, kMaxVecGrid);
}
// 0: plain, 9 | 10: free blocks; -1: a width no kernel was built for
int form_of(const BalBounds& K) {
  if (!K.B.block) return 0;
  return K.camera_width == 9 || K.camera_width == 10 ? K.camera_width : -1;
}

}  // namespace

#define BOUNDS_DISPATCH(kernel, ...)                                                                              \
  switch (form_of(K)) {                                                                                           \
    case 0: hipLaunchKernelGGL((kernel<0>), dim3(grid), dim3(kVecBlock), 0, stream, __VA_ARGS__); break;          \
    case 9: hipLaunchKernelGGL((kernel<9>), dim3(grid), dim3(kVecBlock), 0, stream, __VA_ARGS__); break;          \
    case 10: hipLaunchKernelGGL((kernel<10>), dim3(grid), dim3(kVecBlock), 0, stream, __VA_ARGS__); break;        \
    default: return hipErrorInvalidValue;                                                                         \
  }

hipError_t LaunchBoundsProject(const BalBounds& K, double* x, unsigned long long* counts, int* nparts, hipStream_t stream) {
  const int grid = bounds_grid(K);
  *nparts = grid;
  BOUNDS_DISPATCH(bounds_project_kernel, K.B, K.lower, K.upper, x, counts)
  return hipGetLastError();
}

hipError_t LaunchBoundsTrialPoint(const BalBounds& K, const double* x, const double* step, const double* scale, const double* grad, double t,
                                  bool fold, double* delta, double* out, double* partials, int* nparts, hipStream_t stream) {
  const int grid = bounds_grid(K);
  *nparts = grid;
  BOUNDS_DISPATCH(bounds_trial_kernel, K.B, K.lower, K.upper, x, step, scale, grad, t, fold ? 1 : 0, delta, out, partials)
  return hipGetLastError();
}

hipError_t LaunchBoundsGradientMax(const BalBounds& K, const double* x, const double* g, const double* scale, double* partials, int* nparts,
                                   hipStream_t stream) {
  const int grid = bounds_grid(K);
  *nparts = grid;
  BOUNDS_DISPATCH(bounds_gradient_max_kernel, K.B, K.lower, K.upper, x, g, scale, partials)
  return hipGetLastError();
}
#undef BOUNDS_DISPATCH

}  // namespace chip
