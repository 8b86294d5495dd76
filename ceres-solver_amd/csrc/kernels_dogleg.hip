// kernels_dogleg.hip — the device side of DoglegStrategy (I/dogleg_strategy.cc) for the BAL front end (dogleg.inc).
//
// Every dogleg step lies in span{a, b} with a = g / d and b = gn / d (d: the strategy's diagonal, g the scaled gradient, gn the
// scaled Gauss-Newton step).  One pass over J that yields the five scalars
//   |J a|^2, (J a).(J b), |J b|^2, (J a).f, (J b).f
// therefore gives the Cauchy point's alpha, the subspace model's 2x2 matrix and the model cost change of ANY step alpha a + beta b,
// for every radius a rejected step may ask for later.  Both kernels write their partial sums per workgroup, summed on the host in a
// fixed order: no atomics, results are bit-for-bit repeatable.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device.h"

namespace chip {

namespace {

constexpr int kB = 256;

// lane sums -> one value per workgroup, fixed order (butterfly in the wave, waves in index order)
template <int K>
__device__ __forceinline__ void block_store(double (&v)[K], double* __restrict__ out) {
  __shared__ double sh[kB / 64][K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = 0;
    for (int w = 0; w < kB / 64; ++w) t += sh[w][threadIdx.x];
    out[int64_t(K) * blockIdx.x + threadIdx.x] = t;
  }
}

// A thread per scalar row (grid-strided): (J a)_r and (J b)_r from ONE walk over the row's cells, then the five products.
// f == nullptr: no residuals loaded, the two f products are 0.
__global__ __launch_bounds__(kB) void jacobian_gram_kernel(GenStructure G, const double* __restrict__ v, const double* __restrict__ a,
                                                           const double* __restrict__ b, const double* __restrict__ f,
                                                           double* __restrict__ partials) {
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int row = blockIdx.x * kB + threadIdx.x; row < G.num_rows; row += gridDim.x * kB) {
    const int i = G.row_block_of[row];
    const int r = row - G.rpos[i];
    double ma = 0.0, mb = 0.0;
    for (int k = G.rptr[i]; k < G.rptr[i + 1]; ++k) {
      const int j = G.ccol[k];
      const int cs = G.csz[j];
      const double* c = v + G.cval[k] + int64_t(r) * cs;
      const int p = G.cpos[j];
      for (int q = 0; q < cs; ++q) {
        const double cq = c[q];
        ma += cq * a[p + q];
        mb += cq * b[p + q];
      }
    }
    const double fr = f ? f[row] : 0.0;
    acc[0] += ma * ma;
    acc[1] += ma * mb;
    acc[2] += mb * mb;
    acc[3] += ma * fr;
    acc[4] += mb * fr;
  }
  block_store<5>(acc, partials);
}

// The strategy's vectors from the clamped squared column norms `dsq` (ComputeStep :121-129), the gradient J^T f and the
// Levenberg-Marquardt solution `b` (= gn / diagonal, :607-613):
//   diagonal = sqrt(dsq), gradient = J^T f / diagonal (:176-183), a = gradient / diagonal (:191-195), gn = diagonal * b
// a is written; the partial sums of |gradient|^2, gradient.gn and |gn|^2 go to partials (3 per workgroup).
__global__ __launch_bounds__(kB) void dogleg_prep_kernel(const double* __restrict__ dsq, const double* __restrict__ jtf,
                                                         const double* __restrict__ b, double* __restrict__ a, int64_t n,
                                                         double* __restrict__ partials) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = int64_t(blockIdx.x) * kB + threadIdx.x; i < n; i += int64_t(gridDim.x) * kB) {
    const double d = sqrt(dsq[i]);
    const double g = jtf[i] / d;
    const double gn = d * b[i];
    a[i] = g / d;
    acc[0] += g * g;
    acc[1] += g * gn;
    acc[2] += gn * gn;
  }
  block_store<3>(acc, partials);
}

int grid_for(int64_t n) { return int(std::max<int64_t>(1, std::min<int64_t>(kDoglegGrid, (n + kB - 1) / kB))); }

}  // namespace

hipError_t LaunchJacobianGram(const GenStructure& G, const double* values, const double* a, const double* b, const double* f,
                              double* partials, int* nparts, hipStream_t s) {
  *nparts = grid_for(G.num_rows);
  hipLaunchKernelGGL(jacobian_gram_kernel, dim3(*nparts), dim3(kB), 0, s, G, values, a, b, f, partials);
  return hipGetLastError();
}

hipError_t LaunchDoglegPrep(const double* dsq, const double* jtf, const double* b, double* a, int64_t n, double* partials, int* nparts,
                            hipStream_t s) {
  *nparts = grid_for(n);
  hipLaunchKernelGGL(dogleg_prep_kernel, dim3(*nparts), dim3(kB), 0, s, dsq, jtf, b, a, n, partials);
  return hipGetLastError();
}

}  // namespace chip
