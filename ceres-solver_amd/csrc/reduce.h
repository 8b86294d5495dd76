// reduce.h — the per-workgroup reduction every vector kernel of the BAL front end ends with, and the grid it is launched on.  The
// kernel units stay separate (bal_evaluate.h says why); these helpers are shared text, inlined into each, and the device assembly of
// every unit is what it was with its own copies (profiles/partial_sums_isa_diff.txt).
#ifndef CERES_HIP_REDUCE_H_
#define CERES_HIP_REDUCE_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"

namespace chip {
// the xor butterfly over a wavefront of 64, a fixed tree: every lane gets the result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// The epilogue of a workgroup of kVecBlock = 4 wavefronts: lane 0 of each stores its value to sh[wave]; after __syncthreads() thread 0
// combines the four in a fixed order and writes partials[blockIdx.x], which the host adds in index order (partial_sums.h)
static_assert(kVecBlock == 256, "four wavefronts per workgroup");
template <typename T>
__device__ __forceinline__ void wave_to_lds(T v, T* sh) {
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ double lds_sum4(const double* sh) { return (sh[0] + sh[1]) + (sh[2] + sh[3]); }
__device__ __forceinline__ double lds_max4(const double* sh) { return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3])); }
// workgroups for n work items, kVecBlock each (a kernel walks what lies beyond `cap` workgroups in a grid-stride loop)
inline int vec_grid(int64_t n, int cap) {
  const int64_t g = (n + kVecBlock - 1) / kVecBlock;
  return int(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace chip
#endif  // CERES_HIP_REDUCE_H_
