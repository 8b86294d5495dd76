// kernels_cluster.hip — the CLUSTER_JACOBI preconditioner (VisibilityBasedPreconditioner with one dense block per cluster of cameras,
// I/visibility_based_preconditioner.cc): assembly of the cluster matrices from the eliminated block pairs, the batched factorisation
// M_k = L_k L_k^T and the batched application z = M^-1 r.
//
//   assemble   one thread per stored value of the cluster pairs (kernels_schur.hip's block-sparse storage, filtered to the pairs inside
//              a cluster): written into both triangles of its cluster's dense row-major matrix.  No atomics: every entry has one writer.
//   factor     one workgroup per cluster of at most kClusterLdsDim scalars, the whole matrix in LDS (pitch dim + 1: a column walk
//              touches every bank once), right-looking column Cholesky in fp64; L goes back to the lower triangle in memory.
//              Larger clusters take LaunchDenseCholesky (kernels_schur.hip), one after the other.
//   solve      one workgroup per small cluster: L in LDS (read from memory once per application), thread i owns entry i; forward
//              and backward substitution column by column, the solved entry broadcast through LDS — one barrier per column, 2 dim
//              dependent steps per application.  Gather and scatter by the cluster permutation are part of the kernel.
//              Larger clusters: LaunchClusterGather, LaunchDenseCholeskySolve, LaunchClusterScatter.
// All results are bit-reproducible (fixed summation orders, no atomics on values).
#include <hip/hip_runtime.h>

#include <mutex>

#include "device.h"

namespace chip {
namespace {

constexpr int kB = 256;

__device__ __forceinline__ int find_pair_of(const int64_t* off, int n, int64_t e) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kB) void cluster_assemble_kernel(GenStructure G, SchurPairs P, ClusterLayout C, const double* __restrict__ S,
                                                              int64_t total, double* __restrict__ mats) {
  const int64_t e = int64_t(blockIdx.x) * kB + threadIdx.x;
  if (e >= total) return;
  const int pair = find_pair_of(P.pair_off, P.npairs, e);
  const int bi = P.pair_i[pair], bj = P.pair_j[pair];
  const int nj = G.csz[G.nelim + bj];
  const int64_t ent = e - P.pair_off[pair];
  const int a = int(ent / nj), b = int(ent - int64_t(a) * nj);
  const int k = C.block_cluster[bi];   // == block_cluster[bj]: only pairs inside a cluster are stored
  const int dim = C.cl_off[k + 1] - C.cl_off[k];
  const int row = C.block_loc[bi] + a, col = C.block_loc[bj] + b;
  double* M = mats + C.mat_off[k];
  const double v = S[e];
  M[int64_t(row) * dim + col] = v;
  if (bi != bj) M[int64_t(col) * dim + row] = v;   // (a diagonal pair stores its whole block)
}

// One workgroup per small cluster.  Dynamic LDS: [dim][dim + 1] doubles.
__global__ __launch_bounds__(kB) void cluster_factor_small_kernel(ClusterLayout C, double* __restrict__ mats, int* __restrict__ fail_flag) {
  extern __shared__ double A[];
  const int k = C.small_list[blockIdx.x];
  const int dim = C.cl_off[k + 1] - C.cl_off[k];
  const int pitch = dim + 1;
  double* M = mats + C.mat_off[k];
  const int t = threadIdx.x;
  for (int e = t; e < dim * dim; e += kB) {
    const int r = e / dim, c = e - r * dim;
    A[r * pitch + c] = M[e];
  }
  __syncthreads();
  for (int j = 0; j < dim; ++j) {
    // pivot: every thread reads the same LDS word (a broadcast); the test is the same in every thread
    const double d = A[j * pitch + j];
    const bool ok = d > 0.0;   // (false for NaN)
    const double piv = ok ? sqrt(d) : 1.0;
    if (!ok && t == 0) *fail_flag = 1;   // (plain vector store of a constant: several clusters may raise it)
    __syncthreads();   // everybody has read the pivot before it is overwritten
    if (t == 0) A[j * pitch + j] = piv;
    for (int i = j + 1 + t; i < dim; i += kB) A[i * pitch + j] /= piv;
    __syncthreads();
    // trailing update of the lower triangle: A[i][c] -= L[i][j] L[c][j], j < c <= i
    const int m = dim - j - 1;
    for (int e = t; e < m * m; e += kB) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) A[i * pitch + c] -= A[i * pitch + j] * A[c * pitch + j];
    }
    __syncthreads();
  }
  for (int e = t; e < dim * dim; e += kB) {
    const int r = e / dim, c = e - r * dim;
    if (c <= r) M[e] = A[r * pitch + c];
  }
}

// One workgroup per small cluster: z = (L L^T)^-1 x on the cluster's scalars.  Dynamic LDS: [dim][dim + 1] doubles of L, then dim for
// the solved entries.
__global__ __launch_bounds__(kB) void cluster_solve_small_kernel(ClusterLayout C, const double* __restrict__ mats, const double* __restrict__ x,
                                                                 double* __restrict__ y, const int* __restrict__ status, int lds_dim) {
  if (status && *status != 0) return;
  extern __shared__ double A[];
  double* solved = A + lds_dim * (lds_dim + 1);
  const int k = C.small_list[blockIdx.x];
  const int q0 = C.cl_off[k];
  const int dim = C.cl_off[k + 1] - q0;
  const int pitch = dim + 1;
  const double* M = mats + C.mat_off[k];
  const int t = threadIdx.x;
  for (int e = t; e < dim * dim; e += kB) {
    const int r = e / dim, c = e - r * dim;
    if (c <= r) A[r * pitch + c] = M[e];
  }
  const int p = t < dim ? C.perm[q0 + t] : 0;
  double v = t < dim ? x[p] : 0.0;
  __syncthreads();
  for (int j = 0; j < dim; ++j) {   // L w = x
    if (t == j) { v /= A[j * pitch + j]; solved[j] = v; }
    __syncthreads();
    if (t > j && t < dim) v -= A[t * pitch + j] * solved[j];
  }
  __syncthreads();   // (the backward sweep re-uses `solved`)
  for (int j = dim - 1; j >= 0; --j) {   // L^T z = w
    if (t == j) { v /= A[j * pitch + j]; solved[j] = v; }
    __syncthreads();
    if (t < j) v -= A[j * pitch + t] * solved[j];
  }
  if (t < dim) y[p] = v;
}

__global__ __launch_bounds__(kB) void cluster_gather_kernel(const int32_t* __restrict__ perm, int q0, int len, const double* __restrict__ x,
                                                            double* __restrict__ xc) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < len) xc[q0 + i] = x[perm[q0 + i]];
}
__global__ __launch_bounds__(kB) void cluster_scatter_kernel(const int32_t* __restrict__ perm, int q0, int len, const double* __restrict__ xc,
                                                             double* __restrict__ y) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < len) y[perm[q0 + i]] = xc[q0 + i];
}

inline unsigned blocks_for(int64_t n) { return unsigned((n + kB - 1) / kB); }

// The dynamic-LDS ceiling is an attribute of a (kernel, device) pair: raised once per device (see LaunchDenseCholesky).
hipError_t raise_lds_ceiling() {
  static std::mutex mu;
  static unsigned long long done = 0ull;
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  std::lock_guard<std::mutex> lock(mu);
  if (done & bit) return hipSuccess;
  const void* kernels[2] = {reinterpret_cast<const void*>(cluster_factor_small_kernel), reinterpret_cast<const void*>(cluster_solve_small_kernel)};
  for (const void* k : kernels) {
    hipFuncAttributes fa;
    if (hipError_t e = hipFuncGetAttributes(&fa, k); e != hipSuccess) return e;
    const int dyn = int(kMaxLdsBytes) - int(fa.sharedSizeBytes);
    if (hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, dyn); e != hipSuccess) return e;
  }
  done |= bit;
  return hipSuccess;
}

}  // namespace

hipError_t LaunchClusterAssemble(const GenStructure& G, const SchurPairs& P, const ClusterLayout& C, const double* S, int64_t total,
                                 double* mats, hipStream_t s) {
  if (total > 0) hipLaunchKernelGGL(cluster_assemble_kernel, dim3(blocks_for(total)), dim3(kB), 0, s, G, P, C, S, total, mats);
  return hipGetLastError();
}

hipError_t LaunchClusterFactorSmall(const ClusterLayout& C, double* mats, int* fail_flag, hipStream_t s) {
  if (C.n_small <= 0) return hipSuccess;
  if (C.small_max_dim > kClusterLdsDim) return hipErrorInvalidValue;
  if (hipError_t e = raise_lds_ceiling(); e != hipSuccess) return e;
  const size_t lds = size_t(C.small_max_dim) * size_t(C.small_max_dim + 1) * sizeof(double);
  hipLaunchKernelGGL(cluster_factor_small_kernel, dim3(C.n_small), dim3(kB), lds, s, C, mats, fail_flag);
  return hipGetLastError();
}

hipError_t LaunchClusterSolveSmall(const ClusterLayout& C, const double* mats, const double* x, double* y, const int* status, hipStream_t s) {
  if (C.n_small <= 0) return hipSuccess;
  if (C.small_max_dim > kClusterLdsDim) return hipErrorInvalidValue;
  if (hipError_t e = raise_lds_ceiling(); e != hipSuccess) return e;
  const size_t lds = (size_t(C.small_max_dim) * size_t(C.small_max_dim + 1) + size_t(C.small_max_dim)) * sizeof(double);
  hipLaunchKernelGGL(cluster_solve_small_kernel, dim3(C.n_small), dim3(kB), lds, s, C, mats, x, y, status, C.small_max_dim);
  return hipGetLastError();
}

hipError_t LaunchClusterGather(const int32_t* perm, int q0, int len, const double* x, double* xc, hipStream_t s) {
  if (len > 0) hipLaunchKernelGGL(cluster_gather_kernel, dim3(blocks_for(len)), dim3(kB), 0, s, perm, q0, len, x, xc);
  return hipGetLastError();
}
hipError_t LaunchClusterScatter(const int32_t* perm, int q0, int len, const double* xc, double* y, hipStream_t s) {
  if (len > 0) hipLaunchKernelGGL(cluster_scatter_kernel, dim3(blocks_for(len)), dim3(kB), 0, s, perm, q0, len, xc, y);
  return hipGetLastError();
}

}  // namespace chip
