// The blocks pass of ceres_hip_bal_covariance on a handle with shared intrinsics (design/28_shared_covariance.md; the stages before it
// are kernels_covariance.hip's, unchanged).  A translation unit of its own for the reason bal_evaluate.h records: instantiations added to
// an existing unit move its neighbours' register allocation.
// The camera side of the program has two kinds of column blocks, the free cameras' poses (6) and the groups (3), and a row of point p has
// two camera-side cells: a pose cell at the columns a_k of S^-1 (none when the pose is constant) and a group cell at g_k.  With
// Y_k = C_p^-1 E_k^T [F_k^pose | F_k^grp] (3 x 9, or 3 x 3) and cols_k = {a_k .. a_k + 5, g_k .. g_k + 2}:
//     pose / group - pose / group   the sub-block of S^-1
//     point p - pose / group t      -sum_k Y_k S^-1[cols_k, t]
//     point p - point q             delta_pq C_p^-1 + sum_{k, l} Y_k S^-1[cols_k, cols_l] Y_l^T
// cov_blocks_kernel's scheme: one wavefront per pair, the lanes take the (row of a, row of b) pairs 64 per round, every lane adds its own
// rounds in ascending order, the lanes are added by one fixed butterfly — no floating-point atomics, two calls give the same bits; (b, a)
// is computed as (a, b) and stored transposed.  Every register array is indexed by unrolled loop counters only: a missing pose cell is a
// branch around its two products, never a run-time index.
#include <hip/hip_runtime.h>

#include "device.h"

namespace chip {

namespace {

__device__ __forceinline__ double cov_shared_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// E (2 x 3, row-major) of one row and C_p^-1 (3 x 3)
struct CovSharedPointSide {
  double e[2][3], ci[9];
};
__device__ __forceinline__ void cov_shared_load_point_side(const double* __restrict__ values, const double* __restrict__ cinv, int epos, CovSharedPointSide& S) {
#pragma unroll
  for (int t = 0; t < 6; ++t) S.e[t / 3][t % 3] = values[epos + t];
#pragma unroll
  for (int t = 0; t < 9; ++t) S.ci[t] = cinv[t];
}
// Y (3 x W) = C_p^-1 E^T F of one camera-side cell: F 2 x W row-major at values + fpos
template <int W>
__device__ __forceinline__ void cov_shared_load_y(const double* __restrict__ values, const CovSharedPointSide& S, int fpos, double (&Y)[3][W]) {
  const double* F = values + fpos;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const double f0 = F[c], f1 = F[W + c];
    double w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = S.e[0][a] * f0 + S.e[1][a] * f1;
#pragma unroll
    for (int a = 0; a < 3; ++a) Y[a][c] = S.ci[3 * a] * w[0] + S.ci[3 * a + 1] * w[1] + S.ci[3 * a + 2] * w[2];
  }
}

// R += Yk B Yl^T with B the DA x DB block of S^-1 at (row, col): column c of M = Yk B, then R += M[:, c] Yl[:, c]^T
template <int DA, int DB>
__device__ __forceinline__ void cov_shared_sandwich(const double (&Yk)[3][DA], const double* __restrict__ sinv, int n, int row, int col,
                                                    const double (&Yl)[3][DB], double (&R)[3][3]) {
  const double* B = sinv + int64_t(row) * n + col;
#pragma unroll
  for (int c = 0; c < DB; ++c) {
    double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < DA; ++d) {
      const double bv = B[int64_t(d) * n + c];
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] += Yk[a][d] * bv;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int g = 0; g < 3; ++g) R[a][g] += m[a] * Yl[g][c];
  }
}

// M += Yk B with B the DA x W block of S^-1 at (row, col)
template <int DA, int W>
__device__ __forceinline__ void cov_shared_project(const double (&Yk)[3][DA], const double* __restrict__ sinv, int n, int row, int col, double (&M)[3][W]) {
  const double* B = sinv + int64_t(row) * n + col;
#pragma unroll
  for (int d = 0; d < DA; ++d)
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const double bv = B[int64_t(d) * n + c];
#pragma unroll
      for (int a = 0; a < 3; ++a) M[a][c] += Yk[a][d] * bv;
    }
}

// point p - the W columns of S^-1 from tcol on (a pose: 6, a group: 3), or that block against the point stored transposed
template <int W>
__device__ __forceinline__ void cov_shared_point_side(const CovSharedBlocksArgs& P, int lane, int p, int tcol, bool swap, double* __restrict__ out) {
  const int n = P.n;
  const int p0 = P.pt_ptr[p], np = P.pt_ptr[p + 1] - p0;
  double M[3][W];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < W; ++c) M[a][c] = 0.0;
  for (int t = lane; t < np; t += 64) {
    const int k = p0 + t;
    CovSharedPointSide S;
    cov_shared_load_point_side(P.values, P.cinv + 9 * int64_t(p), P.ent_epos[k], S);
    const int pcol = P.ent_pcol[k];
    if (pcol >= 0) {
      double Yp[3][6];
      cov_shared_load_y<6>(P.values, S, P.ent_ppos[k], Yp);
      cov_shared_project<6, W>(Yp, P.sinv, n, pcol, tcol, M);
    }
    double Yg[3][3];
    cov_shared_load_y<3>(P.values, S, P.ent_gpos[k], Yg);
    cov_shared_project<3, W>(Yg, P.sinv, n, P.ent_gcol[k], tcol, M);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < W; ++c) M[a][c] = cov_shared_wave_sum(M[a][c]);
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < W; ++c) {
        if (swap) out[3 * c + a] = -M[a][c]; else out[W * a + c] = -M[a][c];
      }
  }
}

__device__ __forceinline__ int cov_shared_dim(int kind) { return (kind == kCovSharedPose || kind == kCovSharedConstPose) ? 6 : 3; }

__global__ __launch_bounds__(256) void cov_shared_blocks_kernel(CovSharedBlocksArgs P) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= P.n_pairs) return;
  const int lane = threadIdx.x & 63;
  const int ca = P.code_a[pair], cb = P.code_b[pair];
  double* out = P.out + P.out_off[pair];
  const int ka = ca & 3, kb = cb & 3;
  const int da = cov_shared_dim(ka), db = cov_shared_dim(kb);
  if (ka == kCovSharedConstPose || kb == kCovSharedConstPose) {
    for (int e = lane; e < da * db; e += 64) out[e] = 0.0;
    return;
  }
  const int n = P.n;
  if (ka != kCovSharedPoint && kb != kCovSharedPoint) {   // S^-1 is exactly symmetric: (b, a) reads the transposed entries
    const double* B = P.sinv + int64_t(ca >> 2) * n + (cb >> 2);
    for (int e = lane; e < da * db; e += 64) out[e] = B[int64_t(e / db) * n + e % db];
    return;
  }
  if (ka == kCovSharedPoint && kb == kCovSharedPoint) {
    const bool swap = (ca >> 2) > (cb >> 2);
    const int p = swap ? cb >> 2 : ca >> 2, q = swap ? ca >> 2 : cb >> 2;
    const int p0 = P.pt_ptr[p], np = P.pt_ptr[p + 1] - p0, q0 = P.pt_ptr[q], nq = P.pt_ptr[q + 1] - q0;
    double R[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const int64_t total = int64_t(np) * nq;
    for (int64_t t = lane; t < total; t += 64) {
      const int k = p0 + int(t / nq), l = q0 + int(t % nq);
      CovSharedPointSide Sk, Sl;
      cov_shared_load_point_side(P.values, P.cinv + 9 * int64_t(p), P.ent_epos[k], Sk);
      cov_shared_load_point_side(P.values, P.cinv + 9 * int64_t(q), P.ent_epos[l], Sl);
      const int ak = P.ent_pcol[k], al = P.ent_pcol[l], gk = P.ent_gcol[k], gl = P.ent_gcol[l];
      double Ykg[3][3], Ylg[3][3];
      cov_shared_load_y<3>(P.values, Sk, P.ent_gpos[k], Ykg);
      cov_shared_load_y<3>(P.values, Sl, P.ent_gpos[l], Ylg);
      double Ylp[3][6];
      if (al >= 0) cov_shared_load_y<6>(P.values, Sl, P.ent_ppos[l], Ylp);
      if (ak >= 0) {
        double Ykp[3][6];
        cov_shared_load_y<6>(P.values, Sk, P.ent_ppos[k], Ykp);
        if (al >= 0) cov_shared_sandwich<6, 6>(Ykp, P.sinv, n, ak, al, Ylp, R);
        cov_shared_sandwich<6, 3>(Ykp, P.sinv, n, ak, gl, Ylg, R);
      }
      if (al >= 0) cov_shared_sandwich<3, 6>(Ykg, P.sinv, n, gk, al, Ylp, R);
      cov_shared_sandwich<3, 3>(Ykg, P.sinv, n, gk, gl, Ylg, R);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int g = 0; g < 3; ++g) R[a][g] = cov_shared_wave_sum(R[a][g]);
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          // (a point's own block: the lower triangle, mirrored — exactly symmetric like S^-1)
          const int a2 = p == q ? max(a, g) : a, g2 = p == q ? min(a, g) : g;
          const double v = R[a2][g2] + (p == q ? P.cinv[9 * int64_t(p) + 3 * a2 + g2] : 0.0);
          if (swap) out[3 * g + a] = v; else out[3 * a + g] = v;
        }
    }
    return;
  }
  // point - pose / group, or pose / group - point stored transposed (the kind is the wavefront's: a uniform branch)
  const bool swap = kb == kCovSharedPoint;
  const int p = swap ? cb >> 2 : ca >> 2, tcol = swap ? ca >> 2 : cb >> 2;
  if ((swap ? ka : kb) == kCovSharedPose) cov_shared_point_side<6>(P, lane, p, tcol, swap, out);
  else cov_shared_point_side<3>(P, lane, p, tcol, swap, out);
}

}  // namespace

hipError_t LaunchCovSharedBlocks(const CovSharedBlocksArgs& P, hipStream_t s) {
  if (P.n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(cov_shared_blocks_kernel, dim3(unsigned((P.n_pairs + 3) / 4)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace chip
