// Covariance of a bundle-adjustment problem (ceres::Covariance, include/ceres/covariance.h, I/covariance_impl.cc) in the Schur form
// — design/17_covariance.md.  With C_p = E_p^T E_p, W_p = E_p^T F, Y_p = C_p^-1 W_p and S = F^T F - sum_p W_p^T C_p^-1 W_p:
//     camera - camera   the block of S^-1
//     point p - camera  -Y_p S^-1[:, c]
//     point p - point q delta_pq C_p^-1 + Y_p S^-1 Y_q^T
// What lives here:
//   cov_point_factor_kernel   every 3 x 3 C_p: unit-diagonal scaling, Cholesky, the smallest pivot, C_p^-1 (zeros where it fails: no NaN)
//   cov_diag_scale_kernel /   Lambda = diag(S)^-1/2 and S~ = Lambda S Lambda (factored by LaunchDenseCholesky, kernels_schur.hip)
//   cov_scale_kernel
//   cov_min_kernel            the smallest entry of a vector (or squared diagonal entry of the factor) and where it is: one workgroup,
//                             a fixed order
//   the inverse from the factor, L in the lower triangle of A (n x n, row-major), X = L^-1 in place, then S~^-1 = X^T X:
//     cov_diag_inverse_kernel   the 32 x 32 diagonal blocks of L inverted in place (zeros above the diagonal inside the block)
//     cov_trtri_gemm_kernel     level b = 32, 64, ...: the matrix is cut into pairs of b-wide diagonal blocks [X11 0; X21 X22] with
//                               X21 = -X22 L21 X11 — every pair of a level at once, two launches: T = L21 X11 into the second buffer,
//                               then X21 = -X22 T over L21.  log2(n / 32) levels instead of n / 32 dependent block columns.
//     cov_xtx_kernel            Cov = Lambda X^T X Lambda into the second buffer: the lower triangle is computed, both triangles are
//                               written from the same value (exactly symmetric)
//     All three products are v_mfma_f64_16x16x4_f64 on 32 x 32 outputs per wavefront; they skip the structural zeros of the
//     triangular operands by their k ranges (n^3 / 3 flops for X, n^3 / 3 for X^T X).
//   cov_blocks_kernel         one wavefront per requested pair, lanes over the (observation of a, observation of b) pairs
// No floating-point atomics anywhere: every sum has a fixed order, two calls at one state give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device.h"

namespace chip {

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int kCovBase = 32;   // diagonal blocks inverted directly; also the wavefront's output tile

// ---- points -------------------------------------------------------------------------------------------------------------------------
// blocks: 9 doubles per free point, C_p (symmetric) in, C_p^-1 out.  pivot[p] = the smallest pivot of the Cholesky factorisation of
// Lambda C_p Lambda (Lambda = diag(C_p)^-1/2); 0 stands for "a diagonal entry or a pivot is not positive (or not a number)".
__global__ __launch_bounds__(kVecBlock) void cov_point_factor_kernel(int n_points, double* __restrict__ blocks, double* __restrict__ pivot) {
  const int p = blockIdx.x * kVecBlock + threadIdx.x;
  if (p >= n_points) return;
  double* C = blocks + 9 * int64_t(p);
  const double c00 = C[0], c01 = C[1], c02 = C[2], c11 = C[4], c12 = C[5], c22 = C[8];
  double piv = 0.0;
  double inv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // 00 01 02 11 12 22
  if (c00 > 0.0 && c11 > 0.0 && c22 > 0.0 && c00 < INFINITY && c11 < INFINITY && c22 < INFINITY) {
    const double l0 = 1.0 / sqrt(c00), l1 = 1.0 / sqrt(c11), l2 = 1.0 / sqrt(c22);
    const double a00 = c00 * l0 * l0, a01 = c01 * l0 * l1, a02 = c02 * l0 * l2, a11 = c11 * l1 * l1, a12 = c12 * l1 * l2, a22 = c22 * l2 * l2;
    // Cholesky of the scaled block; the pivots are d0, d1, d2
    const double d0 = a00;
    const double g10 = a01 / sqrt(d0), g20 = a02 / sqrt(d0);
    const double d1 = a11 - g10 * g10;
    if (d1 > 0.0) {
      const double g11 = sqrt(d1);
      const double g21 = (a12 - g20 * g10) / g11;
      const double d2 = a22 - g20 * g20 - g21 * g21;
      if (d2 > 0.0) {
        const double g00 = sqrt(d0), g22 = sqrt(d2);
        piv = fmin(d0, fmin(d1, d2));
        // M = G^-1 (lower), inverse = M^T M
        const double m00 = 1.0 / g00, m11 = 1.0 / g11, m22 = 1.0 / g22;
        const double m10 = -g10 * m00 * m11;
        const double m21 = -g21 * m11 * m22;
        const double m20 = -(g20 * m00 + g21 * m10) * m22;
        inv[0] = (m00 * m00 + m10 * m10 + m20 * m20) * l0 * l0;
        inv[1] = (m10 * m11 + m20 * m21) * l0 * l1;
        inv[2] = (m20 * m22) * l0 * l2;
        inv[3] = (m11 * m11 + m21 * m21) * l1 * l1;
        inv[4] = (m21 * m22) * l1 * l2;
        inv[5] = (m22 * m22) * l2 * l2;
        if (!(piv > 0.0)) piv = 0.0;
      }
    }
  }
  pivot[p] = piv;
  C[0] = inv[0]; C[1] = inv[1]; C[2] = inv[2];
  C[3] = inv[1]; C[4] = inv[3]; C[5] = inv[4];
  C[6] = inv[2]; C[7] = inv[4]; C[8] = inv[5];
}

// out[0] = min_i f(v[i stride]), out[1] = the first i that attains it; f = identity or the square.  Entries that are not numbers count as 0.
__global__ __launch_bounds__(kVecBlock) void cov_min_kernel(const double* __restrict__ v, int64_t count, int64_t stride, int square, double* __restrict__ out) {
  __shared__ double sm[kVecBlock];
  __shared__ int64_t si[kVecBlock];
  double m = INFINITY;
  int64_t at = -1;
  for (int64_t i = threadIdx.x; i < count; i += kVecBlock) {
    double x = v[i * stride];
    if (square) x = x * x;
    if (!(x == x)) x = 0.0;
    if (x < m) { m = x; at = i; }
  }
  sm[threadIdx.x] = m; si[threadIdx.x] = at;
  __syncthreads();
  for (int w = kVecBlock / 2; w >= 1; w >>= 1) {
    if (int(threadIdx.x) < w) {
      const double o = sm[threadIdx.x + w];
      const int64_t oi = si[threadIdx.x + w];
      if (o < sm[threadIdx.x] || (o == sm[threadIdx.x] && oi >= 0 && (si[threadIdx.x] < 0 || oi < si[threadIdx.x]))) { sm[threadIdx.x] = o; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = sm[0]; out[1] = double(si[0]); }
}

// ---- the scaling of S -----------------------------------------------------------------------------------------------------------------
// lam[i] = S_ii^-1/2; a diagonal entry that is not positive and finite raises flag (every writer stores the same 1) and gets lam = 0
__global__ __launch_bounds__(kVecBlock) void cov_diag_scale_kernel(const double* __restrict__ S, int n, double* __restrict__ lam, int* flag) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= n) return;
  const double d = S[int64_t(i) * n + i];
  if (d > 0.0 && d < INFINITY) lam[i] = 1.0 / sqrt(d);
  else { lam[i] = 0.0; *flag = 1; }
}
__global__ __launch_bounds__(kVecBlock) void cov_scale_kernel(double* __restrict__ S, int n, const double* __restrict__ lam) {
  const int64_t e = int64_t(blockIdx.x) * kVecBlock + threadIdx.x;
  if (e >= int64_t(n) * n) return;
  const int r = int(e / n), c = int(e - int64_t(r) * n);
  S[e] = S[e] * lam[r] * lam[c];
}

// ---- the inverse from the factor ------------------------------------------------------------------------------------------------------
// One workgroup of 32 lanes per diagonal block: lane c solves L x = e_c by forward substitution from LDS; the block is replaced by its
// inverse, zeros above the diagonal (the factorisation parks the inverses of its 16 x 16 sub-blocks there: kernels_schur.hip).
__global__ __launch_bounds__(kCovBase) void cov_diag_inverse_kernel(double* A, int n) {
  __shared__ double Ls[kCovBase][kCovBase + 1];
  __shared__ double Xs[kCovBase][kCovBase + 1];
  const int k0 = blockIdx.x * kCovBase, c = threadIdx.x;
  const int nb = min(kCovBase, n - k0);
  for (int r = 0; r < kCovBase; ++r) Ls[r][c] = (r < nb && c <= r) ? A[int64_t(k0 + r) * n + (k0 + c)] : (r == c ? 1.0 : 0.0);
  __syncthreads();
  for (int r = 0; r < kCovBase; ++r) {
    double s = r == c ? 1.0 : 0.0;
    for (int k = c; k < r; ++k) s -= Ls[r][k] * Xs[k][c];   // (lane c reads its own column only)
    Xs[r][c] = r >= c ? s / Ls[r][r] : 0.0;
  }
  __syncthreads();
  for (int r = 0; r < nb; ++r) if (c < nb) A[int64_t(k0 + r) * n + (k0 + c)] = Xs[r][c];
}

// acc[a][b] += sum_k A(i0 + 16 a + .., k) B(k, j0 + 16 b + ..) over k in [k0, k1) (k0 a multiple of 4), terms with k >= klim dropped.
// Operand layout of v_mfma_f64_16x16x4_f64, lane l: li = l & 15, lq = l >> 4 — the A operand is A[li][k + lq], the B operand B[k + lq][li],
// accumulator register r is C[lq + 4 r][li].  B is row-major with pitch ldb; A row-major (A(r, k) = Ab[r lda + k]) or, with kATrans,
// the transpose of a row-major matrix (A(r, k) = Ab[k lda + r]).  Rows and columns past `last` are clamped: their results are never stored.
template <bool kATrans>
__device__ __forceinline__ void cov_mma_32x32(const double* __restrict__ Ab, int64_t lda, int i0, const double* __restrict__ Bb, int64_t ldb, int j0, int last,
                                              int k0, int k1, int klim, int li, int lq, v4f64 (&acc)[2][2]) {
  const int ra0 = min(i0 + li, last), ra1 = min(i0 + 16 + li, last);
  const int cb0 = min(j0 + li, last), cb1 = min(j0 + 16 + li, last);
  const int kend = min(k1, klim);
  const int kfull = kend > k0 ? k0 + (kend - k0) / 4 * 4 : k0;
#pragma unroll 4
  for (int k = k0; k < kfull; k += 4) {
    const int kk = k + lq;
    const double a0 = kATrans ? Ab[int64_t(kk) * lda + ra0] : Ab[int64_t(ra0) * lda + kk];
    const double a1 = kATrans ? Ab[int64_t(kk) * lda + ra1] : Ab[int64_t(ra1) * lda + kk];
    const double b0 = Bb[int64_t(kk) * ldb + cb0], b1 = Bb[int64_t(kk) * ldb + cb1];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
  if (kfull < kend) {   // the last, partial step: k past the limit reads a clamped address and contributes zero
    const int kk = kfull + lq;
    const bool ok = kk < klim;
    const int kc = ok ? kk : klim - 1;
    double a0 = kATrans ? Ab[int64_t(kc) * lda + ra0] : Ab[int64_t(ra0) * lda + kc];
    double a1 = kATrans ? Ab[int64_t(kc) * lda + ra1] : Ab[int64_t(ra1) * lda + kc];
    double b0 = Bb[int64_t(kc) * ldb + cb0], b1 = Bb[int64_t(kc) * ldb + cb1];
    if (!ok) { a0 = 0.0; a1 = 0.0; b0 = 0.0; b1 = 0.0; }
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// Level b of the triangular inversion.  The wavefront's 32 x 32 tile at rows i0, columns j0 belongs to the pair s = i0 / (2 b): block 1
// = columns [c0, c0 + b), block 2 = rows [r0, min(r0 + b, n)), c0 = 2 s b, r0 = c0 + b.  kStep 1: T = L21 X11 -> W (X11 is lower
// triangular: k from j0); kStep 2: X21 = -X22 T -> A over L21 (X22 is lower triangular: k up to the tile's last row).  Reads and writes
// of a launch touch different regions: step 1 writes W only, step 2 reads A's diagonal pairs' block 2 and W and writes A's block (2, 1).
template <int kStep>
__global__ __launch_bounds__(256) void cov_trtri_gemm_kernel(double* A, double* W, int n, int b) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const int i0 = 64 * blockIdx.y + kCovBase * (wv >> 1);
  const int jo = 64 * blockIdx.x + kCovBase * (wv & 1);
  if (i0 >= n || jo >= b) return;
  const int c0 = i0 / (2 * b) * (2 * b), r0 = c0 + b;
  if (i0 < r0) return;   // a row of block 1
  const int j0 = c0 + jo;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = v4f64{0.0, 0.0, 0.0, 0.0};
  if (kStep == 1) cov_mma_32x32<false>(A, n, i0, A, n, j0, n - 1, j0, r0, n, li, lq, acc);
  else cov_mma_32x32<false>(A, n, i0, W, n, j0, n - 1, r0, i0 + kCovBase, n, li, lq, acc);
  double* out = kStep == 1 ? W : A;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * a + lq + 4 * r, j = j0 + 16 * c + li;   // (j < r0 <= i0 < n)
        if (i < n) out[int64_t(i) * n + j] = kStep == 1 ? acc[a][c][r] : -acc[a][c][r];
      }
}

// W[i][j] = W[j][i] = lam_i lam_j sum_{k >= i} X[k][i] X[k][j] for j <= i.  X lower triangular in A (zeros above the diagonal inside
// the 32 x 32 diagonal blocks; nothing above them is read: k starts at the tile's first row).
__global__ __launch_bounds__(256) void cov_xtx_kernel(const double* __restrict__ A, int n, const double* __restrict__ lam, double* __restrict__ W) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const int i0 = 64 * blockIdx.y + kCovBase * (wv >> 1);
  const int j0 = 64 * blockIdx.x + kCovBase * (wv & 1);
  if (i0 >= n || j0 > i0) return;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = v4f64{0.0, 0.0, 0.0, 0.0};
  cov_mma_32x32<true>(A, n, i0, A, n, j0, n - 1, i0, (n + 3) / 4 * 4, n, li, lq, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 16 * a + lq + 4 * r, j = j0 + 16 * c + li;
        if (i < n && j <= i) {
          const double v = acc[a][c][r] * lam[i] * lam[j];
          W[int64_t(i) * n + j] = v;
          W[int64_t(j) * n + i] = v;
        }
      }
}

// ---- blocks ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cov_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Y (3 x CW) = C_p^-1 E^T F of one observation: E 2 x 3 and F 2 x CW row-major in the caller-layout values
template <int CW>
__device__ __forceinline__ void cov_load_y(const double* __restrict__ values, const double* __restrict__ cinv, int epos, int fpos, double (&Y)[3][CW]) {
  const double* E = values + epos;
  const double* F = values + fpos;
  double e[2][3], ci[9];
#pragma unroll
  for (int t = 0; t < 6; ++t) e[t / 3][t % 3] = E[t];
#pragma unroll
  for (int t = 0; t < 9; ++t) ci[t] = cinv[t];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const double f0 = F[c], f1 = F[CW + c];
    double w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = e[0][a] * f0 + e[1][a] * f1;
#pragma unroll
    for (int a = 0; a < 3; ++a) Y[a][c] = ci[3 * a] * w[0] + ci[3 * a + 1] * w[1] + ci[3 * a + 2] * w[2];
  }
}

// One wavefront per pair.  A block's code is 4 index + kind (CovBlocksArgs); the index of a point is its column among the free points,
// of a camera among the free cameras.  The lanes take the (observation of a, observation of b) pairs 64 at a time, every lane adds its
// own in ascending order, the lanes are added by a butterfly: one order, whatever the grid.  (b, a) is computed as (a, b) and stored
// transposed.
template <int CW>
__global__ __launch_bounds__(256) void cov_blocks_kernel(CovBlocksArgs P) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= P.n_pairs) return;
  const int lane = threadIdx.x & 63;
  int ca = P.code_a[pair], cb = P.code_b[pair];
  double* out = P.out + P.out_off[pair];
  int ka = ca & 3, kb = cb & 3;
  const int da = (ka == kCovPoint || ka == kCovConstPoint) ? 3 : CW, db = (kb == kCovPoint || kb == kCovConstPoint) ? 3 : CW;
  if (ka == kCovConstPoint || ka == kCovConstCamera || kb == kCovConstPoint || kb == kCovConstCamera) {
    for (int e = lane; e < da * db; e += 64) out[e] = 0.0;
    return;
  }
  const int n = P.n;
  if (ka == kCovCamera && kb == kCovCamera) {
    const double* B = P.sinv + int64_t(CW) * (ca >> 2) * n + int64_t(CW) * (cb >> 2);
    for (int e = lane; e < CW * CW; e += 64) out[e] = B[int64_t(e / CW) * n + e % CW];
    return;
  }
  if (ka == kCovPoint && kb == kCovPoint) {
    const bool swap = (ca >> 2) > (cb >> 2);
    const int p = swap ? cb >> 2 : ca >> 2, q = swap ? ca >> 2 : cb >> 2;
    const int p0 = P.pt_ptr[p], np = P.pt_ptr[p + 1] - p0, q0 = P.pt_ptr[q], nq = P.pt_ptr[q + 1] - q0;
    double R[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const int64_t total = int64_t(np) * nq;
    for (int64_t t = lane; t < total; t += 64) {
      const int k = p0 + int(t / nq), l = q0 + int(t % nq);
      double Yk[3][CW], Yl[3][CW];
      cov_load_y<CW>(P.values, P.cinv + 9 * int64_t(p), P.ent_epos[k], P.ent_fpos[k], Yk);
      cov_load_y<CW>(P.values, P.cinv + 9 * int64_t(q), P.ent_epos[l], P.ent_fpos[l], Yl);
      const double* B = P.sinv + int64_t(CW) * P.ent_ccol[k] * n + int64_t(CW) * P.ent_ccol[l];
#pragma unroll
      for (int c = 0; c < CW; ++c) {   // column c of M = Yk B, then R += M[:, c] Yl[:, c]^T
        double m[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < CW; ++d) {
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
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int g = 0; g < 3; ++g) R[a][g] = cov_wave_sum(R[a][g]);
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
  // point - camera, or camera - point stored transposed: -sum_k Y_k S^-1[c_k, c]
  const bool swap = ka == kCovCamera;
  const int p = swap ? cb >> 2 : ca >> 2, cam = swap ? ca >> 2 : cb >> 2;
  const int p0 = P.pt_ptr[p], np = P.pt_ptr[p + 1] - p0;
  double M[3][CW];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < CW; ++c) M[a][c] = 0.0;
  for (int t = lane; t < np; t += 64) {
    const int k = p0 + t;
    double Yk[3][CW];
    cov_load_y<CW>(P.values, P.cinv + 9 * int64_t(p), P.ent_epos[k], P.ent_fpos[k], Yk);
    const double* B = P.sinv + int64_t(CW) * P.ent_ccol[k] * n + int64_t(CW) * cam;
#pragma unroll
    for (int d = 0; d < CW; ++d)
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const double bv = B[int64_t(d) * n + c];
#pragma unroll
        for (int a = 0; a < 3; ++a) M[a][c] += Yk[a][d] * bv;
      }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < CW; ++c) M[a][c] = cov_wave_sum(M[a][c]);
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        if (swap) out[3 * c + a] = -M[a][c]; else out[CW * a + c] = -M[a][c];
      }
  }
}

inline unsigned cov_blocks_for(int64_t n) { return unsigned((n + kVecBlock - 1) / kVecBlock); }

}  // namespace

hipError_t LaunchCovPointFactor(int n_points, double* blocks, double* pivot, hipStream_t s) {
  if (n_points > 0) hipLaunchKernelGGL(cov_point_factor_kernel, dim3(cov_blocks_for(n_points)), dim3(kVecBlock), 0, s, n_points, blocks, pivot);
  return hipGetLastError();
}
hipError_t LaunchCovMin(const double* v, int64_t count, int64_t stride, int square, double* out, hipStream_t s) {
  hipLaunchKernelGGL(cov_min_kernel, dim3(1), dim3(kVecBlock), 0, s, v, count, stride, square, out);
  return hipGetLastError();
}
hipError_t LaunchCovScale(double* S, int n, double* lam, int* flag, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cov_diag_scale_kernel, dim3(cov_blocks_for(n)), dim3(kVecBlock), 0, s, S, n, lam, flag);
  hipLaunchKernelGGL(cov_scale_kernel, dim3(cov_blocks_for(int64_t(n) * n)), dim3(kVecBlock), 0, s, S, n, lam);
  return hipGetLastError();
}
hipError_t LaunchCovInverseFromFactor(double* A, int n, const double* lam, double* W, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cov_diag_inverse_kernel, dim3((n + kCovBase - 1) / kCovBase), dim3(kCovBase), 0, s, A, n);
  const unsigned rows = unsigned((n + 63) / 64);
  for (int64_t b = kCovBase; b < n; b *= 2) {
    const dim3 grid(unsigned(std::max<int64_t>(1, b / 64)), rows);
    hipLaunchKernelGGL(cov_trtri_gemm_kernel<1>, grid, dim3(256), 0, s, A, W, n, int(b));
    hipLaunchKernelGGL(cov_trtri_gemm_kernel<2>, grid, dim3(256), 0, s, A, W, n, int(b));
  }
  hipLaunchKernelGGL(cov_xtx_kernel, dim3(rows, rows), dim3(256), 0, s, A, n, lam, W);
  return hipGetLastError();
}
hipError_t LaunchCovBlocks(const CovBlocksArgs& P, int cw, hipStream_t s) {
  if (P.n_pairs <= 0) return hipSuccess;
  const dim3 grid(unsigned((P.n_pairs + 3) / 4));
  if (cw == 9) hipLaunchKernelGGL(cov_blocks_kernel<9>, grid, dim3(256), 0, s, P);
  else if (cw == 10) hipLaunchKernelGGL(cov_blocks_kernel<10>, grid, dim3(256), 0, s, P);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace chip
