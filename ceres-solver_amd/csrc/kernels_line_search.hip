// The line search minimizer's kernels (ceres_hip_bal_minimize_line_search, line_search.inc; gfx950, wave64):
//
//   (a) cost + gradient without a Jacobian: line_search_gradient.h (the angle-axis instantiations live here, the quaternion cameras'
//       in kernels_line_search_quat.hip), and the two kernels that finish the blocks of more than one chunk;
//   (b) the trial point Plus(x, t d) with |x|^2 and |x+ - x|^2, the gradient norms of x - Plus(x, -g), and the dot products of a trial
//       point — per-workgroup partial sums in a fixed order, added by the host in index order after ONE synchronisation;
//   (c) L-BFGS: the secant test, the circular buffer and the two-loop recursion with every scalar in device memory.
//
// (c) in detail.  All its vector kernels run on the same grid G <= kMaxVecGrid with the same grid-stride loop, so a workgroup always owns
// the same elements.  A dot product is G partials (lanes by the xor butterfly, the four wavefronts as (0 + 1) + (2 + 3)); its consumer is
// the NEXT kernel, in which EVERY workgroup adds the G partials in the same fixed tree (lbfgs_total: p[t] + p[t + 256], then halving
// strides 128 .. 1 in LDS) — all workgroups get the same bits, no workgroup waits for another.  One step of the recursion is therefore one
// launch: finish the dot the previous launch left, apply the axpy to the own elements, leave the partials of the next dot.  The two sets
// of partials alternate, so a workgroup that is ahead never overwrites what a slower one still reads.  The number of live slots is
// device data: the host launches the steps for its upper bound, a step beyond the live count returns at once.  Order of operations:
// newest to oldest, the optional scale, oldest to newest, the negation (I/low_rank_inverse_hessian.cc:117-177, I/line_search_direction.cc:119-126).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device.h"
#include "reduce.h"
#include "line_search_gradient.h"
#include "quaternion_plus.h"

namespace chip {

namespace {

// the workgroup's sum / maximum of one value per thread (kVecBlock threads; sh: 4 doubles); every thread gets it
__device__ __forceinline__ double ls_block_sum(double v, double* sh) {
  v = wave_sum(v);
  wave_to_lds(v, sh);
  __syncthreads();
  const double r = lds_sum4(sh);
  __syncthreads();
  return r;
}
__device__ __forceinline__ double ls_block_max(double v, double* sh) {
  v = wave_max(v);
  wave_to_lds(v, sh);
  __syncthreads();
  const double r = lds_max4(sh);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kVecBlock) void ls_point_finish_kernel(LsGradArgs A) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= A.n_long) return;
  const int w0 = A.long_w0[i], w1 = A.long_w1[i], dst = A.long_dst[i];
  double g0 = A.wave_parts[6 * int64_t(w0) + 3], g1 = A.wave_parts[6 * int64_t(w0) + 4], g2 = A.wave_parts[6 * int64_t(w0) + 5];
  for (int w = w0 + 1; w <= w1; ++w) {   // chunk partials, ascending
    g0 += A.wave_parts[6 * int64_t(w)]; g1 += A.wave_parts[6 * int64_t(w) + 1]; g2 += A.wave_parts[6 * int64_t(w) + 2];
  }
  A.grad[dst] = g0; A.grad[dst + 1] = g1; A.grad[dst + 2] = g2;
}

// one thread per (camera of more than one chunk, tangent entry)
__global__ __launch_bounds__(kVecBlock) void ls_camera_finish_kernel(LsGradArgs A, int cw) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= A.n_fin * cw) return;
  const int f = i / cw, j = i - f * cw;
  const int first = A.fin_first[f], count = A.fin_count[f];
  double g = 0.0;
  for (int k = 0; k < count; ++k) g += A.chunk_parts[kLsChunkPitch * int64_t(first + k) + j];   // chunk partials, ascending
  A.grad[A.fin_dst[f] + j] = g;
}

// One work item per free block (its first double in the full state from the list, its tangent entries by its index).  NORMS = false:
// out = Plus(x, t v), sums |x|^2 and |out - x|^2.  NORMS = true: nothing is stored, diff = x - Plus(x, -v), sums |diff|^2 and max |diff|.
template <int CM, bool NORMS>
__global__ __launch_bounds__(kVecBlock) void ls_plus_kernel(BalFreeBlocks B, const double* x, const double* v, double t, double* out, double* partials) {
  constexpr int SW = CM == kCamAngleAxis ? 9 : 10;
  constexpr int CW = CM == kCamQuaternion ? 10 : 9;
  __shared__ double sh[4];
  double s0 = 0.0, s1 = 0.0;   // !NORMS: |x|^2, |out - x|^2; NORMS: |diff|^2, max |diff|
  const int64_t nfp = B.n_free_points, n = nfp + B.n_free_cameras;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    const int64_t a = B.block[i];
    const bool point = i < nfp;
    const int64_t tb = point ? 3 * i : 3 * nfp + CW * (i - nfp);
    const int width = point ? 3 : SW;
    int j0 = 0, tj = 0;   // ambient / tangent entry the element-wise part starts at
    if (CM == kCamQuaternionManifold && !point) {
      double q[4], qp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = x[a + k];
      quaternion_plus(q, t * v[tb], t * v[tb + 1], t * v[tb + 2], qp);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (NORMS) {
          const double d = q[k] - qp[k];
          s0 += d * d; s1 = fmax(s1, fabs(d));
        } else {
          const double d = qp[k] - q[k];
          out[a + k] = qp[k];
          s0 += q[k] * q[k]; s1 += d * d;
        }
      }
      j0 = 4; tj = 3;
    }
    for (int j = j0; j < width; ++j, ++tj) {
      const double xi = x[a + j];
      const double xo = xi + t * v[tb + tj];
      if constexpr (NORMS) {
        const double d = xi - xo;
        s0 += d * d; s1 = fmax(s1, fabs(d));
      } else {
        const double d = xo - xi;
        out[a + j] = xo;
        s0 += xi * xi; s1 += d * d;
      }
    }
  }
  s0 = ls_block_sum(s0, sh);
  s1 = NORMS ? ls_block_max(s1, sh) : ls_block_sum(s1, sh);
  if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[gridDim.x + blockIdx.x] = s1; }
}

__global__ __launch_bounds__(kVecBlock) void ls_dots_kernel(const double* a, const double* b, const double* c, int64_t n, double* partials) {
  __shared__ double sh[4];
  double ab = 0.0, ac = 0.0, m = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    const double ai = a[i];
    ab += ai * b[i];
    if (c) ac += ai * c[i];
    m = fmax(m, fabs(ai));
  }
  ab = ls_block_sum(ab, sh); ac = ls_block_sum(ac, sh); m = ls_block_max(m, sh);
  if (threadIdx.x == 0) { partials[blockIdx.x] = ab; partials[gridDim.x + blockIdx.x] = ac; partials[2 * gridDim.x + blockIdx.x] = m; }
}

__global__ __launch_bounds__(kVecBlock) void ls_combine_kernel(double alpha, const double* x, double beta, const double* y, double gamma, const double* w,
                                                               double* z, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kVecBlock) {
    double v = alpha * x[i];
    if (y) v += beta * y[i];
    if (w) v -= gamma * w[i];
    z[i] = v;
  }
}

// ---- L-BFGS ----
// the sum of G <= 2 kVecBlock partials in a fixed tree; every thread of the workgroup gets it (sh: kVecBlock doubles)
__device__ __forceinline__ double lbfgs_total(const double* p, int G, double* sh) {
  const int t = threadIdx.x;
  double v = t < G ? p[t] : 0.0;
  if (t + kVecBlock < G) v += p[t + kVecBlock];
  sh[t] = v;
  __syncthreads();
  for (int s = kVecBlock / 2; s >= 1; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ void lbfgs_reset_kernel(LbfgsArgs A) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { *A.count = 0; *A.scale = 1.0; }
}

// partials of s . y (set 0) and y . y (set 1), s = a sv, y = y1 - y0
__global__ __launch_bounds__(kVecBlock) void lbfgs_update_dots_kernel(LbfgsArgs A, double a, const double* sv, const double* y1, const double* y0) {
  __shared__ double sh[4];
  double sy = 0.0, yy = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < A.n; i += int64_t(gridDim.x) * kVecBlock) {
    const double s = a * sv[i], y = y0 ? y1[i] - y0[i] : y1[i];
    sy += s * y; yy += y * y;
  }
  sy = ls_block_sum(sy, sh); yy = ls_block_sum(yy, sh);
  if (threadIdx.x == 0) { A.parts[blockIdx.x] = sy; A.parts[kMaxVecGrid + blockIdx.x] = yy; }
}

// the secant test (delta_x . delta_gradient <= 1e-10: the update is skipped) in every workgroup; an accepted pair goes to the slot the
// circular buffer gives up next (the state itself is advanced by lbfgs_update_commit_kernel, after every workgroup has read it)
__device__ __forceinline__ bool lbfgs_accepts(double sy) { return !(sy <= 1e-10); }
__global__ __launch_bounds__(kVecBlock) void lbfgs_update_store_kernel(LbfgsArgs A, double a, const double* sv, const double* y1, const double* y0) {
  __shared__ double sh[kVecBlock];
  const double sy = lbfgs_total(A.parts, gridDim.x, sh);
  if (!lbfgs_accepts(sy)) return;
  const int count = *A.count;
  const int slot = count < A.rank ? count : A.order[0];
  double* S = A.S + int64_t(slot) * A.n;
  double* Y = A.Y + int64_t(slot) * A.n;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < A.n; i += int64_t(gridDim.x) * kVecBlock) {
    S[i] = a * sv[i];
    Y[i] = y0 ? y1[i] - y0[i] : y1[i];
  }
}
// one workgroup; G: the grid of the two kernels before
__global__ __launch_bounds__(kVecBlock) void lbfgs_update_commit_kernel(LbfgsArgs A, int G, int log_index) {
  __shared__ double sh[kVecBlock];
  const double sy = lbfgs_total(A.parts, G, sh);
  const double yy = lbfgs_total(A.parts + kMaxVecGrid, G, sh);
  if (threadIdx.x != 0) return;
  const bool ok = lbfgs_accepts(sy);
  if (A.accepted && log_index >= 0) A.accepted[log_index] = ok ? 1 : 0;
  if (!ok) return;
  const int count = *A.count;
  int slot = count;
  if (count < A.rank) {
    *A.count = count + 1;
  } else {   // the oldest slot becomes the newest
    slot = A.order[0];
    for (int k = 0; k + 1 < count; ++k) A.order[k] = A.order[k + 1];
  }
  A.order[count < A.rank ? count : count - 1] = slot;
  A.sy[slot] = sy;
  *A.scale = sy / yy;
}

// d . g and max |d| of the finished direction (sets 2 and 3)
__device__ __forceinline__ void lbfgs_store_final(const LbfgsArgs& A, double dg, double mx, double* sh4) {
  dg = ls_block_sum(dg, sh4); mx = ls_block_max(mx, sh4);
  if (threadIdx.x == 0) { A.parts[2 * kMaxVecGrid + blockIdx.x] = dg; A.parts[3 * kMaxVecGrid + blockIdx.x] = mx; }
}

// no live slot: d = -g.  Otherwise d = g and the partials of (newest delta_x) . d
__global__ __launch_bounds__(kVecBlock) void lbfgs_begin_kernel(LbfgsArgs A, const double* g, double* d) {
  __shared__ double sh4[4];
  const int count = *A.count;
  if (count == 0) {
    double dg = 0.0, mx = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < A.n; i += int64_t(gridDim.x) * kVecBlock) {
      const double gi = g[i], v = -gi;
      d[i] = v;
      dg += v * gi; mx = fmax(mx, fabs(v));
    }
    lbfgs_store_final(A, dg, mx, sh4);
    return;
  }
  const double* S = A.S + int64_t(A.order[count - 1]) * A.n;
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; i < A.n; i += int64_t(gridDim.x) * kVecBlock) {
    const double v = g[i];
    d[i] = v;
    acc += S[i] * v;
  }
  acc = ls_block_sum(acc, sh4);
  if (threadIdx.x == 0) A.parts[blockIdx.x] = acc;
}

// step j of the first loop (newest to oldest): alpha = (delta_x_i . d) / (s . y)_i from the partials the launch before left,
// d -= alpha delta_gradient_i, and the partials of the next dot — the next older delta_x, or after the last step (where the optional
// scale is applied) the oldest delta_gradient, which the second loop starts with
__global__ __launch_bounds__(kVecBlock) void lbfgs_first_loop_kernel(LbfgsArgs A, double* d, int j) {
  __shared__ double sh[kVecBlock];
  __shared__ double sh4[4];
  const int count = *A.count;
  if (j >= count) return;
  const int i = A.order[count - 1 - j];
  const double alpha = lbfgs_total(A.parts + (j & 1) * kMaxVecGrid, gridDim.x, sh) / A.sy[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) A.alpha[i] = alpha;
  const bool last = j + 1 == count;
  const bool scaled = last && A.use_scaling;
  const double sc = scaled ? *A.scale : 1.0;
  const double* Y = A.Y + int64_t(i) * A.n;
  const double* nxt = last ? A.Y + int64_t(A.order[0]) * A.n : A.S + int64_t(A.order[count - 2 - j]) * A.n;
  double acc = 0.0;
  for (int64_t k = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; k < A.n; k += int64_t(gridDim.x) * kVecBlock) {
    double v = d[k] - alpha * Y[k];
    if (scaled) v *= sc;
    d[k] = v;
    acc += nxt[k] * v;
  }
  acc = ls_block_sum(acc, sh4);
  if (threadIdx.x == 0) A.parts[((j + 1) & 1) * kMaxVecGrid + blockIdx.x] = acc;
}

// step j of the second loop (oldest to newest): beta = (delta_gradient_i . d) / (s . y)_i, d += delta_x_i (alpha_i - beta); the last step
// negates d and leaves d . g and max |d|
__global__ __launch_bounds__(kVecBlock) void lbfgs_second_loop_kernel(LbfgsArgs A, const double* g, double* d, int j) {
  __shared__ double sh[kVecBlock];
  __shared__ double sh4[4];
  const int count = *A.count;
  if (j >= count) return;
  const int i = A.order[j];
  const int q = count + j;   // the step's number over both loops: which set of partials it reads
  const double beta = lbfgs_total(A.parts + (q & 1) * kMaxVecGrid, gridDim.x, sh) / A.sy[i];
  const double coef = A.alpha[i] - beta;
  const double* S = A.S + int64_t(i) * A.n;
  if (j + 1 == count) {
    double dg = 0.0, mx = 0.0;
    for (int64_t k = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; k < A.n; k += int64_t(gridDim.x) * kVecBlock) {
      const double v = -(d[k] + S[k] * coef);
      d[k] = v;
      dg += v * g[k]; mx = fmax(mx, fabs(v));
    }
    lbfgs_store_final(A, dg, mx, sh4);
    return;
  }
  const double* nxt = A.Y + int64_t(A.order[j + 1]) * A.n;
  double acc = 0.0;
  for (int64_t k = int64_t(blockIdx.x) * kVecBlock + threadIdx.x; k < A.n; k += int64_t(gridDim.x) * kVecBlock) {
    const double v = d[k] + S[k] * coef;
    d[k] = v;
    acc += nxt[k] * v;
  }
  acc = ls_block_sum(acc, sh4);
  if (threadIdx.x == 0) A.parts[((q + 1) & 1) * kMaxVecGrid + blockIdx.x] = acc;
}

}  // namespace

hipError_t LaunchLsGradient(const LsGradArgs& A, bool gradient, int camera_model, int* nparts, hipStream_t stream) {
  if (A.n_rows <= 0 || !A.row_cam || !A.row_pt || !A.row_obs || !A.state || !A.cost_partials) return hipErrorInvalidValue;
  if (gradient && (!A.row_pdst || !A.grad || !A.wave_parts || A.n_chunks <= 0 || !A.chunk_cam || !A.cm_pt || !A.cm_obs)) return hipErrorInvalidValue;
  const int64_t row_chunks = (A.n_rows + 63) / 64;
  const int gp = int(std::min<int64_t>(kMaxEvalGrid, (row_chunks + 3) / 4));
  const int gc = int(std::min<int64_t>(kMaxLsCameraGrid, (int64_t(A.n_chunks) + 3) / 4));
  *nparts = gp;
  if (camera_model != kCamAngleAxis) {
    hipError_t e = LaunchLsGradientQuat(A, gradient, camera_model, gp, gc, stream);
    if (e != hipSuccess) return e;
  } else {
    const bool robust = A.loss.type != kLossNone;
    if (!gradient) {
      if (robust) hipLaunchKernelGGL((ls_point_pass_kernel<kCamAngleAxis, true, false>), dim3(gp), dim3(kVecBlock), 0, stream, A);
      else hipLaunchKernelGGL((ls_point_pass_kernel<kCamAngleAxis, false, false>), dim3(gp), dim3(kVecBlock), 0, stream, A);
      return hipGetLastError();
    }
    if (robust) {
      hipLaunchKernelGGL((ls_point_pass_kernel<kCamAngleAxis, true, true>), dim3(gp), dim3(kVecBlock), 0, stream, A);
      hipLaunchKernelGGL((ls_camera_pass_kernel<kCamAngleAxis, true>), dim3(gc), dim3(kVecBlock), 0, stream, A);
    } else {
      hipLaunchKernelGGL((ls_point_pass_kernel<kCamAngleAxis, false, true>), dim3(gp), dim3(kVecBlock), 0, stream, A);
      hipLaunchKernelGGL((ls_camera_pass_kernel<kCamAngleAxis, false>), dim3(gc), dim3(kVecBlock), 0, stream, A);
    }
  }
  if (!gradient) return hipGetLastError();
  if (A.n_long > 0) hipLaunchKernelGGL(ls_point_finish_kernel, dim3((A.n_long + kVecBlock - 1) / kVecBlock), dim3(kVecBlock), 0, stream, A);
  if (A.n_fin > 0) {
    const int cw = camera_model == kCamQuaternion ? 10 : 9;
    hipLaunchKernelGGL(ls_camera_finish_kernel, dim3((A.n_fin * cw + kVecBlock - 1) / kVecBlock), dim3(kVecBlock), 0, stream, A, cw);
  }
  return hipGetLastError();
}

hipError_t LaunchLsTrialPoint(const BalFreeBlocks& B, int camera_model, const double* x, const double* direction, double t, double* out,
                              double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(B.n_free_points + B.n_free_cameras, kMaxVecGrid);
  *nparts = grid;
  switch (camera_model) {
    case kCamAngleAxis: hipLaunchKernelGGL((ls_plus_kernel<kCamAngleAxis, false>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, direction, t, out, partials); break;
    case kCamQuaternion: hipLaunchKernelGGL((ls_plus_kernel<kCamQuaternion, false>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, direction, t, out, partials); break;
    case kCamQuaternionManifold:
      hipLaunchKernelGGL((ls_plus_kernel<kCamQuaternionManifold, false>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, direction, t, out, partials);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchLsGradientNorms(const BalFreeBlocks& B, int camera_model, const double* x, const double* g, double* partials, int* nparts,
                                 hipStream_t stream) {
  const int grid = vec_grid(B.n_free_points + B.n_free_cameras, kMaxVecGrid);
  *nparts = grid;
  switch (camera_model) {
    case kCamAngleAxis: hipLaunchKernelGGL((ls_plus_kernel<kCamAngleAxis, true>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, g, -1.0, nullptr, partials); break;
    case kCamQuaternion: hipLaunchKernelGGL((ls_plus_kernel<kCamQuaternion, true>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, g, -1.0, nullptr, partials); break;
    case kCamQuaternionManifold:
      hipLaunchKernelGGL((ls_plus_kernel<kCamQuaternionManifold, true>), dim3(grid), dim3(kVecBlock), 0, stream, B, x, g, -1.0, nullptr, partials);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchLsDots(const double* a, const double* b, const double* c, int64_t n, double* partials, int* nparts, hipStream_t stream) {
  const int grid = vec_grid(n, kMaxVecGrid);
  *nparts = grid;
  hipLaunchKernelGGL(ls_dots_kernel, dim3(grid), dim3(kVecBlock), 0, stream, a, b, c, n, partials);
  return hipGetLastError();
}

hipError_t LaunchLsCombine(double alpha, const double* x, double beta, const double* y, double gamma, const double* w, double* z, int64_t n,
                           hipStream_t stream) {
  hipLaunchKernelGGL(ls_combine_kernel, dim3(vec_grid(n, kMaxVecGrid)), dim3(kVecBlock), 0, stream, alpha, x, beta, y, gamma, w, z, n);
  return hipGetLastError();
}

hipError_t LaunchLbfgsReset(const LbfgsArgs& A, hipStream_t stream) {
  hipLaunchKernelGGL(lbfgs_reset_kernel, dim3(1), dim3(64), 0, stream, A);
  return hipGetLastError();
}

hipError_t LaunchLbfgsUpdate(const LbfgsArgs& A, double a, const double* sv, const double* y1, const double* y0, int log_index, hipStream_t stream) {
  if (A.n <= 0 || A.rank <= 0) return hipErrorInvalidValue;
  const int grid = vec_grid(A.n, kMaxVecGrid);
  hipLaunchKernelGGL(lbfgs_update_dots_kernel, dim3(grid), dim3(kVecBlock), 0, stream, A, a, sv, y1, y0);
  hipLaunchKernelGGL(lbfgs_update_store_kernel, dim3(grid), dim3(kVecBlock), 0, stream, A, a, sv, y1, y0);
  hipLaunchKernelGGL(lbfgs_update_commit_kernel, dim3(1), dim3(kVecBlock), 0, stream, A, grid, log_index);
  return hipGetLastError();
}

hipError_t LaunchLbfgsDirection(const LbfgsArgs& A, const double* g, double* d, int max_live, int* nparts, hipStream_t stream) {
  if (A.n <= 0 || A.rank <= 0) return hipErrorInvalidValue;
  const int grid = vec_grid(A.n, kMaxVecGrid);
  *nparts = grid;
  const int steps = std::min(max_live, int(A.rank));
  hipLaunchKernelGGL(lbfgs_begin_kernel, dim3(grid), dim3(kVecBlock), 0, stream, A, g, d);
  for (int j = 0; j < steps; ++j) hipLaunchKernelGGL(lbfgs_first_loop_kernel, dim3(grid), dim3(kVecBlock), 0, stream, A, d, j);
  for (int j = 0; j < steps; ++j) hipLaunchKernelGGL(lbfgs_second_loop_kernel, dim3(grid), dim3(kVecBlock), 0, stream, A, g, d, j);
  return hipGetLastError();
}

}  // namespace chip
