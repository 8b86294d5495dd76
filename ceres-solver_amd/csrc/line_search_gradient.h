// line_search_gradient.h — cost and gradient of a BAL problem WITHOUT a Jacobian in memory (Evaluator::Evaluate(state, cost, nullptr,
// gradient, nullptr), I/program_evaluator.h), a template on the camera model.  kernels_line_search.hip instantiates the angle-axis
// camera, kernels_line_search_quat.hip the two quaternion cameras (a translation unit of their own, for the reason bal_evaluate.h gives).
//
// Two passes, each evaluating its observations from the state (snavely.h, robust_loss.h) — per observation nothing but the index, pixel
// and state reads touches memory; the gradient of one observation is rho' J^T r (= J~^T r~ of the Corrector):
//
//   POINT PASS   over the rows (grouped by point).  One lane per row, one wavefront per CHUNK of 64 consecutive rows; wavefront w of
//                the launch takes the chunks w, w + W, w + 2 W, ... (W wavefronts in the launch, a fixed number).  Inside a chunk the
//                lanes' contributions are added by a segmented inclusive scan keyed on the point (shuffles, distances 1, 2, 4 .. 32 —
//                a fixed tree).  A point whose rows all lie in one chunk is written by the last lane of its run.  Every chunk also
//                stores the sum of its FIRST and of its LAST run (6 doubles per 64 rows); a point whose run crosses a chunk boundary
//                is finished by ls_point_finish_kernel: last-run sum of its first chunk, then the first-run sums of its other chunks
//                in ascending order.  The cost: each lane adds its rows' rho / 2 in chunk order, the lanes are added by the xor
//                butterfly, the four wavefronts as (0 + 1) + (2 + 3), and the host adds the workgroups' partials in index order.
//   CAMERA PASS  over per-camera observation lists (rows in ascending order), cut into chunks of at most 64 entries of ONE camera.
//                One lane per entry, the lanes added by the xor butterfly.  A camera of one chunk is written directly; the chunks of a
//                longer one go to chunk partials, which ls_camera_finish_kernel adds in ascending order.
//
// No atomics: the order of every sum is fixed by the structure alone, so two calls at one state give the same bits.  Every tangent
// entry of a free block is stored on every call (by one of the four kernels), whatever the buffer held before.
#pragma once
#include <hip/hip_runtime.h>

#include "device.h"
#include "reduce.h"
#include "robust_loss.h"
#include "snavely.h"

namespace chip {

namespace {

// residual, Jacobian and the loss of one observation: w = rho' (1 without a loss), half_rho = the observation's cost
template <int CM, bool ROBUST, bool JAC>
__device__ __forceinline__ void ls_observation(const LsGradArgs& A, int c, int p, double2 o, double (&res)[2],
                                               double (&jc)[CM == kCamQuaternion ? 20 : 18], double (&jp)[6], double& w, double& half_rho) {
  constexpr int SW = CM == kCamAngleAxis ? 9 : 10;
  double cam[SW], X[3];
  const double* cs = A.state + A.cam_base + SW * int64_t(c);
  const double* ps = A.state + 3 * int64_t(p);
#pragma unroll
  for (int i = 0; i < SW; ++i) cam[i] = cs[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) X[i] = ps[i];
  if constexpr (CM == kCamAngleAxis) snavely<JAC>(cam, X, o.x, o.y, res, jc, jp);
  else snavely_quat<JAC, CM == kCamQuaternionManifold>(cam, X, o.x, o.y, res, jc, jp);
  const double sq = res[0] * res[0] + res[1] * res[1];
  if constexpr (ROBUST) {
    double rho[3];
    robust_rho(A.loss, sq, rho);
    half_rho = 0.5 * rho[0];
    w = rho[1];
  } else {
    half_rho = 0.5 * sq;
    w = 1.0;
  }
}

// GRAD = false: the cost alone (no Jacobian is evaluated, nothing but the cost partials is stored)
template <int CM, bool ROBUST, bool GRAD>
__global__ __launch_bounds__(kVecBlock) void ls_point_pass_kernel(LsGradArgs A) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_chunks = (A.n_rows + 63) >> 6;
  double cost = 0.0;
  for (int64_t ch = int64_t(blockIdx.x) * 4 + wave; ch < n_chunks; ch += int64_t(gridDim.x) * 4) {
    const int64_t base = ch * 64, r = base + lane;
    const bool valid = r < A.n_rows;
    int key = -2;   // where the row's point starts in the tangent vector; -1: a constant point; -2: no row
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (valid) {
      double res[2], jc[CM == kCamQuaternion ? 20 : 18], jp[6], w, hr;
      ls_observation<CM, ROBUST, GRAD>(A, A.row_cam[r], A.row_pt[r], A.row_obs[r], res, jc, jp, w, hr);
      cost += hr;
      if constexpr (GRAD) {
        key = A.row_pdst[r];
        g0 = w * (jp[0] * res[0] + jp[3] * res[1]);
        g1 = w * (jp[1] * res[0] + jp[4] * res[1]);
        g2 = w * (jp[2] * res[0] + jp[5] * res[1]);
      }
    }
    if constexpr (GRAD) {
      const int key_before = __shfl_up(key, 1, 64), key_after = __shfl_down(key, 1, 64);
      const bool head = lane == 0 || key_before != key;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {   // runs are contiguous: the lane d below belongs to this run iff its key is this one
        const int kd = __shfl_up(key, d, 64);
        const double a0 = __shfl_up(g0, d, 64), a1 = __shfl_up(g1, d, 64), a2 = __shfl_up(g2, d, 64);
        if (lane >= d && kd == key) { g0 += a0; g1 += a1; g2 += a2; }
      }
      const unsigned long long heads = __ballot(head);
      const bool tail = valid && (lane == 63 || key_after != key);
      if (tail) {
        const int start = 63 - __clzll(heads & ((2ull << lane) - 1ull));   // the run's first lane
        const bool first_run = start == 0, last_run = lane == 63 || r == A.n_rows - 1;
        double* wp = A.wave_parts + 6 * ch;
        if (first_run) { wp[0] = g0; wp[1] = g1; wp[2] = g2; }
        if (last_run) { wp[3] = g0; wp[4] = g1; wp[5] = g2; }
        if (key >= 0) {
          const bool from_before = first_run && base > 0 && A.row_pdst[base - 1] == key;
          const bool goes_on = lane == 63 && r + 1 < A.n_rows && A.row_pdst[r + 1] == key;
          if (!from_before && !goes_on) { A.grad[key] = g0; A.grad[key + 1] = g1; A.grad[key + 2] = g2; }
        }
      }
    }
  }
  cost = wave_sum(cost);
  if (lane == 0) sh[wave] = cost;
  __syncthreads();
  if (threadIdx.x == 0) A.cost_partials[blockIdx.x] = lds_sum4(sh);
}

template <int CM, bool ROBUST>
__global__ __launch_bounds__(kVecBlock) void ls_camera_pass_kernel(LsGradArgs A) {
  constexpr int CW = CM == kCamQuaternion ? 10 : 9;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t ch = int64_t(blockIdx.x) * 4 + wave; ch < A.n_chunks; ch += int64_t(gridDim.x) * 4) {
    const int c = A.chunk_cam[ch], start = A.chunk_start[ch], len = A.chunk_len[ch], dst = A.chunk_dst[ch];
    double g[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) g[j] = 0.0;
    if (lane < len) {
      const int64_t e = int64_t(start) + lane;
      double res[2], jc[2 * CW], jp[6], w, hr;
      ls_observation<CM, ROBUST, true>(A, c, A.cm_pt[e], A.cm_obs[e], res, jc, jp, w, hr);
#pragma unroll
      for (int j = 0; j < CW; ++j) g[j] = w * (jc[j] * res[0] + jc[CW + j] * res[1]);
    }
    double mine = 0.0;
#pragma unroll
    for (int j = 0; j < CW; ++j) {
      const double t = wave_sum(g[j]);
      if (lane == j) mine = t;
    }
    if (lane < CW) {
      if (dst >= 0) A.grad[dst + lane] = mine;                       // the camera's only chunk
      else A.chunk_parts[kLsChunkPitch * int64_t(-dst - 1) + lane] = mine;
    }
  }
}

}  // namespace

}  // namespace chip
