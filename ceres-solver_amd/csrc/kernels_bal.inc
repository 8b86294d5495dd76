// kernels_bal.hip — fused single-pass kernels for the static <2,3,9> (BAL) structure.
//
// Data layout in HBM (built once per LM step from the caller's values, whatever their layout — by the step's first pass over
// J, which gathers through cell.position and writes the tiles on the way; bal_pack_kernel is the stand-alone form):
//   tiles of 64 observation slots, one wavefront per tile;
//   J   [tile][12][64] double2   pair j of slot l holds Jacobian doubles (2j, 2j+1) of the
//                                24 = 6 (E, 2x3 row-major) + 18 (F, 2x9 row-major)
//   b   [tile][64]     double2   the two residuals of the slot
//   cam [tile][64] int32, seg [tile][64] uint32 (first | last<<8 | valid<<16 | store lanes of the tile's dense point range),
//   pt0 [tile] int32             points of a tile are consecutive ids: a slot's point = pt0 + (segment heads at or below it) - 1
// so that every global load of the hot kernels is a 16-byte-per-lane, 1 KiB-per-wave
// contiguous access and the algorithmic traffic is 192 + 8 bytes per observation.  Streamed-once data is read with
// non-temporal loads (stream_load<>), the tiles are written with non-temporal stores (tile_store<>).
//
// All per-point reductions (E^T·, (E^T E)^-1) are segmented wavefront scans over
// __shfl_up — observations of a point are adjacent lanes by construction of the
// plan (plan.cc); points longer than 64 observations own whole tiles, which sit behind the
// normal ones and are taken in ROUNDS: one tile per wave of a workgroup, the tile sums exchanged
// through LDS, every tile finished from registers (compute_long_round, fused_long_rounds).  Per-camera sums (F^T·) go to a
// workgroup-private accumulator in LDS (9 doubles per camera: 128 KB for Venice's
// 1778 cameras, LDS is 160 KB) with ds_add_f64, flushed once per workgroup and
// combined by bal_reduce_partials_kernel; when the cameras do not fit in LDS the tile pass leaves F_o^T z_o per slot
// (72-byte rows, transposed through LDS into coalesced stores) and bal_camera_chunk_kernel sums them camera by camera.
// Camera-major work on the Jacobian itself (the 9x9 preconditioner blocks) is bal_camera_items_kernel / bal_camera_items_mfma_kernel
// (per-item partial sums: lane per observation, or — short items — the matrix pipe) + bal_invert9_kernel (sums a camera's items,
// adds D^2 or the fused LM diagonal, inverts).  For camera spaces of a few hundred scalars the S.x pass also finishes the CG
// iteration (cg_iteration_tail).
//
// Reference operators restated by each MODE (file:line in include/ceres_hip.h):
//   kSx        ImplicitSchurComplement::RightMultiplyAndAccumulate (4 passes there, 1 here)
//   kJtJx      CgnrLinearOperator::RightMultiplyAndAccumulate      (2 passes there, 1 here); also leaves partial sums of x . y
//   kJtb       A^T b
//   kInit      ImplicitSchurComplement::Init: (E^T E + D^2)^-1, rhs; also the 2x2 blocks
//              M_o = I - E_o (E^T E)^-1 E_o^T that SCHUR_JACOBI needs, and the fused LM diagonal of the point columns
//   kCgnrInit  J^T b, the point blocks of JACOBI and the fused LM diagonal, in one pass
//   kEte       block diagonal (E^T E + D^2)^-1 only (CGNR JACOBI point blocks)
//   kColNorm   BlockSparseMatrix::SquaredColumnNorm
//   kBackSub   ImplicitSchurComplement::BackSubstitute; as the last kernel of an LM step also the negation, the finite check
//              and the model-cost partial sums (gated on the CG status word when enqueued speculatively)
//   kSpseZ     the inverse power-series operator of SCHUR_POWER_SERIES_EXPANSION (S.x without the F^T F term)
//   kJx        J x (model cost where nothing else has it in hand)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

#include "device.h"
#include "p2p.h"
#ifndef CERES_HIP_NE
#define CERES_HIP_NE 3   // width of the point (E) blocks: 3 unless the shape's translation unit says otherwise (2, 4: common.h)
#endif
#ifndef CERES_HIP_NR
#define CERES_HIP_NR 2   // height of the row blocks (residuals per observation): 2 unless the translation unit says otherwise (3, 4)
#endif
// the software-pipelined streaming kernels and their cooperative point-space accesses: 2-high rows on 3-wide points
#if CERES_HIP_NE == 3 && CERES_HIP_NR == 2
#define CERES_HIP_PIPELINED 1
#else
#define CERES_HIP_PIPELINED 0
#endif
#if CERES_HIP_NR == 2 && CERES_HIP_NE == 3 && CERES_HIP_NF == 9 && CERES_HIP_NS == 0
#define CERES_HIP_IS_BAL_SHAPE 1
#include "robust_loss.h"
#include "snavely.h"
#else
#define CERES_HIP_IS_BAL_SHAPE 0
#endif

#if !defined(CERES_HIP_NF) || !defined(CERES_HIP_NS) || !defined(CERES_HIP_SHAPE)
#error "kernels_bal.inc is compiled once per shape through kernels_bal_shape_*.hip (CERES_HIP_NF, CERES_HIP_NS, CERES_HIP_SHAPE)"
#endif

namespace chip {
namespace CERES_HIP_SHAPE {

// The SHAPE of this translation unit (common.h): point blocks NE wide, camera blocks NF wide, a shared strip of NS scalars per row (0: none).
constexpr int NR = CERES_HIP_NR, NE = CERES_HIP_NE, NF = CERES_HIP_NF, NS = CERES_HIP_NS;
constexpr int NSX = NS > 0 ? NS : 1;            // array extent for the strip (no zero-length arrays)
constexpr int kVals = NR * (NE + NF + NS);      // doubles per slot: the E cell (NR x NE, row-major), the F cell (NR x NF), the strip (NR x NS)
constexpr int kPairs = (kVals + 1) / 2;         // double2 per slot (2-high rows: NE + NF + NS)
constexpr int kBPairs = (NR + 1) / 2;           // double2 per slot of the residual tiles: b[tile][kBPairs][64]
constexpr int kTriR = NR * (NR + 1) / 2;        // packed upper triangle of M_o = I - E (E^T E)^-1 E^T (NR x NR)
constexpr int kMoPitch = (kTriR + 1) / 2 * 2;   // doubles per M_o record (2-high rows: [m00 m01 m11 m01], 32 bytes)
__device__ __forceinline__ constexpr int tri_r(int a, int b) { return a * (2 * NR + 1 - a) / 2 + (b - a); }   // entry (a, b), a <= b, of a packed M_o
constexpr int kTriE = NE * (NE + 1) / 2;        // packed upper triangle of a point block: (0,0) (0,1) .. (1,1) ..
constexpr int kEteiPitch = (kTriE + 1) / 2 * 2; // doubles per point in the store of packed inverses (whole 16-byte records)
constexpr int kNX = kTriE + NE;                 // per-point sums of the set-up modes: E^T E, then E^T b
__device__ __forceinline__ constexpr int tri_e(int a, int b) { return a * (2 * NE + 1 - a) / 2 + (b - a); }   // entry (a, b), a <= b, of a packed point block
constexpr int kTilePitch = (kPairs + (CERES_HIP_AB_TILE_ROWS - 12)) * 64;   // double2 elements from one tile to the next
constexpr int kTri = NF * (NF + 1) / 2;         // packed upper triangle of a camera block
constexpr int kCamPart = kTri + NF;             // per-item partial sums: the triangle + the NF column square sums
constexpr bool kHasF32 = NR == 2 && NE == 3 && NF == 9 && NS == 0;    // fp32 tile storage (an accuracy mode) exists for the BAL shape only
constexpr bool kHasCgTail = NR == 2 && NE == 3 && NF == 9 && NS == 0; // so does the CG iteration inside the S.x pass (cg_iteration_tail)
constexpr int kTriS = NS * (NS + 1) / 2;       // packed upper triangle of the strip's own NS x NS matrix
constexpr int kTriSX = kTriS > 0 ? kTriS : 1;
constexpr int kPerWave = 64 / NF;               // cameras (or ring units) a wavefront takes NF lanes each
__device__ __forceinline__ constexpr int tri_index(int a, int b) { return a * (2 * NF + 1 - a) / 2 + (b - a); }   // entry (a, b), a <= b

namespace {

__device__ __forceinline__ double shfl_up(double v, int d) { return __shfl_up(v, (unsigned)d, 64); }
__device__ __forceinline__ double shfl_idx(double v, int l) { return __shfl(v, l, 64); }
__device__ __forceinline__ double shfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }

// Inclusive segmented scan (segments = runs of lanes [first,last]); afterwards the
// last lane of each segment holds the segment sum.  `span` bounds the longest
// segment in the tile (wave-uniform) so that short tracks take fewer steps.
template <int N>
__device__ __forceinline__ void seg_scan(double (&v)[N], int lane, int first, int span) {
  for (int d = 1; d < span; d <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double t = shfl_up(v[i], d);
      if (lane - d >= first) v[i] += t;
    }
  }
}
template <int N>
__device__ __forceinline__ void seg_allreduce(double (&v)[N], int lane, int first, int last, int span) {
  seg_scan<N>(v, lane, first, span);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = shfl_idx(v[i], last);
}
template <int N>
__device__ __forceinline__ void wave_allreduce(double (&v)[N]) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += shfl_xor(v[i], m);
  }
}

// Inverse of the SPD 3x3 matrix [a0 a1 a2; a1 a3 a4; a2 a4 a5] through its Cholesky
// factor (the reference: selfadjointView<Upper>().llt().solve(I),
// I/implicit_schur_complement.cc:179-204).  Output in the same packed order.
__device__ __forceinline__ void invert_spd3(const double (&a)[6], double (&o)[6]) {
  const double l00 = sqrt(a[0]);
  const double i00 = 1.0 / l00;
  const double l10 = a[1] * i00, l20 = a[2] * i00;
  const double l11 = sqrt(a[3] - l10 * l10);
  const double i11 = 1.0 / l11;
  const double l21 = (a[4] - l20 * l10) * i11;
  const double l22 = sqrt(a[5] - l20 * l20 - l21 * l21);
  const double i22 = 1.0 / l22;
  // W = L^-1 (lower): w00 w10 w11 w20 w21 w22
  const double w10 = -l10 * i00 * i11;
  const double w21 = -l21 * i11 * i22;
  const double w20 = -(l20 * i00 + l21 * w10) * i22;
  // A^-1 = W^T W
  o[0] = i00 * i00 + w10 * w10 + w20 * w20;
  o[1] = w10 * i11 + w20 * w21;
  o[2] = w20 * i22;
  o[3] = i11 * i11 + w21 * w21;
  o[4] = w21 * i22;
  o[5] = i22 * i22;
}

// The same for N x N (packed upper triangle, row by row): L column by column, W = L^-1, A^-1 = W^T W.  Point blocks of 2 and 4 scalars
// (the reference's (2,2,*) and (2,4,*) specialisations, internal/ceres/generate_template_specializations.py:55-75).
template <int N>
__device__ __forceinline__ void invert_spd_packed(const double (&a)[N * (N + 1) / 2], double (&o)[N * (N + 1) / 2]) {
  double L[N][N], W[N][N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = a[j * (2 * N + 1 - j) / 2];
#pragma unroll
    for (int k = 0; k < N; ++k) if (k < j) d -= L[j][k] * L[j][k];
    L[j][j] = sqrt(d);
    const double inv = 1.0 / L[j][j];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i <= j) continue;
      double v = a[j * (2 * N + 1 - j) / 2 + (i - j)];   // a(j, i) = a(i, j)
#pragma unroll
      for (int k = 0; k < N; ++k) if (k < j) v -= L[i][k] * L[j][k];
      L[i][j] = v * inv;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {   // column j of W = L^-1
    W[j][j] = 1.0 / L[j][j];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i <= j) continue;
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) if (k >= j && k < i) v += L[i][k] * W[k][j];
      W[i][j] = -v / L[i][i];
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (j < i) continue;
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) if (k >= j) v += W[k][i] * W[k][j];
      o[i * (2 * N + 1 - i) / 2 + (j - i)] = v;
    }
  }
}
template <>
__device__ __forceinline__ void invert_spd_packed<3>(const double (&a)[6], double (&o)[6]) { invert_spd3(a, o); }
__device__ __forceinline__ void invert_spd_e(const double (&a)[kTriE], double (&o)[kTriE]) { invert_spd_packed<NE>(a, o); }

// Streamed-once data is read with non-temporal loads: the L2 then evicts it first, and what is re-used (camera vectors, dirty
// point-space output lines, the partial sums) stays.  CERES_HIP_AB_NT_LOADS selects how far this goes in A/B builds
// (tools/build_variant.sh): 0 = nowhere, 1 = the 12 pairs of a packed tile in the pipelined kernels, 2 = + packed tiles and b in the
// unpipelined kernels (the product), 3 = + the caller-layout gathers of a step's first pass, 4 = + index words and per-point
// inverses.  Measured on the Venice shape (profiles/r02t_nt_load_levels_venice.txt): level 1 S.x 0.2138 -> 0.2000 ms and JtJx
// -7 %, level 2 back-substitution 0.252 -> 0.233 ms; level 3 is a disaster (non-temporal loads bypass the L1 that the per-lane
// 8-byte gathers of a 192-byte record live on: kInit 0.50 -> 0.75 ms) and level 4 costs S.x 2 %.
// The tiles a step's first pass writes on the way (fused re-layout) go out with non-temporal stores: 1 GB that the L2 cannot keep
// until its next reader anyway (kInit 0.484 -> 0.467 ms, CGNR set-up 0.734 -> 0.719 ms, stand-alone pack 0.376 -> 0.360 ms;
// profiles/r02v_nt_tile_stores_venice.txt).  CERES_HIP_AB_NT_TILE_STORES: 0 = plain stores, 1 = tiles, 2 = + M_o and (E^T E)^-1.
#ifndef CERES_HIP_AB_NT_TILE_STORES
#define CERES_HIP_AB_NT_TILE_STORES 1
#endif
// `plain` (launch-uniform, BalArgs::flags & 4): the whole tile stream fits the Infinity Cache, the pass that reads it next finds it
// on die if the stores are plain ones (the load side: issue_pairs<NT = false>).
template <int LEVEL = 1, typename T>
__device__ __forceinline__ void tile_store(T* p, const T& v, bool plain = false) {
  if (plain) { *p = v; return; }
#if CERES_HIP_AB_NT_TILE_STORES
  if constexpr (CERES_HIP_AB_NT_TILE_STORES < LEVEL) { *p = v; return; }
  typedef int v4 __attribute__((ext_vector_type(4)));
  static_assert(sizeof(T) == 16, "16-byte tile elements");
  v4 raw;
  __builtin_memcpy(&raw, &v, 16);
  __builtin_nontemporal_store(raw, reinterpret_cast<v4*>(p));
#else
  *p = v;
#endif
}
#ifndef CERES_HIP_AB_NT_LOADS
#define CERES_HIP_AB_NT_LOADS 2
#endif
#ifndef CERES_HIP_AB_PREFETCH
#define CERES_HIP_AB_PREFETCH 1
#endif
// Timing-only ablations of the streaming kernels (WRONG RESULTS; tools/gpu_r05m.sh): 1 = no LDS atomics, 2 = no camera-part gathers,
// 4 = no segmented scan, 8 = no per-point inverse loads, 16 = no scalar tile words inside a stage (kind / aux / pt0 constants),
// 32 / 64 = the camera-part gathers of the 440 most popular cameras / of all cameras redirected to one line
#ifndef CERES_HIP_AB_ABLATE
#define CERES_HIP_AB_ABLATE 0
#endif
// tiles in flight ahead of the one being computed in bal_stream_kernel's main loop: 1 = two register sets in ping-pong (rounds 1-4), 2 = three
#ifndef CERES_HIP_AB_PIPE_DEPTH
#define CERES_HIP_AB_PIPE_DEPTH 1
#endif
template <int LEVEL, typename T>
__device__ __forceinline__ T stream_load(const T* p) {
  if constexpr (CERES_HIP_AB_NT_LOADS >= LEVEL) {
    if constexpr (sizeof(T) == 16) {
      typedef int v4 __attribute__((ext_vector_type(4)));
      const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
      T out;
      __builtin_memcpy(&out, &v, 16);
      return out;
    } else {
      return __builtin_nontemporal_load(p);
    }
  } else {
    return *p;
  }
}

// What a thread carries through a kernel besides the slot: the workgroup's LDS accumulator (camera rows; nullptr in the modes that
// scatter nothing), and — shapes with a shared strip — the strip's part of x (wave-uniform, loaded once) and this lane's running sums of
// H^T z over all its slots (reduced over the workgroup into the accumulator entries behind the cameras' when the kernel ends).
struct Ctx {
  double* lds;
  double xs[NSX], hs[NSX];
  double tt[kTriSX];   // kShBlocks: this lane's share of the strip's own matrix (packed upper triangle)
};
__device__ __forceinline__ void ctx_init(const BalArgs& A, Ctx& c, double* lds) {
  c.lds = lds;
#pragma unroll
  for (int j = 0; j < NSX; ++j) { c.hs[j] = 0.0; c.xs[j] = (NS > 0 && A.x_f && A.sh_pos[j] >= 0) ? A.x_f[A.sh_pos[j]] : 0.0; }
#pragma unroll
  for (int j = 0; j < kTriSX; ++j) c.tt[j] = 0.0;
}

struct Slot {
  double e[NR * NE], f[NR * NF];   // the point cell (NR x NE, row-major) and the camera cell (NR x NF)
  double h[NR * NSX];  // the shared strip (NS > 0): row r at [r NS, (r + 1) NS)
  double b[NR];        // the slot's residuals
  int64_t slot;
  int64_t zbase;  // cameras not in LDS: ring row of the tile's first spilled slot (wave-uniform)
  uint32_t seg;
  int cam, pt, first, last;
  int acc;        // LDS accumulator row of the slot's camera (kSlotSpill: none, the slot's F^T z is spilled); plan.cc, slot_word
  bool valid;
  bool nocam;     // a valid slot without a camera cell (its F is zero; with accumulators outside LDS it is neither summed nor spilled)
  float4 raw[6];  // fp32 tiles in the PIPELINED kernels: the slot's 24 values as loaded; widened (widen_slot) in the stage that computes
};

// Derives the fields of a slot from its segment word.  The point id is not stored per slot (it was:
// 4 of 204 bytes per observation): points of a tile are consecutive ids starting at tile_pt0, so a
// slot's point is pt0 + (number of segment heads at or below its lane) - 1.  Tiles of a long point
// have one segment: every lane gets pt0.
__device__ __forceinline__ void finish_slot(Slot& s, int lane, int pt0) {
  const uint32_t sg = s.seg;
  s.first = sg & 0xff;
  s.last = (sg >> 8) & 0xff;
  s.valid = (sg >> 16) & 1;
  const unsigned long long heads = __ballot(s.valid && lane == s.first);
  const int rank = __popcll(heads & ((2ull << lane) - 1ull)) - 1;
  s.pt = pt0 + rank;
  s.acc = int(uint32_t(s.cam) >> kSlotCamBits);   // the index word: camera | accumulator row << kSlotCamBits (0 above the camera when every camera has its LDS row)
  s.cam &= (1 << kSlotCamBits) - 1;
  s.nocam = s.cam == kSlotNoCamera;
  if (s.nocam) s.cam = 0;
  if (!s.valid) { s.cam = 0; s.pt = 0; s.acc = kSlotSpill; }
}

// Loads one slot.  Normally from the packed tiles; on the FIRST pass over a step's Jacobian
// (A.src_values != nullptr and may_gather) the 24 doubles are gathered from the caller's
// layout through slot_epos / slot_fpos and the tile is written on the way, which fuses the
// re-layout (bal_pack_kernel) into the first kernel that needs the data anyway.
// CAN_GATHER is a compile-time property of the mode (only kInit / kCgnrInit are ever a step's
// first pass): the streaming kernels do not carry the gather code or its registers.
// F32: the tiles hold the Jacobian rounded to fp32 ([tile][6][64] float4, 96 B per observation instead
// of 192); all arithmetic stays fp64.  Not a parity mode (SURVEY.md §7 item 6): accuracy is reported.
// the 2 kPairs doubles of a slot, in tile order -> its fields
__device__ __forceinline__ void unpack_values(const double (&v)[2 * kPairs], Slot& s) {
#pragma unroll
  for (int i = 0; i < NR * NE; ++i) s.e[i] = v[i];
#pragma unroll
  for (int i = 0; i < NR * NF; ++i) s.f[i] = v[NR * NE + i];
#pragma unroll
  for (int i = 0; i < NR * NSX; ++i) s.h[i] = NS > 0 ? v[(NR * NE + NR * NF + i) % (2 * kPairs)] : 0.0;
}
__device__ __forceinline__ void zero_b(Slot& s) {
#pragma unroll
  for (int r = 0; r < NR; ++r) s.b[r] = 0.0;
}
// the slot's residuals from the residual tiles b[tile][kBPairs][64] (issued with the slot's other loads)
__device__ __forceinline__ void load_b(const BalArgs& A, int64_t tile, int lane, Slot& s) {
  const double2* q = A.b + tile * (kBPairs * kTile) + lane;
  double2 bb[kBPairs];
#pragma unroll
  for (int j = 0; j < kBPairs; ++j) bb[j] = stream_load<2>(q + j * kTile);
#pragma unroll
  for (int r = 0; r < NR; ++r) s.b[r] = (r & 1) ? bb[r / 2].y : bb[r / 2].x;
}
__device__ __forceinline__ void store_b(double2* b_out, int64_t tile, int lane, const double (&b)[NR]) {
  double2* q = b_out + tile * (kBPairs * kTile) + lane;
#pragma unroll
  for (int j = 0; j < kBPairs; ++j) tile_store(q + j * kTile, make_double2(b[2 * j], 2 * j + 1 < NR ? b[(2 * j + 1) % NR] : 0.0));
}
__device__ __forceinline__ void unpack_pairs(const double2 (&p)[kPairs], Slot& s) {
  double v[2 * kPairs];
#pragma unroll
  for (int j = 0; j < kPairs; ++j) { v[2 * j] = p[j].x; v[2 * j + 1] = p[j].y; }
  unpack_values(v, s);
}
// The 2 kPairs doubles of a slot gathered from the caller's layout: the E cell, the camera cell (zeros for a row without one: a locked
// camera) and — shapes with a strip — the row's shared cells, each a row-major NR x w cell that lands at its strip offset.
__device__ __forceinline__ void gather_values(const BalArgs& A, int64_t sl, int ep, double (&v)[2 * kPairs], int fp) {
#pragma unroll
  for (int i = 0; i < 2 * kPairs; ++i) v[i] = 0.0;
  if (ep < 0) return;
  const double* e = A.src_values + ep;
#pragma unroll
  for (int i = 0; i < NR * NE; ++i) v[i] = stream_load<3>(e + i);
  if (fp >= 0) {
    const double* f = A.src_values + fp;
#pragma unroll
    for (int i = 0; i < NR * NF; ++i) v[NR * NE + i] = stream_load<3>(f + i);
  }
  if constexpr (NS > 0) {
#pragma unroll
    for (int q = 0; q < kMaxSharedCellsPerRow; ++q) {
      if (!A.slot_hpos[q]) continue;
      const int hp = A.slot_hpos[q][sl];
      if (hp < 0) continue;
      const int desc = A.slot_hdesc[q][sl], off = desc & 0xff, w = desc >> 8;
      const double* c = A.src_values + hp;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        if (j >= off && j < off + w) {
#pragma unroll
          for (int r = 0; r < NR; ++r) v[(NR * NE + NR * NF + r * NS + j) % (2 * kPairs)] = stream_load<3>(c + r * w + (j - off));
        }
      }
    }
  }
}

// The index words of a slot, loaded ONE TILE AHEAD by the unpipelined kernels' tile loop (bal_fused_kernel, round 6): everything a
// tile's value loads are addressed through.  Without it a tile is a chain of three or four dependent round trips (tile words -> position
// words -> values; index words -> camera part of x, point inverse), which is what a wave's handful of tiles costs on the small shapes
// and on one rank's eighth of a large one.
struct SlotPre { int ep, fp, bp, cam; uint32_t seg; int pt0; int64_t zbase; };
template <bool CAN_GATHER>
__device__ __forceinline__ void issue_pre(const BalArgs& A, int64_t tile, int lane, SlotPre& q) {
  const int64_t sl = tile * kTile + lane;
  q.ep = q.fp = q.bp = 0;
  if (CAN_GATHER && A.src_values) {
    q.ep = A.slot_epos[sl];
    q.fp = A.slot_fpos[sl];
    if (A.src_b) q.bp = A.slot_bpos[sl];
  }
  q.cam = A.slot_cam[sl];
  q.seg = A.slot_seg[sl];
  q.pt0 = A.tile_pt0[tile];
  q.zbase = A.tile_zbase ? A.tile_zbase[tile] : 0;
}

// The VALUES of a slot gathered from the caller's layout one tile ahead (a step's first pass: kInit, kCgnrInit, ...), through the index
// words that were asked for a tile before that: the tile loop of bal_fused_kernel then has the next tile's twenty-six gathers in flight
// while it sums, inverts and stores this one.  Only issues loads (load_slot consumes them).
struct ValPre { double v[2 * kPairs]; double b[NR]; };
__device__ __forceinline__ void issue_values(const BalArgs& A, int64_t tile, int lane, const SlotPre& q, ValPre& o) {
  const int64_t sl = tile * kTile + lane;
  gather_values(A, sl, q.ep, o.v, q.fp);
#pragma unroll
  for (int r = 0; r < NR; ++r) o.b[r] = 0.0;
  if (q.ep >= 0 && A.src_b) {
#pragma unroll
    for (int r = 0; r < NR; ++r) o.b[r] = stream_load<3>(A.src_b + q.bp + r);
  }
}

template <bool CAN_GATHER, bool F32>
__device__ __forceinline__ void load_slot(const BalArgs& A, int64_t tile, int lane, Slot& s, bool want_b,
                                          bool may_gather = true, const SlotPre* pre = nullptr, const ValPre* vp = nullptr, bool have_v = false) {
  const int64_t sl = tile * kTile + lane;
  s.slot = sl;
  s.zbase = pre ? pre->zbase : (A.tile_zbase ? A.tile_zbase[tile] : 0);
  zero_b(s);
  if (CAN_GATHER && A.src_values && may_gather) {
    const int ep = pre ? pre->ep : A.slot_epos[sl];
    double v[2 * kPairs];
    if (have_v) {   // (asked for a tile ago: issue_values.  have_v is wave-uniform and false wherever vp is null — no test of the pointer: a private
                    // object's address compared with null is not a constant for the compiler, and the object would live in scratch)
#pragma unroll
      for (int i = 0; i < 2 * kPairs; ++i) v[i] = vp->v[i];
#pragma unroll
      for (int r = 0; r < NR; ++r) s.b[r] = vp->b[r];
    } else {
      gather_values(A, sl, ep, v, pre ? pre->fp : (ep >= 0 ? A.slot_fpos[sl] : -1));
      if (ep >= 0 && A.src_b) {
        const int bp = pre ? pre->bp : A.slot_bpos[sl];
#pragma unroll
        for (int r = 0; r < NR; ++r) s.b[r] = stream_load<3>(A.src_b + bp + r);
      }
    }
    if constexpr (F32) {
      static_assert(!F32 || kHasF32, "fp32 tiles: BAL shape only");
      float4* o = A.Jf_out + tile * (6 * kTile) + lane;
#pragma unroll
      for (int q = 0; q < 6; ++q) tile_store(o + q * kTile, make_float4(float(v[4 * q]), float(v[4 * q + 1]), float(v[4 * q + 2]), float(v[4 * q + 3])), (A.flags & 4) != 0);
#pragma unroll
      for (int i = 0; i < 2 * kPairs; ++i) v[i] = double(float(v[i]));  // this pass computes with what later passes will read
    } else {
      double2* o = A.J_out + tile * kTilePitch + lane;
#pragma unroll
      for (int j = 0; j < kPairs; ++j) tile_store(o + j * kTile, make_double2(v[2 * j], v[2 * j + 1]), (A.flags & 4) != 0);
    }
    if (A.src_b) store_b(A.b_out, tile, lane, s.b);
    unpack_values(v, s);
  } else if constexpr (F32) {
    static_assert(!F32 || kHasF32, "fp32 tiles: BAL shape only");
    const float4* J = A.Jf + tile * (6 * kTile) + lane;
    float4 p[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) p[q] = stream_load<2>(J + q * kTile);
    if (want_b && A.have_b) load_b(A, tile, lane, s);
    double v[2 * kPairs];
#pragma unroll
    for (int q = 0; q < 6; ++q) { v[4 * q] = p[q].x; v[4 * q + 1] = p[q].y; v[4 * q + 2] = p[q].z; v[4 * q + 3] = p[q].w; }
    unpack_values(v, s);
  } else {
    const double2* J = A.J + tile * kTilePitch + lane;
    double2 p[kPairs];
#pragma unroll
    for (int j = 0; j < kPairs; ++j) p[j] = stream_load<2>(J + j * kTile);
    if (want_b && A.have_b) load_b(A, tile, lane, s);
    unpack_pairs(p, s);
  }
  s.cam = pre ? pre->cam : A.slot_cam[sl];
  s.seg = pre ? pre->seg : A.slot_seg[sl];
  finish_slot(s, lane, pre ? pre->pt0 : A.tile_pt0[tile]);
}

// The software-pipelined streaming kernel splits a slot load in three, each of which only ISSUES
// loads and consumes nothing: the index words (SlotIdx), the 12 pairs of a packed fp64 tile
// (issue_pairs), and what is addressed THROUGH the index words (issue_aux, further down).
struct SlotIdx { int cam; uint32_t seg; };
__device__ __forceinline__ void issue_idx(const BalArgs& A, int64_t tile, int lane, SlotIdx& i) {
  const int64_t sl = tile * kTile + lane;
  i.cam = stream_load<4>(A.slot_cam + sl);
  i.seg = stream_load<4>(A.slot_seg + sl);
}
// NT: the tile stream is larger than the Infinity Cache (non-temporal loads, see stream_load); a problem whose tiles fit there — and in
// the L2s, whose workgroup -> tile mapping is the same in every pass — is better off with plain loads: the next pass finds them on die
// (Ladybug shape: S.x 49 -> 41 us, Dubrovnik 13.0 -> 11.7; profiles/r03n_small_shapes_nt_loads_ab.txt).
// F32 (round 5): the fp32 tiles ([tile][6][64] float4) through the same pipeline — the six loads land in Slot::raw and are widened to the
// fp64 fields by widen_slot() at the head of the stage that computes (a conversion consumes the loaded value: it must not sit in the
// stage that issues).  The ping-pong sets then carry 24 registers of raw values instead of 48.
template <bool NT = true, bool F32 = false>
__device__ __forceinline__ void issue_pairs(const BalArgs& A, int64_t tile, int lane, Slot& s) {
  s.slot = tile * kTile + lane;
  s.zbase = A.tile_zbase ? A.tile_zbase[tile] : 0;
  zero_b(s);
  if constexpr (F32) {
    static_assert(!F32 || kHasF32, "fp32 tiles: BAL shape only");
    const float4* J = A.Jf + tile * (6 * kTile) + lane;
#pragma unroll
    for (int q = 0; q < 6; ++q) s.raw[q] = NT ? stream_load<1>(J + q * kTile) : J[q * kTile];
  } else {
    const double2* J = A.J + tile * kTilePitch + lane;
    double2 p[kPairs];
#pragma unroll
    for (int j = 0; j < kPairs; ++j) p[j] = NT ? stream_load<1>(J + j * kTile) : J[j * kTile];
    unpack_pairs(p, s);
  }
}
template <bool F32>
__device__ __forceinline__ void widen_slot(Slot& s) {
  if constexpr (F32) {
    double v[2 * kPairs];
#pragma unroll
    for (int q = 0; q < 6; ++q) { v[(4 * q) % (2 * kPairs)] = s.raw[q].x; v[(4 * q + 1) % (2 * kPairs)] = s.raw[q].y; v[(4 * q + 2) % (2 * kPairs)] = s.raw[q].z; v[(4 * q + 3) % (2 * kPairs)] = s.raw[q].w; }
    unpack_values(v, s);
  }
}

__device__ __forceinline__ int pt_off(const BalArgs& A, int p) { return A.pt_pos ? A.pt_pos[p] : NE * p; }
__device__ __forceinline__ int cam_off(const BalArgs& A, int c) { return A.cam_pos ? A.cam_pos[c] : A.cam_base + NF * c; }

// the packed inverse of a point's block: kTriE doubles in kEteiPitch / 2 records of 16 bytes
__device__ __forceinline__ void load_ete_inverse(const BalArgs& A, int pt, double (&ei)[kTriE]) {
  const double2* q = reinterpret_cast<const double2*>(A.etei + int64_t(pt) * kEteiPitch);
  double2 r[kEteiPitch / 2];
#pragma unroll
  for (int j = 0; j < kEteiPitch / 2; ++j) r[j] = stream_load<4>(q + j);
#pragma unroll
  for (int i = 0; i < kTriE; ++i) ei[i] = (i & 1) ? r[i / 2].y : r[i / 2].x;
}
// v = M u, M symmetric NE x NE in packed upper-triangle order
__device__ __forceinline__ void sym_mul(const double (&m)[kTriE], const double (&u)[NE], double (&v)[NE]) {
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) t += m[i <= j ? tri_e(i, j) : tri_e(j, i)] * u[j];
    v[i] = t;
  }
}
// w = E^T z (the slot's NR x NE point cell, row-major) and r = E v
__device__ __forceinline__ void et_times(const double (&e)[NR * NE], const double (&z)[NR], double (&w)[NE]) {
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) t += e[r * NE + j] * z[r];
    w[j] = t;
  }
}
__device__ __forceinline__ void e_times(const double (&e)[NR * NE], const double (&v)[NE], double (&out)[NR]) {
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) t += e[r * NE + j] * v[j];
    out[r] = t;
  }
}

// The NF camera scalars of a slot (contiguous; L2-resident for the camera counts that fit LDS).
// The scalars are fetched as 16-byte pairs — global memory needs no 16-byte alignment (camera c of a 9-wide shape starts at 72 c bytes),
// the vector type says so — NF / 2 + NF % 2 gather instructions per lane instead of NF.  Measured NEUTRAL on the Venice shape (round 5,
// profiles/r05h_*: S.x 0.691 of peak either way): the hypothesis was that a lane's gather costs the CU's address pipeline a clock per lane
// and instruction whatever its width (576 of ~970 such clocks per S.x tile next to 192 for the tile stream) — that pipeline is not what
// S.x waits for.  Kept because it is fewer instructions; CERES_HIP_AB_XC_WIDE=0 in an A/B build restores the scalar loads.
#ifndef CERES_HIP_AB_XC_WIDE
#define CERES_HIP_AB_XC_WIDE 1
#endif
typedef double xc_pair __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void load_camera_scalars(const double* __restrict__ p, double (&xc)[NF]) {
#if CERES_HIP_AB_XC_WIDE
#pragma unroll
  for (int k = 0; k + 1 < NF; k += 2) { const xc_pair v = *reinterpret_cast<const xc_pair*>(p + k); xc[k] = v.x; xc[k + 1] = v.y; }
  if constexpr (NF & 1) xc[NF - 1] = p[NF - 1];
#else
#pragma unroll
  for (int k = 0; k < NF; ++k) xc[k] = p[k];
#endif
}
// Back-substitution and the model-cost pass scatter nothing, so their LDS is free: the whole camera part of x sits there
// (BalArgs::x_lds_scalars, staged by bal_fused_kernel) and a slot reads its camera's NF scalars from it.  Gathered from memory these
// reads cost the back-substitution 33 of its 226 us on the Venice shape — every workgroup asking the L2 for the same few hundred
// popular lines (profiles/r05p_*).  (All `extern __shared__` arrays of a kernel name the same dynamic LDS.)
extern __shared__ double lds_x_all[];
#if CERES_HIP_AB_ABLATE & 128   // (timing only: the unpipelined kernels' camera-part gathers all read camera 0's line)
__device__ __forceinline__ void load_xc(const BalArgs& A, int cam, double (&xc)[NF]) { load_camera_scalars(A.x_f + cam_off(A, 0), xc); }
#else
__device__ __forceinline__ void load_xc(const BalArgs& A, int cam, double (&xc)[NF]) {
  if (A.x_lds_scalars > 0) {   // (launch-uniform)
    const double* p = lds_x_all + NF * cam;
#pragma unroll
    for (int k = 0; k < NF; ++k) xc[k] = p[k];
  } else {
    load_camera_scalars(A.x_f + cam_off(A, cam), xc);
  }
}
#endif

// t = F * xc (+ H * xs: the strip's part of x, wave-uniform, in the context)
__device__ __forceinline__ void f_times(const Slot& s, const Ctx& c, const double (&xc)[NF], double (&t)[NR]) {
#pragma unroll
  for (int r = 0; r < NR; ++r) t[r] = 0.0;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
#pragma unroll
    for (int r = 0; r < NR; ++r) t[r] += s.f[r * NF + k] * xc[k];
  }
  if constexpr (NS > 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
#pragma unroll
      for (int r = 0; r < NR; ++r) t[r] += s.h[r * NS + k] * c.xs[k];
    }
  }
}
// column k of the camera cell times z: (F^T z)_k
__device__ __forceinline__ double ft_entry(const Slot& s, int k, const double (&z)[NR]) {
  double t = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) t += s.f[r * NF + k] * z[r];
  return t;
}
// The strip's share of J^T z: this lane's running sums (Ctx), no atomics — reduced over the workgroup when the kernel ends.
__device__ __forceinline__ void shared_ht(const Slot& s, Ctx& c, const double (&z)[NR]) {
  if constexpr (NS > 0) {
    if (!s.valid) return;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) t += s.h[r * NS + k] * z[r];
      c.hs[k] += t;
    }
  }
}
// Camera-space contribution F^T z of one observation.  LDS: NF ds_add_f64 into the workgroup's accumulator, one row per camera.
// Otherwise (more cameras than LDS rows) the HYBRID form: a slot whose camera has a row in THIS workgroup's accumulator (one of
// the popular cameras every workgroup holds, or a camera of the workgroup's own window: Slot::acc, plan.cc) adds into it the same
// way; the others are SPILLED — the NF products are stored in a ring, the spilled slots of a tile back to back from the tile's
// ring row s.zbase on, and bal_camera_chunk_kernel sums them camera by camera in a second pass (global fp64 atomics on a few
// thousand hot addresses are an order of magnitude slower).  A lane storing its own 8 NF-byte row would issue NF 8-byte stores
// at that stride, and it is the L2's request rate, not its bytes, that such stores exhaust (the per-slot output cost as much
// as reading the tile stream): the wave packs the rows through a private LDS strip (behind the accumulator rows) and
// stores one contiguous range.  Without a hybrid plan (CGNR on caller-ordered vectors, chunked rings) every slot spills.
template <bool LDS>
__device__ __forceinline__ void scatter_ft(const BalArgs& A, const Slot& s, Ctx& c, const double (&z)[NR]) {
  double* const acc = c.lds;
  shared_ht(s, c, z);
  if constexpr (LDS) {
    if (!s.valid) return;
    const int base = NF * s.cam;
#if CERES_HIP_AB_ABLATE & 1
    double keep = 0;
#pragma unroll
    for (int k = 0; k < NF; ++k) keep += ft_entry(s, k, z);
    if (keep == 1.2345e-300) acc[base] = keep;   // (keeps the products alive, never stores)
#else
#pragma unroll
    for (int k = 0; k < NF; ++k) atomicAdd(&acc[base + k], ft_entry(s, k, z));  // ds_add_f64
#endif
  } else {
    const bool local = s.valid && s.acc != kSlotSpill;
    if (local) {
      const int base = NF * s.acc;
#pragma unroll
      for (int k = 0; k < NF; ++k) atomicAdd(&acc[base + k], ft_entry(s, k, z));
    }
    const bool spill = s.valid && !local && !s.nocam;
    // (nothing to store for a tile without spilled slots: that includes the tiles of long points the pipelined kernel runs through
    // here with every lane masked — their real values are written by whichever wave owns the point's head tile)
    const unsigned long long mask = __ballot(spill);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int rank = __popcll(mask & ((1ull << lane) - 1ull)), nn = NF * __popcll(mask);
    double* st = acc + NF * A.hyb_rows + (threadIdx.x >> 6) * (kTile * NF);  // this wave's strip
    if (spill) {
#pragma unroll
      for (int k = 0; k < NF; ++k) st[rank * NF + k] = ft_entry(s, k, z);
    }
    __builtin_amdgcn_wave_barrier();
    double* w = A.zbuf + int64_t(NF) * s.zbase;
#pragma unroll
    for (int j = 0; j < NF; ++j) if (kTile * j + lane < nn) w[kTile * j + lane] = st[kTile * j + lane];
    __builtin_amdgcn_wave_barrier();
  }
}

// End of a scattering kernel (LDS accumulators): every wave adds its lanes' strip sums into the accumulator entries behind the cameras'.
__device__ __forceinline__ void flush_shared_sums(const BalArgs& A, Ctx& c) {
  if constexpr (NS > 0) {
    double v[NSX];
#pragma unroll
    for (int k = 0; k < NSX; ++k) v[k] = c.hs[k];
    wave_allreduce<NSX>(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) atomicAdd(&c.lds[A.n_acc - NS + k], v[k]);
    }
  }
}

// The same with the accumulators outside LDS (hybrid / spilled sums): the strip's entries live behind the cameras' in the global sums
// the camera-major pass adds into (A.strip_sums, zeroed by the caller); one atomic per wave and strip scalar.
__device__ __forceinline__ void flush_shared_sums_global(const BalArgs& A, Ctx& c) {
  if constexpr (NS > 0) {
    if (!A.strip_sums) return;
    double v[NSX];
#pragma unroll
    for (int k = 0; k < NSX; ++k) v[k] = c.hs[k];
    wave_allreduce<NSX>(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) unsafeAtomicAdd(A.strip_sums + k, v[k]);
    }
  }
}

// Camera-column squared norms: sum over the observation of F[:,k]^2 (LDS accumulators only); the strip's columns likewise.
__device__ __forceinline__ void scatter_f_squares(const Slot& s, Ctx& c) {
  if (!s.valid) return;
  const int base = NF * s.cam;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) t += s.f[r * NF + k] * s.f[r * NF + k];
    atomicAdd(&c.lds[base + k], t);
  }
  if constexpr (NS > 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) t += s.h[r * NS + k] * s.h[r * NS + k];
      c.hs[k] += t;
    }
  }
}

// A/B builds only (tools/build_variant.sh, loaded through CERES_HIP_LIBRARY): how the cooperative JtJx path stores y_e.
// 0 = plain stores (the product), 1 = non-temporal stores, 2 = no stores at all (timing ablation: results are wrong).
#ifndef CERES_HIP_AB_YE_STORE
#define CERES_HIP_AB_YE_STORE 0
#endif
// 3 (timing ablation, needs CERES_HIP_AB_TILE_ROWS=13): the output goes into the 1 KiB gap right behind the tile it was computed from
// (`alt`), i.e. into the DRAM neighbourhood the wave is reading anyway, instead of the point-space vector.
__device__ __forceinline__ void store_ye(double* p, double v, double* alt = nullptr) {
#if CERES_HIP_AB_YE_STORE == 1
  __builtin_nontemporal_store(v, p);
#elif CERES_HIP_AB_YE_STORE == 2
  (void)p; (void)v;
#elif CERES_HIP_AB_YE_STORE == 3
  (void)p; *alt = v;
#elif CERES_HIP_AB_YE_STORE == 4   // sc1: system-scope (write-through) store
  (void)alt; asm volatile("global_store_dwordx2 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
#elif CERES_HIP_AB_YE_STORE == 5   // sc0 sc1
  (void)alt; asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
#elif CERES_HIP_AB_YE_STORE == 6   // sc0 sc1 nt
  (void)alt; asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1 nt" : : "v"(p), "v"(v) : "memory");
#else
  (void)alt;
  *p = v;
#endif
}
// A/B builds only: non-temporal loads for the point-space x / D of the pipelined JtJx (each scalar is read by exactly one tile)
#ifndef CERES_HIP_AB_XE_NT
#define CERES_HIP_AB_XE_NT 0
#endif
__device__ __forceinline__ double load_xe(const double* p) {
#if CERES_HIP_AB_XE_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
// XCD-aware tile walk: workgroups are dealt round-robin to the 8 XCDs, each with its own L2, and neighbouring tiles share lines of
// everything indexed by point (x_e, D_e, y_e, (E^T E)^-1: a tile's point range starts wherever the previous one ended).  Workgroup b
// therefore walks the tile groups of "logical workgroup" (b % 8) * (grid / 8) + b / 8: XCD x gets the logical workgroups
// [x grid / 8, (x + 1) grid / 8), whose tiles are neighbours at every step of the grid-strided loop, so a shared line is fetched
// into ONE L2 instead of two.  Measured on the Venice shape (profiles/r03a_ab_*): S.x 0.2010 -> 0.1933 ms, JtJx 0.2374 -> 0.2334 ms.
// CERES_HIP_AB_XCD_GROUP=0 in an A/B build restores the identity mapping.
#ifndef CERES_HIP_AB_XCD_GROUP
#define CERES_HIP_AB_XCD_GROUP 1
#endif
__device__ __forceinline__ int64_t logical_workgroup() {
#if CERES_HIP_AB_XCD_GROUP
  return (gridDim.x % 8 == 0) ? int64_t(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8 : int64_t(blockIdx.x);
#else
  return blockIdx.x;
#endif
}

__device__ __forceinline__ double* ye_alt(const BalArgs& A, const Slot& s) {
#if CERES_HIP_AB_YE_STORE == 3
  static_assert(CERES_HIP_AB_TILE_ROWS == 13, "the gap behind the tile");
  return reinterpret_cast<double*>(const_cast<double2*>(A.J) + (s.slot / kTile) * kTilePitch + kPairs * kTile);
#else
  (void)A; (void)s;
  return nullptr;
#endif
}

enum Mode { kSx = 0, kJtJx = 1, kJtb = 2, kInit = 3, kEte = 4, kBackSub = 5, kCgnrInit = 6, kColNorm = 7, kJx = 8, kSpseZ = 9, kShBlocks = 10 };

template <int MODE>
constexpr bool kWantsB = (MODE == kJtb || MODE == kInit || MODE == kBackSub || MODE == kCgnrInit || MODE == kJx);
template <int MODE>
constexpr bool kCanGather = (MODE == kInit || MODE == kCgnrInit || MODE == kColNorm || MODE == kJtb);

// E^T E (packed symmetric) of one slot.
__device__ __forceinline__ void ete_of(const Slot& s, double (&a)[kTriE]) {
#pragma unroll
  for (int i = 0; i < NE; ++i) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      if (j < i) continue;
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) t += s.e[r * NE + i] * s.e[r * NE + j];
      a[tri_e(i, j)] = t;
    }
  }
}
// the squared column norms of the slot's point cell
__device__ __forceinline__ void e_col_squares(const Slot& s, double (&w)[NE]) {
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) t += s.e[r * NE + j] * s.e[r * NE + j];
    w[j] = t;
  }
}

// Regularisation of the point block.  Either D is given (A.D_e), or — fused LM diagonal,
// A.lm_radius > 0 — it is formed right here from the block's own diagonal, which IS
// diag(J^T J) over the point's columns: d = clamp(a_jj, min, max), D^2 = d / radius
// (LevenbergMarquardtStrategy::ComputeStep, I/levenberg_marquardt_strategy.cc:84-96); `writer`
// lanes record d (for a later reuse_diagonal step) and D.
// pt / po: the point and its offset in x_e / y_e; the caller's D (and the LM diagonal) may live at another offset (A.d_pos: CGNR on
// internally numbered points), and then the writer also leaves D in the internal order (A.D_int_out) for the operator.
__device__ __forceinline__ void add_e_diagonal(const BalArgs& A, int pt, int po, double (&a)[kTriE], bool writer) {
  const int pd = A.d_pos ? A.d_pos[pt] : po;
  if (A.lm_radius > 0.0) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const double d = fmin(fmax(a[tri_e(j, j)], A.lm_min), A.lm_max);
      const double q = d / A.lm_radius;
      if (writer) {
        const double sq = sqrt(q);
        A.lm_diag_e[pd + j] = d;
        A.lm_D_e[pd + j] = sq;
        if (A.D_int_out) A.D_int_out[po + j] = sq;
      }
      a[tri_e(j, j)] += q;
    }
  } else if (A.D_e) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const double d = A.D_e[pd + j];
      if (writer && A.D_int_out) A.D_int_out[po + j] = d;
      a[tri_e(j, j)] += d * d;
    }
  }
}
// the identity (padding lanes invert it)
__device__ __forceinline__ void set_identity_e(double (&a)[kTriE]) {
#pragma unroll
  for (int i = 0; i < NE; ++i) {
#pragma unroll
    for (int j = 0; j < NE; ++j) if (j >= i) a[tri_e(i, j)] = i == j ? 1.0 : 0.0;
  }
}

__device__ __forceinline__ void store_ete_inverse(const BalArgs& A, int pt, const double (&ei)[kTriE]) {
  if (A.etei) {
    double2* q = reinterpret_cast<double2*>(A.etei + int64_t(pt) * kEteiPitch);
#pragma unroll
    for (int j = 0; j < kEteiPitch / 2; ++j) tile_store<2>(q + j, make_double2(ei[2 * j], 2 * j + 1 < kTriE ? ei[(2 * j + 1) % kTriE] : 0.0));
  }
  if (A.point_blocks) {  // dense NE x NE in the all-blocks diagonal store (CGNR JACOBI)
    double* o = A.point_blocks + (A.pt_diag_off ? A.pt_diag_off[pt] : int64_t(NE * NE) * pt);
#pragma unroll
    for (int i = 0; i < NE; ++i) {
#pragma unroll
      for (int j = 0; j < NE; ++j) o[NE * i + j] = ei[i <= j ? tri_e(i, j) : tri_e(j, i)];
    }
  }
}

// One slot's share of its point's set-up sums: E^T E (packed), then E^T b; zeros for a padding slot.
__device__ __forceinline__ void slot_point_sums(const Slot& s, double (&r)[kNX]) {
  double a[kTriE], g[NE];
  ete_of(s, a);
  et_times(s.e, s.b, g);
#pragma unroll
  for (int i = 0; i < kTriE; ++i) r[i] = s.valid ? a[i] : 0.0;
#pragma unroll
  for (int j = 0; j < NE; ++j) r[kTriE + j] = s.valid ? g[j] : 0.0;
}
// the point part of the solution (back-substitution): y_e = v, or -v and the finite check when the LM step is wanted
__device__ __forceinline__ void store_point_solution(const BalArgs& A, int po, const double (&v)[NE]) {
  const double sg = A.negate_out ? -1.0 : 1.0;  // the LM step is -x
  double t = 0.0;
#pragma unroll
  for (int j = 0; j < NE; ++j) { A.y_e[po + j] = sg * v[j]; t += v[j]; }
  if (A.negate_out && !isfinite(t)) atomicAdd(A.nonfinite, 1);
}

// Point tail (design/20_point_tail.md): a point's finished sum E^T F x of an S.x pass, kept for the tail (A.u_out != nullptr), and its
// E^T b from kInit (A.etb_out); both indexed like y_e.  Called by the ONE lane that holds the point's sum.  Only the instantiations with
// every camera's accumulator in LDS capture (the handles that take the point tail run no other): the others' code is what it was.
__device__ __forceinline__ void store_point_capture(double* out, int po, const double* v) {
#pragma unroll
  for (int j = 0; j < NE; ++j) out[po + j] = v[j];
}

// sum over the slot's rows of m_r (b_r + half m_r): the observation's share of a model cost change
__device__ __forceinline__ double cost_terms(const double (&m)[NR], const double (&b)[NR], double half) {
  double t = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) t += m[r] * (b[r] + half * m[r]);
  return t;
}

// Everything after the per-point quantities are known, for kInit.
template <bool LDS>
__device__ __forceinline__ void init_apply(const BalArgs& A, const Slot& s, int64_t sl,
                                           const double (&ei)[kTriE], const double (&g)[NE], Ctx& acc) {
  double h[NE], eh[NR], w[NR];
  sym_mul(ei, g, h);
  e_times(s.e, h, eh);
#pragma unroll
  for (int r = 0; r < NR; ++r) w[r] = s.b[r] - eh[r];
  if (A.have_b) scatter_ft<LDS>(A, s, acc, w);
  if (A.Mo && s.valid) {  // M = I - E Ei E^T, symmetric NR x NR: the packed upper triangle, row by row
    double q[NR][NE];   // q_r = Ei e_r
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double er[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) er[j] = s.e[r * NE + j];
      sym_mul(ei, er, q[r]);
    }
    double m[kMoPitch];
#pragma unroll
    for (int i = 0; i < kMoPitch; ++i) m[i] = 0.0;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
#pragma unroll
      for (int b = 0; b < NR; ++b) {
        if (b < a) continue;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < NE; ++j) d += s.e[a * NE + j] * q[b][j];
        m[tri_r(a, b)] = (a == b ? 1.0 : 0.0) - d;
      }
    }
    if constexpr (NR == 2) m[3] = m[1];   // [m00 m01 m11 m01], 32 B: m01 again for bal_camera_items_mfma_kernel
    double2* mo = reinterpret_cast<double2*>(A.Mo + kMoPitch * (A.mo_index ? int64_t(A.mo_index[sl]) : sl));
#pragma unroll
    for (int i = 0; i < kMoPitch / 2; ++i) tile_store<2>(mo + i, make_double2(m[2 * i], m[2 * i + 1]));
  }
}

// What a streaming mode (kSx, kSpseZ, kJtJx) needs from global memory besides the slot itself.
struct StreamAux {
  double xc[NF];            // the slot's camera part of x
  double ei[kTriE];        // kSx / kSpseZ: (E^T E)^-1 of the slot's point
  double xa, xb, da, db;   // kJtJx, cooperative: scalars `lane` and `64 + lane` of the tile's point range of x, D
  double xp[NE], dd[NE];   // kJtJx, otherwise: the slot's own point part of x, D
  int64_t base;
  bool coop;
};

// Issues the loads of `aux`; consumes only the slot's index words (s.cam, s.pt).
template <int MODE>
__device__ __forceinline__ void load_aux(const BalArgs& A, const Slot& s, int lane, int npts, StreamAux& x) {
  load_xc(A, s.cam, x.xc);
  x.xa = x.xb = x.da = x.db = 0.0;
  x.base = 0;
  x.coop = false;
#pragma unroll
  for (int j = 0; j < NE; ++j) { x.xp[j] = 0.0; x.dd[j] = 0.0; }
  if constexpr (MODE == kSx || MODE == kSpseZ) {
    load_ete_inverse(A, s.pt, x.ei);
  } else if constexpr (MODE == kJtJx) {
    // Point-space x / D / y of a tile are ONE contiguous range when the layout is
    // points-then-cameras (pt_pos == nullptr): [3 p0, 3 p0 + 3 npts).  Then lane L loads and
    // stores scalars L (and 64 + L) of that range — dense 8-byte-per-lane accesses — and the
    // per-observation copies travel by wavefront shuffle, instead of three strided loads per
    // lane and three partial-wave scattered stores per point.  (3-wide points only: the plan's tile words count in threes.)
    x.coop = CERES_HIP_PIPELINED && A.pt_pos == nullptr && !(A.flags & 1);
    if (x.coop) {
      const int n3 = 3 * npts;
      x.base = 3 * int64_t(__builtin_amdgcn_readfirstlane(s.pt));  // lane 0 of a normal tile is valid
      if (lane < n3) { x.xa = A.x_e[x.base + lane]; if (A.D_e) x.da = A.D_e[x.base + lane]; }
      if (n3 > 64 && lane + 64 < n3) { x.xb = A.x_e[x.base + 64 + lane]; if (A.D_e) x.db = A.D_e[x.base + 64 + lane]; }
    } else {
      const int po = pt_off(A, s.pt);
#pragma unroll
      for (int j = 0; j < NE; ++j) { x.xp[j] = A.x_e[po + j]; if (A.D_e) x.dd[j] = A.D_e[po + j]; }
    }
  }
}

// The arithmetic of a streaming mode on one normal tile; issues no global loads.
// CAP: how a kSx pass keeps the points' sums — 0: where A.u_out is set (the unpipelined kernels), 1: always, with dense stores (the
// capturing instantiation of the pipelined kernel), 2: never (its other instantiation: no capture code at all)
template <int MODE, bool LDS, int CAP = 0>
__device__ __forceinline__ void compute_stream(const BalArgs& A, const Slot& s, int lane, int span, int npts,
                                               const StreamAux& x, Ctx& acc, double& dot) {
  if constexpr (MODE == kSx || MODE == kSpseZ) {
    double v[NE];
    double t[NR];
    f_times(s, acc, x.xc, t);
    double u[NE];
    et_times(s.e, t, u);
    if (!s.valid) {
#pragma unroll
      for (int j = 0; j < NE; ++j) u[j] = 0;
    }
#if !(CERES_HIP_AB_ABLATE & 4)
    seg_allreduce<NE>(u, lane, s.first, s.last, span);
#endif
    if constexpr (MODE == kSx && LDS && CAP == 1) {
#if CERES_HIP_PIPELINED
      // The capturing instantiation of the pipelined kernel (launched only with A.u_out set: no store under a launch-uniform branch, the
      // stage's s_waitcnt counts stay static): the tile's points are consecutive ids, their sums one contiguous range of u_out, and
      // lane L stores scalar L (and 64 + L) of it, gathered from the point's last lane — JtJx's cooperative store of y_e.  One or two
      // dense stores per tile.  Measured on the Venice shape (design/20_point_tail.md §20.6): the pass takes 199 - 208 us with them, 160 - 171
      // without; three scattered 8-byte stores per point under a run-time branch took it to 208 - 217 us.
      const int n3 = 3 * npts;
      double* const out = A.u_out + 3 * int64_t(__builtin_amdgcn_readfirstlane(s.pt));
      const int ta = (s.seg >> 17) & 63, tb = (s.seg >> 24) & 63;
      {
        const double v0 = shfl_idx(u[0], ta), v1 = shfl_idx(u[1], ta), v2 = shfl_idx(u[2], ta);
        const int c = lane % 3;
        if ((s.seg >> 23) & 1) out[lane] = c == 0 ? v0 : (c == 1 ? v1 : v2);
      }
      if (n3 > 64) {
        const double v0 = shfl_idx(u[0], tb), v1 = shfl_idx(u[1], tb), v2 = shfl_idx(u[2], tb);
        const int c = (lane + 1) % 3;  // (64 + lane) % 3
        if ((s.seg >> 30) & 1) out[64 + lane] = c == 0 ? v0 : (c == 1 ? v1 : v2);
      }
#endif
    } else if constexpr (MODE == kSx && LDS && CAP == 0) {
      if (A.u_out && s.valid && lane == s.last) store_point_capture(A.u_out, NE * s.pt, u);
    }
    sym_mul(x.ei, u, v);
    // kSx: F^T (F x - E (E^T E)^-1 E^T F x);  kSpseZ: only the second term, F^T E (E^T E)^-1 E^T F x
    // (ImplicitSchurComplement::InversePowerSeriesOperatorRightMultiplyAccumulate, :146-174)
    double ev[NR], z[NR];
    e_times(s.e, v, ev);
#pragma unroll
    for (int r = 0; r < NR; ++r) z[r] = MODE == kSx ? t[r] - ev[r] : ev[r];
    scatter_ft<LDS>(A, s, acc, z);
  } else {
    static_assert(MODE == kJtJx, "streaming modes");
    double xp[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) xp[j] = x.xp[j];
#if CERES_HIP_PIPELINED
    const int n3 = 3 * npts;
    if (x.coop) {
      const int li = s.valid ? 3 * s.pt - int(x.base) : 0;
      if (n3 <= 64) {
#pragma unroll
        for (int j = 0; j < 3; ++j) xp[j] = shfl_idx(x.xa, li + j);
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double va = shfl_idx(x.xa, (li + j) & 63), vb = shfl_idx(x.xb, (li + j) & 63);
          xp[j] = (li + j) < 64 ? va : vb;
        }
      }
    }
#endif
    double z[NR];
    f_times(s, acc, x.xc, z);
    {
      double ex[NR];
      e_times(s.e, xp, ex);
#pragma unroll
      for (int r = 0; r < NR; ++r) z[r] += ex[r];
    }
    scatter_ft<LDS>(A, s, acc, z);
    double w[NE];
    et_times(s.e, z, w);
    if (!s.valid) {
#pragma unroll
      for (int j = 0; j < NE; ++j) w[j] = 0;
    }
    seg_scan<NE>(w, lane, s.first, span);
#if CERES_HIP_PIPELINED
    if (x.coop) {
      // lane L gathers component L % 3 of point L / 3 from that point's last lane and stores scalar L
      const int ta = (s.seg >> 17) & 63, tb = (s.seg >> 24) & 63;
      {
        const double v0 = shfl_idx(w[0], ta), v1 = shfl_idx(w[1], ta), v2 = shfl_idx(w[2], ta);
        const int c = lane % 3;
        const double v = c == 0 ? v0 : (c == 1 ? v1 : v2);
        if ((s.seg >> 23) & 1) { const double yv = v + x.da * x.da * x.xa; store_ye(A.y_e + x.base + lane, yv, ye_alt(A, s) + lane); dot += x.xa * yv; }
      }
      if (n3 > 64) {
        const double v0 = shfl_idx(w[0], tb), v1 = shfl_idx(w[1], tb), v2 = shfl_idx(w[2], tb);
        const int c = (lane + 1) % 3;  // (64 + lane) % 3
        const double v = c == 0 ? v0 : (c == 1 ? v1 : v2);
        if ((s.seg >> 30) & 1) { const double yv = v + x.db * x.db * x.xb; store_ye(A.y_e + x.base + 64 + lane, yv, ye_alt(A, s) + 64 + lane); dot += x.xb * yv; }
      }
    } else
#endif
    if (s.valid && lane == s.last) {
      const int po = pt_off(A, s.pt);
#pragma unroll
      for (int j = 0; j < NE; ++j) { const double yv = w[j] + x.dd[j] * x.dd[j] * xp[j]; A.y_e[po + j] = yv; dot += xp[j] * yv; }
    }
  }
}

// kShBlocks, one normal tile: the strip's own matrix.  Every row adds H^T H; with the point inverses at hand (A.etei: SCHUR_JACOBI) the
// last lane of a point subtracts G^T (E^T E + D^2)^-1 G, G = sum over the point's rows of E^T H (3 x NS) — the rows of a point all hold
// the shared cell, so SchurEliminator's update of this diagonal cell couples them (I/schur_eliminator_impl.h:498-565: every pair of F
// cells of the chunk, the pair (shared, shared) from different rows included).
__device__ __forceinline__ void strip_minus_gtg(const BalArgs& A, int pt, const double (&g)[NE * NSX], Ctx& c) {
  double ei[kTriE];
  load_ete_inverse(A, pt, ei);
  int idx = 0;
#pragma unroll
  for (int a = 0; a < NS; ++a) {
    double u[NE], w[NE];
#pragma unroll
    for (int d = 0; d < NE; ++d) u[d] = g[d * NSX + a];
    sym_mul(ei, u, w);   // column a of (E^T E)^-1 G
#pragma unroll
    for (int b = a; b < NS; ++b) {
      double t = 0.0;
#pragma unroll
      for (int d = 0; d < NE; ++d) t += w[d] * g[d * NSX + b];
      c.tt[idx++] -= t;
    }
  }
}
// E and the strip of a slot, nothing else: kShBlocks does not look at the camera cell (of a <2, 8 | 6, 3> slot it reads 22 of the 34 doubles)
struct SlotEH {
  double e[NR * NE], h[NR * NSX];
  uint32_t seg;
  int pt, first, last;
  bool valid;
};
__device__ __forceinline__ void load_slot_eh(const BalArgs& A, int64_t tile, int lane, SlotEH& s) {
  const double2* J = A.J + tile * kTilePitch + lane;
  double v[2 * kPairs];
#pragma unroll
  for (int i = 0; i < 2 * kPairs; ++i) v[i] = 0.0;
#pragma unroll
  for (int j = 0; j < kPairs; ++j) {   // the pairs that hold E values or strip values, nothing of the camera cell
    const bool need = 2 * j < NR * NE || (NS > 0 && 2 * j + 1 >= NR * (NE + NF) && 2 * j < kVals);
    if (need) { const double2 q = stream_load<2>(J + j * kTile); v[2 * j] = q.x; v[2 * j + 1] = q.y; }
  }
  s.seg = A.slot_seg[tile * kTile + lane];
  s.first = s.seg & 0xff;
  s.last = (s.seg >> 8) & 0xff;
  s.valid = (s.seg >> 16) & 1;
  const unsigned long long heads = __ballot(s.valid && lane == s.first);
  s.pt = A.tile_pt0[tile] + __popcll(heads & ((2ull << lane) - 1ull)) - 1;
#pragma unroll
  for (int i = 0; i < NR * NE; ++i) s.e[i] = v[i];
#pragma unroll
  for (int i = 0; i < NR * NSX; ++i) s.h[i] = NS > 0 ? v[(NR * NE + NR * NF + i) % (2 * kPairs)] : 0.0;
}
// this row's H^T H into c.tt, its E^T H ADDED to g
__device__ __forceinline__ void strip_row_terms(const SlotEH& s, Ctx& c, double (&g)[NE * NSX]) {
  if (!s.valid) return;
  int idx = 0;
#pragma unroll
  for (int a = 0; a < NS; ++a) {
#pragma unroll
    for (int b = a; b < NS; ++b) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) t += s.h[r * NS + a] * s.h[r * NS + b];
      c.tt[idx++] += t;
    }
  }
#pragma unroll
  for (int d = 0; d < NE; ++d) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) t += s.e[r * NE + d] * s.h[r * NS + j];
      g[d * NSX + j] += t;
    }
  }
}
__device__ __forceinline__ void shared_block_sums(const BalArgs& A, int64_t tile, int lane, int span, Ctx& c) {
  if constexpr (NS > 0) {
    SlotEH s;
    load_slot_eh(A, tile, lane, s);
    double g[NE * NSX];
#pragma unroll
    for (int i = 0; i < NE * NSX; ++i) g[i] = 0.0;
    strip_row_terms(s, c, g);
    if (A.etei) {
      seg_scan<NE * NSX>(g, lane, s.first, span);
      if (s.valid && lane == s.last) strip_minus_gtg(A, s.pt, g, c);
    }
  }
}
// a point of more than 64 observations: one wave sums its tiles' E^T H, lane 0 subtracts
__device__ __forceinline__ void shared_block_sums_long(const BalArgs& A, int64_t tile, int nt, int lane, Ctx& c) {
  if constexpr (NS > 0) {
    double gs[NE * NSX];
#pragma unroll
    for (int i = 0; i < NE * NSX; ++i) gs[i] = 0.0;
    int pt = 0;
    for (int t = 0; t < nt; ++t) {
      SlotEH s;
      load_slot_eh(A, tile + t, lane, s);
      if (t == 0) pt = __shfl(s.pt, 0, 64);
      strip_row_terms(s, c, gs);
    }
    if (A.etei) {
      wave_allreduce<NE * NSX>(gs);
      if (lane == 0) strip_minus_gtg(A, pt, gs, c);
    }
  }
}

template <int MODE, bool LDS, bool F32>
__device__ __forceinline__ void process_tile(const BalArgs& A, int64_t tile, int lane, int span, int npts, Ctx& acc,
                                             double& lane_acc, const SlotPre* pre = nullptr, const ValPre* vp = nullptr, bool have_v = false) {
  if constexpr (MODE == kShBlocks) {
    shared_block_sums(A, tile, lane, span, acc);
    return;
  }
  Slot s;
  load_slot<kCanGather<MODE>, F32>(A, tile, lane, s, kWantsB<MODE>, true, pre, vp, have_v);
  const int64_t sl = tile * kTile + lane;
  const int po = pt_off(A, s.pt);
  if constexpr (MODE == kSx || MODE == kSpseZ || MODE == kJtJx) {
    StreamAux x;
    load_aux<MODE>(A, s, lane, npts, x);
    compute_stream<MODE, LDS>(A, s, lane, span, npts, x, acc, lane_acc);
  } else if constexpr (MODE == kJtb) {
    scatter_ft<LDS>(A, s, acc, s.b);
    double w[NE];
    et_times(s.e, s.b, w);
    if (!s.valid) {
#pragma unroll
      for (int j = 0; j < NE; ++j) w[j] = 0;
    }
    seg_scan<NE>(w, lane, s.first, span);
    if (s.valid && lane == s.last) {
#pragma unroll
      for (int j = 0; j < NE; ++j) A.y_e[po + j] = w[j];
    }
  } else if constexpr (MODE == kInit || MODE == kEte) {
    double r[kNX];   // E^T E (packed), then E^T b
    slot_point_sums(s, r);
    if constexpr (MODE == kInit) {
      seg_allreduce<kNX>(r, lane, s.first, s.last, span);
    } else {
      double a6[kTriE];
#pragma unroll
      for (int i = 0; i < kTriE; ++i) a6[i] = r[i];
      seg_allreduce<kTriE>(a6, lane, s.first, s.last, span);
#pragma unroll
      for (int i = 0; i < kTriE; ++i) r[i] = a6[i];
    }
    double a[kTriE], ei[kTriE];
#pragma unroll
    for (int i = 0; i < kTriE; ++i) a[i] = r[i];
    add_e_diagonal(A, s.pt, po, a, s.valid && lane == s.last);
    if (!s.valid) set_identity_e(a);
    invert_spd_e(a, ei);
    if (s.valid && lane == s.last) store_ete_inverse(A, s.pt, ei);
    if constexpr (MODE == kInit) {
      if (A.etb_out && s.valid && lane == s.last) store_point_capture(A.etb_out, po, r + kTriE);
      double g[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) g[j] = r[kTriE + j];
      init_apply<LDS>(A, s, sl, ei, g, acc);
    }
  } else if constexpr (MODE == kColNorm) {
    // diag(J^T J): BlockSparseMatrix::SquaredColumnNorm (I/block_sparse_matrix.cc:351-401), one pass
    double w[NE];
    e_col_squares(s, w);
    if (!s.valid) {
#pragma unroll
      for (int j = 0; j < NE; ++j) w[j] = 0;
    }
    scatter_f_squares(s, acc);
    seg_scan<NE>(w, lane, s.first, span);
    if (s.valid && lane == s.last) {
#pragma unroll
      for (int j = 0; j < NE; ++j) A.y_e[po + j] = w[j];
    }
  } else if constexpr (MODE == kJx) {
    // model cost change of a trust-region step: -(J x)'(f + J x / 2), I/trust_region_minimizer.cc:420-438;
    // no per-point or per-camera reduction, every tile (also those of long points) is independent
    double xc[NF];
    load_xc(A, s.cam, xc);
    double xe[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) xe[j] = A.x_e[po + j];
    double m[NR], ex[NR];
    f_times(s, acc, xc, m);
    e_times(s.e, xe, ex);
#pragma unroll
    for (int r = 0; r < NR; ++r) m[r] += ex[r];
    if (s.valid) lane_acc -= cost_terms(m, s.b, 0.5);
  } else if constexpr (MODE == kCgnrInit) {
    // CGNR set-up in one pass: rhs = J^T b (point part by segment sums, camera part scattered)
    // and, if requested, the JACOBI point blocks (E^T E + D^2)^-1.
    double r[kNX];
    slot_point_sums(s, r);
    scatter_ft<LDS>(A, s, acc, s.b);
    seg_scan<kNX>(r, lane, s.first, span);
    if (s.valid && lane == s.last) {
#pragma unroll
      for (int j = 0; j < NE; ++j) A.y_e[po + j] = r[kTriE + j];
      if (A.point_blocks) {
        double a[kTriE], ei[kTriE];
#pragma unroll
        for (int i = 0; i < kTriE; ++i) a[i] = r[i];
        add_e_diagonal(A, s.pt, po, a, true);
        invert_spd_e(a, ei);
        store_ete_inverse(A, s.pt, ei);
      }
    }
  } else if constexpr (MODE == kBackSub) {
    double zc[NF], ei[kTriE];
    load_xc(A, s.cam, zc);
    load_ete_inverse(A, s.pt, ei);  // issued with the other loads, by all lanes, not behind the scan
    double t[NR];
    f_times(s, acc, zc, t);
#pragma unroll
    for (int r = 0; r < NR; ++r) t[r] = s.b[r] - t[r];
    double u[NE];
    et_times(s.e, t, u);
    if (!s.valid) {
#pragma unroll
      for (int j = 0; j < NE; ++j) u[j] = 0;
    }
    seg_scan<NE>(u, lane, s.first, span);
    double v[NE];
    sym_mul(ei, u, v);  // the point's solution on the last lane of its segment
    if (s.valid && lane == s.last) store_point_solution(A, po, v);
    if (A.scalar_out) {
      // Model cost change of the trust-region step -x, fused: with m = J x of this observation
      // (F z + E y, y broadcast from the segment's last lane), -(J step)'(f + J step / 2) = m'(f - m / 2).
      // I/trust_region_minimizer.cc:420-438; saves the separate pass over J (kJx) per LM step.
#pragma unroll
      for (int j = 0; j < NE; ++j) v[j] = shfl_idx(v[j], s.last);
      double m[NR];
      e_times(s.e, v, m);
#pragma unroll
      for (int r = 0; r < NR; ++r) m[r] += s.b[r] - t[r];
      if (s.valid) lane_acc += cost_terms(m, s.b, -0.5);
    }
  }
}

// A point with more than 64 observations: tiles [tile, tile+nt) belong to it alone.
// Sweep 1 accumulates the per-point sums over all its tiles, sweep 2 (only where the
// per-observation result depends on them) re-reads the tiles, which are L2-warm.
template <int MODE, bool LDS, bool F32>
__device__ __forceinline__ void process_long_point(const BalArgs& A, int64_t tile, int nt, int lane, Ctx& acc, double& lane_acc) {
  if constexpr (MODE == kShBlocks) {
    shared_block_sums_long(A, tile, nt, lane, acc);
    return;
  }
  Slot s;
  if constexpr (MODE == kColNorm) {
    double w[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) w[j] = 0.0;
    int pt = 0;
    for (int t = 0; t < nt; ++t) {
      load_slot<true, F32>(A, tile + t, lane, s, false);
      if (t == 0) pt = __shfl(s.pt, 0, 64);
      scatter_f_squares(s, acc);
      if (s.valid) {
        double q[NE];
        e_col_squares(s, q);
#pragma unroll
        for (int j = 0; j < NE; ++j) w[j] += q[j];
      }
    }
    wave_allreduce<NE>(w);
    if (lane == 0) {
      const int po = pt_off(A, pt);
#pragma unroll
      for (int j = 0; j < NE; ++j) A.y_e[po + j] = w[j];
    }
    return;
  }
  if constexpr (MODE == kSx || MODE == kBackSub || MODE == kSpseZ) {
    double u[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) u[j] = 0.0;
    int pt = 0;
    for (int t = 0; t < nt; ++t) {
      load_slot<kCanGather<MODE>, F32>(A, tile + t, lane, s, kWantsB<MODE>);
      if (t == 0) pt = __shfl(s.pt, 0, 64);
      double xc[NF];
      load_xc(A, s.cam, xc);
      double ft[NR];
      f_times(s, acc, xc, ft);
      if constexpr (MODE == kBackSub) {
#pragma unroll
        for (int r = 0; r < NR; ++r) ft[r] = s.b[r] - ft[r];
      }
      if (s.valid) {
        double q[NE];
        et_times(s.e, ft, q);
#pragma unroll
        for (int j = 0; j < NE; ++j) u[j] += q[j];
      }
    }
    wave_allreduce<NE>(u);
    double ei[kTriE], v[NE];
    load_ete_inverse(A, pt, ei);
    sym_mul(ei, u, v);
    if constexpr (MODE == kBackSub) {
      if (lane == 0) store_point_solution(A, pt_off(A, pt), v);
      if (A.scalar_out) {  // fused model cost change: second sweep over the point's (L2-warm) tiles
        for (int t = 0; t < nt; ++t) {
          load_slot<false, F32>(A, tile + t, lane, s, true, false);
          double xc[NF];
          load_xc(A, s.cam, xc);
          double m[NR], ev[NR];
          f_times(s, acc, xc, m);
          e_times(s.e, v, ev);
#pragma unroll
          for (int r = 0; r < NR; ++r) m[r] += ev[r];
          if (s.valid) lane_acc += cost_terms(m, s.b, -0.5);
        }
      }
    } else {
      for (int t = 0; t < nt; ++t) {
        load_slot<false, F32>(A, tile + t, lane, s, false, false);
        double xc[NF];
        load_xc(A, s.cam, xc);
        double ft[NR], ev[NR], z[NR];
        f_times(s, acc, xc, ft);
        e_times(s.e, v, ev);
#pragma unroll
        for (int r = 0; r < NR; ++r) z[r] = MODE == kSx ? ft[r] - ev[r] : ev[r];
        scatter_ft<LDS>(A, s, acc, z);
      }
    }
  } else if constexpr (MODE == kJtJx || MODE == kJtb) {
    double w[NE], xp[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) { w[j] = 0.0; xp[j] = 0.0; }
    int pt = 0, po = 0;
    for (int t = 0; t < nt; ++t) {
      load_slot<kCanGather<MODE>, F32>(A, tile + t, lane, s, kWantsB<MODE>);
      if (t == 0) {
        pt = __shfl(s.pt, 0, 64);
        po = pt_off(A, pt);
        if constexpr (MODE == kJtJx) {
#pragma unroll
          for (int j = 0; j < NE; ++j) xp[j] = A.x_e[po + j];
        }
      }
      double z[NR];
      if constexpr (MODE == kJtJx) {
        double xc[NF];
        load_xc(A, s.cam, xc);
        f_times(s, acc, xc, z);
        double ex[NR];
        e_times(s.e, xp, ex);
#pragma unroll
        for (int r = 0; r < NR; ++r) z[r] += ex[r];
      } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) z[r] = s.b[r];
      }
      scatter_ft<LDS>(A, s, acc, z);
      if (s.valid) {
        double q[NE];
        et_times(s.e, z, q);
#pragma unroll
        for (int j = 0; j < NE; ++j) w[j] += q[j];
      }
    }
    wave_allreduce<NE>(w);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        double d = 0;
        if (MODE == kJtJx && A.D_e) { d = A.D_e[po + j]; d = d * d * xp[j]; }
        A.y_e[po + j] = w[j] + d;
        if (MODE == kJtJx) lane_acc += xp[j] * (w[j] + d);  // x_e . y_e share of CG's p.q
      }
    }
  } else if constexpr (MODE == kInit || MODE == kEte || MODE == kCgnrInit) {
    double r[kNX];
#pragma unroll
    for (int i = 0; i < kNX; ++i) r[i] = 0.0;
    int pt = 0;
    for (int t = 0; t < nt; ++t) {
      load_slot<kCanGather<MODE>, F32>(A, tile + t, lane, s, kWantsB<MODE>);
      if (t == 0) pt = __shfl(s.pt, 0, 64);
      if constexpr (MODE == kCgnrInit) scatter_ft<LDS>(A, s, acc, s.b);
      double q[kNX];
      slot_point_sums(s, q);
#pragma unroll
      for (int i = 0; i < kNX; ++i) r[i] += q[i];
    }
    wave_allreduce<kNX>(r);
    const int po = pt_off(A, pt);
    double a[kTriE], ei[kTriE];
#pragma unroll
    for (int i = 0; i < kTriE; ++i) a[i] = r[i];
    add_e_diagonal(A, pt, po, a, lane == 0);
    invert_spd_e(a, ei);
    if constexpr (MODE == kCgnrInit) {
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NE; ++j) A.y_e[po + j] = r[kTriE + j];
        if (A.point_blocks) store_ete_inverse(A, pt, ei);
      }
    } else {
      if (lane == 0) store_ete_inverse(A, pt, ei);
    }
    if constexpr (MODE == kInit) {
      if (A.etb_out && lane == 0) store_point_capture(A.etb_out, po, r + kTriE);
      double g[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) g[j] = r[kTriE + j];
      for (int t = 0; t < nt; ++t) {
        load_slot<false, F32>(A, tile + t, lane, s, true, false);  // second sweep: from the tiles just written
        const int64_t sl = (tile + t) * kTile + lane;
        init_apply<LDS>(A, s, sl, ei, g, acc);
      }
    }
  }
}

// The long points of the unpipelined kernels, in the same ROUNDS as the streaming kernels' (plan.cc, compute_long_round): the waves of
// a workgroup — in sub-workgroups of kRoundWaves — take one tile each, exchange the tile's sums (3 or 9 doubles) through LDS and finish
// the tile from registers; a point of more than kRoundWaves tiles runs sum rounds, then (where the per-observation result needs the
// sums: S.x, Init's M_o and rhs, the model cost of the back-substitution) apply rounds that re-read its tiles.  Every wave of the
// workgroup runs the same number of rounds (the barriers are the workgroup's): a sub-workgroup out of rounds idles.
template <int MODE, bool LDS, int BLOCK, bool F32>
__device__ __forceinline__ void fused_long_rounds(const BalArgs& A, int lane, bool grouped, int range, Ctx& acc, double& lane_acc) {
  constexpr int NX = (MODE == kInit || MODE == kEte || MODE == kCgnrInit) ? kNX : NE;
  constexpr int SUBS = BLOCK / 64 / kRoundWaves;
  constexpr bool kTwoPhase = (MODE == kSx || MODE == kSpseZ || MODE == kInit || MODE == kBackSub);
  static_assert(SUBS >= 1, "a workgroup holds at least one round");
  __shared__ double xr[SUBS][kRoundWaves][NX];
  const int wave_all = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int sub = wave_all / kRoundWaves, wave = wave_all % kRoundWaves;
  // a workgroup that owns a hybrid group takes the group's sequences; otherwise the workgroups share ALL sequences (also those of a
  // hybrid plan: the passes that scatter nothing walk every tile)
  const int64_t qe = grouped ? int64_t(A.round_ptr[range + 1]) : int64_t(A.n_seq);
  const int64_t qstride = grouped ? 1 : int64_t(gridDim.x) * SUBS;
  const int64_t q_first = grouped ? int64_t(A.round_ptr[range]) : logical_workgroup() * SUBS;
  // rounds of the busiest sub-workgroup (a hybrid group's sequences all go to sub-workgroup 0: scattering modes run 8 waves there)
  int64_t n_iter = 0;
  for (int j = 0; j < (grouped ? 1 : SUBS); ++j) {
    int64_t n = 0;
    if (grouped) { if (q_first < qe) n = A.seq_ptr[qe] - A.seq_ptr[q_first]; }
    else for (int64_t q = q_first + j; q < qe; q += qstride) n += A.seq_ptr[q + 1] - A.seq_ptr[q];
    n_iter = max(n_iter, n);
  }
  int64_t it_q = q_first + (grouped ? 0 : sub);
  bool it_real = grouped ? (sub == 0 && it_q < qe) : it_q < qe;
  int64_t it_r = 0, it_end = 0;
  if (it_real) { it_r = A.seq_ptr[it_q]; it_end = A.seq_ptr[grouped ? qe : it_q + 1]; if (grouped) it_q = qe - 1; }
  double carry[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) carry[i] = 0.0;
  for (int64_t iter = 0; iter < n_iter; ++iter) {
    uint32_t word = kRoundIdle, word0 = kRoundIdle;
    int flag = 0;
    if (it_real) {
      word = A.round_word[it_r * kRoundWaves + wave];
      word0 = A.round_word[it_r * kRoundWaves];
      flag = A.round_flag[it_r];
      if (it_r + 1 < it_end) ++it_r;
      else if (it_q + qstride < qe) { it_q += qstride; it_r = A.seq_ptr[it_q]; it_end = A.seq_ptr[it_q + 1]; }
      else it_real = false;
    }
    const bool active = word != kRoundIdle;
    const int64_t tile = int64_t(word & 0x3FFFFFFu);
    const int w0 = flag ? 0 : (active ? int((word >> 26) & 7u) : wave);
    const int cnt = flag ? (word0 != kRoundIdle ? int((word0 >> 29) & 7u) + 1 : 1) : (active ? int((word >> 29) & 7u) + 1 : 1);
    const bool apply_round = (flag & kRoundApply) != 0;
    Slot s;
    s.valid = false; s.nocam = false; s.pt = 0; s.cam = 0; s.acc = kSlotSpill; s.zbase = 0; s.slot = 0;
    zero_b(s);
    double part[NX], ft[NR], xp[NE];
#pragma unroll
    for (int i = 0; i < NX; ++i) part[i] = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) ft[r] = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) xp[j] = 0.0;
    int pt = 0, po = 0;
    if (active && (!apply_round || kTwoPhase)) {
      // (an apply round re-reads the tiles the sum rounds wrote: never a gather)
      load_slot<kCanGather<MODE>, F32>(A, tile, lane, s, kWantsB<MODE>, !apply_round);
      pt = __builtin_amdgcn_readfirstlane(s.pt);   // one segment: every valid lane holds the point
      po = pt_off(A, pt);
    }
    // ---- this tile's share of the point's sums
    if (active && !apply_round) {
      if constexpr (MODE == kColNorm) {
        scatter_f_squares(s, acc);
        if (s.valid) e_col_squares(s, part);
      } else if constexpr (MODE == kSx || MODE == kSpseZ || MODE == kBackSub) {
        double xc[NF];
        load_xc(A, s.cam, xc);
        f_times(s, acc, xc, ft);
        if constexpr (MODE == kBackSub) {
#pragma unroll
          for (int r = 0; r < NR; ++r) ft[r] = s.b[r] - ft[r];
        }
        if (s.valid) et_times(s.e, ft, part);
      } else if constexpr (MODE == kJtJx || MODE == kJtb) {
        double z[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) z[r] = s.b[r];
        if constexpr (MODE == kJtJx) {
#pragma unroll
          for (int j = 0; j < NE; ++j) xp[j] = A.x_e[po + j];
          double xc[NF];
          load_xc(A, s.cam, xc);
          f_times(s, acc, xc, z);
          double ex[NR];
          e_times(s.e, xp, ex);
#pragma unroll
          for (int r = 0; r < NR; ++r) z[r] += ex[r];
        }
        scatter_ft<LDS>(A, s, acc, z);
        if (s.valid) et_times(s.e, z, part);
      } else {
        static_assert(MODE == kInit || MODE == kEte || MODE == kCgnrInit, "set-up modes");
        if constexpr (MODE == kCgnrInit) scatter_ft<LDS>(A, s, acc, s.b);
        slot_point_sums(s, part);
      }
      wave_allreduce<NX>(part);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[sub][wave][i] = part[i];
      }
    }
    __syncthreads();
    double tot[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) tot[i] = 0.0;
    if ((active || flag) && !apply_round) {   // (an idle wave of a sum round adds up too: it may hold a tile in the apply rounds)
      for (int k = 0; k < cnt; ++k) {
#pragma unroll
        for (int i = 0; i < NX; ++i) tot[i] += xr[sub][w0 + k][i];
      }
    }
    __syncthreads();
    if (flag & kRoundSum) {
#pragma unroll
      for (int i = 0; i < NX; ++i) { carry[i] += tot[i]; tot[i] = carry[i]; }
      if (!(flag & kRoundLast)) continue;
      if constexpr (!kTwoPhase) {
#pragma unroll
        for (int i = 0; i < NX; ++i) carry[i] = 0.0;
      }
    } else if (apply_round) {
#pragma unroll
      for (int i = 0; i < NX; ++i) tot[i] = carry[i];
      if (flag & kRoundLast) {
#pragma unroll
        for (int i = 0; i < NX; ++i) carry[i] = 0.0;
      }
      if constexpr (!kTwoPhase) continue;
    }
    if (!active) continue;
    // ---- the point's sums are in tot.  `finish`: what is stored once per point (first wave of the point; a point of more than
    // kRoundWaves tiles: in its last sum round).  `apply`: what every tile does with the sums (such a point: in its apply rounds).
    const bool finish = wave == w0 && lane == 0 && !apply_round;
    const bool apply = flag == 0 || apply_round;
    if constexpr (MODE == kColNorm || MODE == kJtb) {
      if (finish) {
#pragma unroll
        for (int j = 0; j < NE; ++j) A.y_e[po + j] = tot[j];
      }
    } else if constexpr (MODE == kJtJx) {
      if (finish) {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
          double d = 0;
          if (A.D_e) { d = A.D_e[po + j]; d = d * d * xp[j]; }
          A.y_e[po + j] = tot[j] + d;
          lane_acc += xp[j] * (tot[j] + d);
        }
      }
    } else if constexpr (MODE == kSx || MODE == kSpseZ || MODE == kBackSub) {
      double ei[kTriE], v[NE], u[NE];
      load_ete_inverse(A, pt, ei);
#pragma unroll
      for (int j = 0; j < NE; ++j) u[j] = tot[j];
      if constexpr (MODE == kSx && LDS) {
        if (A.u_out && finish) store_point_capture(A.u_out, NE * pt, u);
      }
      sym_mul(ei, u, v);
      if constexpr (MODE == kBackSub) {
        if (finish) store_point_solution(A, po, v);
        if (!A.scalar_out || !apply) continue;
      } else if (!apply) continue;
      if (apply_round) {   // the sums came from earlier rounds: this tile's F x again
        double xc[NF];
        load_xc(A, s.cam, xc);
        f_times(s, acc, xc, ft);
        if constexpr (MODE == kBackSub) {
#pragma unroll
          for (int r = 0; r < NR; ++r) ft[r] = s.b[r] - ft[r];
        }
      }
      double ev[NR];
      e_times(s.e, v, ev);
      if constexpr (MODE == kBackSub) {   // fused model cost change: J x = F z + E x_e with F z = b - t
        double m[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) m[r] = (s.b[r] - ft[r]) + ev[r];
        if (s.valid) lane_acc += cost_terms(m, s.b, -0.5);
      } else {
        double z[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) z[r] = MODE == kSx ? ft[r] - ev[r] : ev[r];
        scatter_ft<LDS>(A, s, acc, z);
      }
    } else {
      double a[kTriE], ei[kTriE];
#pragma unroll
      for (int i = 0; i < kTriE; ++i) a[i] = tot[i];
      add_e_diagonal(A, pt, po, a, finish);
      invert_spd_e(a, ei);
      if constexpr (MODE == kCgnrInit) {
        if (finish) {
#pragma unroll
          for (int j = 0; j < NE; ++j) A.y_e[po + j] = tot[kTriE + j];
          if (A.point_blocks) store_ete_inverse(A, pt, ei);
        }
      } else {
        if (finish) store_ete_inverse(A, pt, ei);
      }
      if constexpr (MODE == kInit) {
        if (A.etb_out && finish) store_point_capture(A.etb_out, po, tot + kTriE);
        if (apply) {
          double g[NE];
#pragma unroll
          for (int j = 0; j < NE; ++j) g[j] = tot[kTriE + j];
          init_apply<LDS>(A, s, tile * kTile + lane, ei, g, acc);
        }
      }
    }
  }
}

template <int MODE, bool LDS, int BLOCK, bool F32>
__global__ __launch_bounds__(BLOCK) void bal_fused_kernel(BalArgs A) {
  extern __shared__ double lds_acc[];
  if constexpr (MODE == kInit || MODE == kCgnrInit) {
    if (A.clear_flags && blockIdx.x == 0 && threadIdx.x == 0) { A.clear_flags[0] = 0; A.clear_flags[1] = 0; }
  }
  if (A.status && *A.status != 0) return;  // CG already terminated: nothing to do
  if (A.run_after_cg && !CgStatusAllowsSolution(*A.run_after_cg)) return;  // speculative tail: CG has not ended (or failed)
  if constexpr (MODE == kBackSub) {   // ... or the point tail, enqueued beside this pass, finishes the solve (device.h)
    if (A.run_after_cg && A.skip_updates && PointTailTakes(*A.run_after_cg, *A.skip_updates)) return;
  }
  constexpr bool kScatters = (MODE == kSx || MODE == kJtJx || MODE == kJtb || MODE == kInit || MODE == kCgnrInit || MODE == kColNorm || MODE == kSpseZ);
  Ctx acc;
  ctx_init(A, acc, nullptr);
  if constexpr (kScatters) {
    // every camera's accumulator row and the strip's entries (LDS), or the hybrid rows of this workgroup — hyb_rows of them, then one strip per wave (scatter_ft)
    acc.lds = lds_acc;
    const int n_acc = LDS ? A.n_acc : NF * A.hyb_rows;
    for (int i = threadIdx.x; i < n_acc; i += BLOCK) acc.lds[i] = 0.0;
    __syncthreads();
  }
  if constexpr (MODE == kBackSub || MODE == kJx) {
    if (A.x_lds_scalars > 0) {   // (launch-uniform) the camera part of x into LDS: row c = camera c
      for (int i = threadIdx.x; i < A.x_lds_scalars; i += BLOCK) lds_acc[i] = A.x_f[cam_off(A, i / NF) + i % NF];
      __syncthreads();
    }
  }
  const int lane = threadIdx.x & 63;
  double lane_acc = 0.0;
  if constexpr (MODE == kBackSub) {  // y_f = z (:238-242), a few KB: no separate copy launch
    if (A.copy_dst)
      for (int i = blockIdx.x * BLOCK + threadIdx.x; i < A.copy_n; i += gridDim.x * BLOCK) {
        const double z = A.copy_src[i];
        A.copy_dst[i] = A.negate_out ? -z : z;
        if (A.negate_out && !isfinite(z)) atomicAdd(A.nonfinite, 1);
      }
  }
  // grid-strided over [tile_begin, tile_end); hybrid accumulation: workgroup g owns the tiles of group g (plan.cc)
  const bool grouped = kScatters && !LDS && A.grp_tile_ptr != nullptr;
  const int64_t tile0 = grouped ? A.grp_tile_ptr[blockIdx.x] + (threadIdx.x >> 6) : A.tile_begin + logical_workgroup() * (BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = grouped ? BLOCK / 64 : int64_t(gridDim.x) * (BLOCK / 64);
  const int64_t tile_end = grouped ? A.grp_tile_ptr[blockIdx.x + 1] : (A.tile_end > 0 ? A.tile_end : A.n_tiles);
  if constexpr (MODE == kShBlocks) {
    for (int64_t tile = tile0; tile < tile_end; tile += nwaves) {
      const int kind = A.tile_kind[tile];
      const int aux = A.tile_aux[tile];
      if (kind == 2) continue;
      if (kind == 0) process_tile<MODE, LDS, F32>(A, tile, lane, aux & 0xff, aux >> 8, acc, lane_acc);
      else process_long_point<MODE, LDS, F32>(A, tile, aux, lane, acc, lane_acc);
    }
  } else if (tile0 < tile_end) {
    // the index words (SlotPre) and tile words of the NEXT tile of this wave's walk are in flight while this one is computed; past
    // the end the last tile's are asked for again (one code path)
    constexpr bool kPre = CERES_HIP_AB_PREFETCH != 0;   // (A/B builds: 0 = every tile loads its own index words, as before round 6)
    // CERES_HIP_AB_PREFETCH=2 (A/B builds; NOT the default): on a step's first pass (the values still in the caller's layout) the next
    // tile's VALUES are in flight as well, through index words that are then asked for TWO tiles ahead.  Measured level with index words
    // only on every shape (Venice 1.492 / 1.505 against 1.486 / 1.494 ms per step, Ladybug 0.329 both, kInit 501 us on Venice either way:
    // profiles/r06v_values_prefetch_ab.jsonl) — the pass moves its 2.39 GB at what a device copy reaches, it is not waiting for a chain.
    // (512-thread instances: at 1024 threads a wave has 128 registers, the second set of values would live in scratch)
    constexpr bool kVal = CERES_HIP_AB_PREFETCH >= 2 && kCanGather<MODE> && MODE != kJx && BLOCK <= 512;
    if (kVal && A.src_values) {   // (launch-uniform)
      if constexpr (kVal) {
        SlotPre p0, p1, p2;
        ValPre v0, v1;
        const int64_t t1 = tile0 + nwaves < tile_end ? tile0 + nwaves : tile0;
        issue_pre<true>(A, tile0, lane, p0);
        issue_pre<true>(A, t1, lane, p1);
        int kind = A.tile_kind[tile0], aux = A.tile_aux[tile0];
        int kind_n = A.tile_kind[t1], aux_n = A.tile_aux[t1];
        bool have0 = kind == 0, have1 = false;   // (wave-uniform)
        if (have0) issue_values(A, tile0, lane, p0, v0);
        for (int64_t tile = tile0; tile < tile_end; tile += nwaves) {
          const int64_t tn = tile + nwaves < tile_end ? tile + nwaves : tile;
          const int64_t tnn = tn + nwaves < tile_end ? tn + nwaves : tn;
          const int kind_nn = A.tile_kind[tnn], aux_nn = A.tile_aux[tnn];
          issue_pre<true>(A, tnn, lane, p2);
          have1 = kind_n == 0 && tn != tile;
          if (have1) issue_values(A, tn, lane, p1, v1);
          __builtin_amdgcn_sched_barrier(0);
          if (kind == 0) process_tile<MODE, LDS, F32>(A, tile, lane, aux & 0xff, aux >> 8, acc, lane_acc, &p0, &v0, have0);
          else if (kind == 1) process_long_point<MODE, LDS, F32>(A, tile, aux, lane, acc, lane_acc);
          __builtin_amdgcn_sched_barrier(0);
          p0 = p1; p1 = p2; have0 = have1;
#pragma unroll
          for (int i = 0; i < 2 * kPairs; ++i) v0.v[i] = v1.v[i];   // (element by element: a struct copy is a memcpy, which keeps both sets in scratch)
#pragma unroll
          for (int r = 0; r < NR; ++r) v0.b[r] = v1.b[r];
          kind = kind_n; aux = aux_n; kind_n = kind_nn; aux_n = aux_nn;
        }
      }
    } else {
      SlotPre pre, nxt;
      if constexpr (kPre) issue_pre<kCanGather<MODE>>(A, tile0, lane, pre);
      int kind = A.tile_kind[tile0], aux = A.tile_aux[tile0];
      for (int64_t tile = tile0; tile < tile_end; tile += nwaves) {
        const int64_t tn = tile + nwaves < tile_end ? tile + nwaves : tile;
        const int kind_n = A.tile_kind[tn], aux_n = A.tile_aux[tn];
        if constexpr (kPre) issue_pre<kCanGather<MODE>>(A, tn, lane, nxt);
        if constexpr (MODE == kJx) {
          process_tile<MODE, LDS, F32>(A, tile, lane, 1, 0, acc, lane_acc, kPre ? &pre : nullptr);
        } else {
          // 2: a long point's continuation; 3: the head of a long point that is taken in rounds (below)
          if (kind == 0) process_tile<MODE, LDS, F32>(A, tile, lane, aux & 0xff, aux >> 8, acc, lane_acc, kPre ? &pre : nullptr);
          else if (kind == 1) process_long_point<MODE, LDS, F32>(A, tile, aux, lane, acc, lane_acc);
        }
        if constexpr (kPre) pre = nxt;
        kind = kind_n; aux = aux_n;
      }
    }
  }
  if constexpr (MODE != kJx && MODE != kShBlocks) {
    if (A.round_word) fused_long_rounds<MODE, LDS, BLOCK, F32>(A, lane, grouped, grouped ? int(blockIdx.x) : 0, acc, lane_acc);   // (workgroup-uniform)
  }
  if constexpr (MODE == kShBlocks && NS > 0) {   // the workgroup's share of the strip's matrix: kTriS sums, lanes then waves in a fixed order
    __shared__ double st[BLOCK / 64][kTriSX];
    double v[kTriSX];
#pragma unroll
    for (int i = 0; i < kTriSX; ++i) v[i] = acc.tt[i];
    wave_allreduce<kTriSX>(v);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kTriSX; ++i) st[threadIdx.x >> 6][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < kTriS) {
      double t = 0;
      for (int w = 0; w < BLOCK / 64; ++w) t += st[w][threadIdx.x];
      A.scalar_out[int64_t(blockIdx.x) * kTriS + threadIdx.x] = t;
    }
  }
  double* const scalar_dst = MODE == kJtJx ? A.pq_out : A.scalar_out;
  if ((MODE == kJx || MODE == kBackSub || MODE == kJtJx) && scalar_dst) {  // one partial per workgroup, summed in fixed order by the caller
    __shared__ double red[16];
    double v = lane_acc;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0;
      for (int i = 0; i < BLOCK / 64; ++i) t += red[i];
      if (MODE == kJtJx && A.pq_accumulate) t += scalar_dst[blockIdx.x];
      scalar_dst[blockIdx.x] = t;
    }
  }
  if constexpr (kScatters && LDS) {
    flush_shared_sums(A, acc);
    __syncthreads();
    double* out = A.partials + int64_t(blockIdx.x) * A.n_acc;
    for (int i = threadIdx.x; i < A.n_acc; i += BLOCK) out[i] = acc.lds[i];
  } else if constexpr (kScatters) {
    flush_shared_sums_global(A, acc);
    if (A.hyb_rows > 0) {  // this workgroup's accumulator rows join the spilled rows in the ring: the second pass sums both
      __syncthreads();
      double* out = A.zbuf + NF * (A.z_flush_row0 + int64_t(blockIdx.x) * A.hyb_rows);
      for (int i = threadIdx.x; i < NF * A.hyb_rows; i += BLOCK) out[i] = acc.lds[i];
    }
  }
}

#if CERES_HIP_PIPELINED   // (the pipelined kernels and their cooperative point-space accesses count in threes and in pairs of rows:
                          // 3-wide points with 2-high rows only; the other shapes run the streaming modes on bal_fused_kernel)
// (two-row forms of f_times / scatter_ft for the code below)
__device__ __forceinline__ void f_times(const Slot& s, const Ctx& c, const double (&xc)[NF], double& t0, double& t1) {
  double t[NR];
  f_times(s, c, xc, t);
  t0 = t[0]; t1 = t[1 % NR];
}
template <bool LDS>
__device__ __forceinline__ void scatter_ft(const BalArgs& A, const Slot& s, Ctx& c, double z0, double z1) {
  double z[NR];
  z[0] = z0; z[1 % NR] = z1;
  scatter_ft<LDS>(A, s, c, z);
}
// Software-pipelined variant of the streaming modes (kSx, kSpseZ, kJtJx; packed fp64 tiles,
// points-then-cameras vector layout).  bal_fused_kernel runs load -> wait -> compute -> store per
// tile and leans on the other 3 waves of its SIMD to keep HBM busy; the SQ counters
// (profiles/r01d_pmc_sq_*.txt) show its waves parked in s_waitcnt 45-60 % of their cycles, and
// switching the 24 MB of point-space stores of JtJx off saved 12 % — vmcnt retires in order, so
// the write acknowledgement of tile N sat in front of the loads of tile N+1.  Here a wave always
// has the next tile in flight while it computes (8 waves per CU, 512 threads, <= 256 VGPRs):
//   stage N:  issue index words (N+2) | issue pairs (N+1) | issue aux (N+1), addressed through
//             index words (N+1) that were issued a stage ago | compute (N) | store (N)
// so compute(N) only waits for loads issued during stage N-1, and a store has a whole stage to
// retire before anything queued behind it is needed.
// s_waitcnt counts are static, so every path through a stage must issue the SAME loads in the
// same order or the compiler has to fall back to vmcnt(0): no load here sits under a
// wave-uniform condition (the host picks this kernel only when x_f is unpadded, the layout is
// contiguous and — kJtJx — D is given), a wave past its last tile re-issues that tile, and
// tiles of long points run through compute() with every lane invalid.
// Row of the slot's camera in the LDS copy of x_f (BalArgs::xhot_cam), or -1.  n_xhot is 0 unless every camera's accumulator is in LDS,
// and only then does the word's row field carry this (plan.cc); invalid slots have kSlotSpill there.
__device__ __forceinline__ int hot_x_row(const BalArgs& A, const Slot& s) {
  const unsigned r = unsigned(s.acc) - 1u;
  return (A.n_xhot > 0 && s.valid && r < unsigned(A.n_xhot)) ? int(r) : -1;
}
// The camera part of x for the slots of popular cameras, from LDS, at the head of the stage that computes (an LDS round trip of a
// hundred cycles there costs less than carrying nine more doubles per register set through the issue stage).
__device__ __forceinline__ void take_hot_x(const BalArgs& A, const Slot& s, const double* __restrict__ xh, StreamAux& x) {
  if (A.n_xhot <= 0) return;   // (launch-uniform)
  const int r = hot_x_row(A, s);
  const double* row = xh + NF * (r >= 0 ? r : 0);
  double t[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) t[k] = row[k];
#pragma unroll
  for (int k = 0; k < NF; ++k) x.xc[k] = r >= 0 ? t[k] : x.xc[k];
}
template <int MODE>
__device__ __forceinline__ void issue_aux(const BalArgs& A, const Slot& s, int lane, int npts, StreamAux& x) {
#if CERES_HIP_AB_ABLATE & 96   // 32: lanes of the 440 most popular cameras (synthetic: the lowest ids) all read camera 0's line; 64: every lane does
  const double* xf = A.x_f + A.cam_base + NF * int64_t((CERES_HIP_AB_ABLATE & 64) || s.cam < 440 ? 0 : s.cam);
#else
  // a slot whose camera has its part of x in LDS (hot_x_row) still issues the gather — the load count of a stage must not depend on
  // the data — but every such lane asks for the same line (camera 0's), which the wave's request coalesces into one
  const double* xf = A.x_f + A.cam_base + NF * int64_t(hot_x_row(A, s) >= 0 ? 0 : s.cam);
#endif
#if CERES_HIP_AB_ABLATE & 2
#pragma unroll
  for (int j = 0; j < NF; ++j) x.xc[j] = 1.0 + 0.001 * j + 1e-6 * s.cam;
#else
  load_camera_scalars(xf, x.xc);
#endif
  x.xa = x.xb = x.da = x.db = 0.0;
  x.base = 0;
  x.coop = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) { x.xp[j] = 0.0; x.dd[j] = 0.0; }
  if constexpr (MODE == kSx || MODE == kSpseZ) {
#if CERES_HIP_AB_ABLATE & 8
#pragma unroll
    for (int j = 0; j < kTriE; ++j) x.ei[j] = 0.5 + 0.01 * j + 1e-7 * s.pt;
#else
    load_ete_inverse(A, s.pt, x.ei);
#endif
  } else {
    const int n3 = 3 * npts;
    x.base = 3 * int64_t(__builtin_amdgcn_readfirstlane(s.pt));
    // per-lane predicates only mask lanes, the four load instructions are always issued
    // (lanes past the range read scalar 0 of it; nothing downstream looks at those lanes, and
    // selecting zeros here would consume the loads — a wait — in the issue phase)
    const bool a = lane < n3, b = lane + 64 < n3;
    const int64_t ia = x.base + (a ? lane : 0), ib = x.base + (b ? 64 + lane : 0);
    x.xa = load_xe(A.x_e + ia); x.da = load_xe(A.D_e + ia); x.xb = load_xe(A.x_e + ib); x.db = load_xe(A.D_e + ib);
  }
}

// The rest of CG iteration `it` by ONE workgroup, for a camera space of at most kCgTailMax scalars (CgTail, device.h): q = S p from the
// workgroups' partial sums (+ D_f^2 p), then ConjugateGradientsSolver's step exactly as cg_update_kernel and
// cg_finalize_direction_kernel split it (I/conjugate_gradients_solver.h:190-290): p.q, alpha, x += alpha p, r -= alpha q, z = M^-1 r,
// Q1, |r|, the termination tests, beta, p = z + beta p — same scalars, same failure codes, same double-buffered rho / Q0.
// `lds`: the workgroup's accumulator array (n_acc doubles, flushed already): scratch for q, then for the new r.
template <int BLOCK>
__device__ __forceinline__ void cg_iteration_tail(const BalArgs& A, double* lds) {
  static_assert(BLOCK > 0 && kHasCgTail && NF == 9, "the tail indexes 9 x 9 blocks back to back");
  constexpr int PER = (kCgTailMax + BLOCK - 1) / BLOCK;
  __shared__ double sh[3][BLOCK / 64];
  const CgTail& T = A.tail;
  CgScalars& S = *T.S;
  const int n = A.n_acc, it = T.it, nparts = int(gridDim.x);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  auto sum3 = [&](double& a, double& b, double& c) {   // over the workgroup, fixed order; every thread gets the sums
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { a += __shfl_xor(a, m, 64); b += __shfl_xor(b, m, 64); c += __shfl_xor(c, m, 64); }
    __syncthreads();
    if (lane == 0) { sh[0][wv] = a; sh[1][wv] = b; sh[2][wv] = c; }
    __syncthreads();
    a = b = c = 0.0;
    for (int w = 0; w < BLOCK / 64; ++w) { a += sh[0][w]; b += sh[1][w]; c += sh[2][w]; }
  };
  // everything this kernel reads of S, before anything of it is written
  const int staged = S.fail_dir;
  const double rho = S.rho_pp[it & 1], Q0 = S.Q0_pp[it & 1], q_tol = S.q_tol, tol_r = S.tol_r;
  const int min_it = S.min_it, max_it = S.max_it;
  // everything the step reads of the CG vectors and of M^-1 is requested first, in one go with the partial sums: the tail is a chain
  // of memory round trips otherwise (11 us, as long as the three launches it replaces)
  double pv[PER], dv[PER], xo[PER], ro[PER], bv[PER], mrow[PER][9];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * BLOCK;
    const bool in = i < n;
    const int ii = in ? i : 0;
    pv[k] = T.p[ii]; dv[k] = T.D_f ? T.D_f[ii] : 0.0; xo[k] = T.x[ii]; ro[k] = T.r[ii]; bv[k] = T.rhs[ii];
    const double* m = T.blocks + int64_t(9) * ii;   // row (i % 9) of camera i / 9: 81 c + 9 a = 9 i
#pragma unroll
    for (int j = 0; j < 9; ++j) mrow[k][j] = m[j];
    if (!in) pv[k] = 0.0;
  }
  // the partial sums, all threads at once and every load of a thread independent of the others: (element i, subset sp) adds up the
  // partials sp, sp + ns, ... (at most kCgTailLoads of them: run_cg's condition) — ONE memory round trip; a thread per element walking
  // the partials alone was 35 us, batches of four dependent on each other 6 us
  const int ns = max(1, BLOCK / n);
  double* part = lds + n;   // [ns][n], behind the accumulator array (launch_stream2 sizes the LDS for it)
  {
    const int idx = threadIdx.x;
    const bool mine = idx < ns * n;
    const int sp = mine ? idx / n : 0, i = mine ? idx - sp * n : 0;
    double v[kCgTailLoads];
#pragma unroll
    for (int j = 0; j < kCgTailLoads; ++j) {
      const int w = sp + j * ns;
      v[j] = (mine && w < nparts) ? A.partials[int64_t(w) * n + i] : 0.0;
    }
#pragma unroll
    for (int h = kCgTailLoads / 2; h >= 1; h >>= 1) {
#pragma unroll
      for (int j = 0; j < h; ++j) v[j] += v[j + h];
    }
    if (mine) part[idx] = v[0];
  }
  __syncthreads();
  double qv[PER];
  double pq = 0, unused0 = 0, unused1 = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * BLOCK;
    qv[k] = 0.0;
    if (i < n) {
      double q = 0;
      for (int sp = 0; sp < ns; ++sp) q += part[sp * n + i];
      q += dv[k] * dv[k] * pv[k];
      qv[k] = q;
      pq += pv[k] * q;
    }
  }
  sum3(pq, unused0, unused1);
  if (staged) pq = 1.0;
  int fail = staged;
  double alpha = 0;
  if (!fail) {
    if (pq <= 0 || isinf(pq)) fail = kCgIndefinite;
    else { alpha = rho / pq; if (isinf(alpha)) fail = kCgFailAlpha; }
  }
  if (threadIdx.x == 0) {
    S.pq = pq; S.alpha = alpha; S.rho_new = rho; S.fail_step = fail;
    if (!fail) {   // x-update `it` is done: the point tail's history (device.h), as cg_update_kernel keeps it
      if (it <= kPointTailMaxIterations) S.alpha_hist[it - 1] = alpha;
      S.n_updates = it;
    }
  }
  if (fail) {
    if (threadIdx.x == 0) S.status = fail;
    return;
  }
  double q1 = 0, rr = 0, rz = 0, rn[PER], zv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * BLOCK;
    rn[k] = 0.0;
    if (i < n) {
      const double xv = xo[k] + alpha * pv[k];
      const double rv = ro[k] - alpha * qv[k];
      T.x[i] = xv; T.r[i] = rv;
      rn[k] = rv;
      lds[i] = rv;
      q1 -= xv * (bv[k] + rv);
      rr += rv * rv;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = threadIdx.x + k * BLOCK;
    zv[k] = 0.0;
    if (i < n) {
      const int c = i / 9;
      double t = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) t += mrow[k][j] * lds[9 * c + j];
      zv[k] = t;
      T.z[i] = t;
      rz += rn[k] * t;
    }
  }
  sum3(q1, rr, rz);
  const double Q1 = q1, rho_next = rz;
  const double norm_r = sqrt(rr);
  const double zeta = it * (Q1 - Q0) / Q1;
  int status = kCgRunning;
  if (zeta < q_tol && it >= min_it) status = kCgConvergedZeta;
  else if (norm_r <= tol_r && it >= min_it) status = kCgConvergedResidual;
  else if (it >= max_it) status = kCgMaxIterations;
  int fail_dir = 0;
  double beta = 0.0;
  if (status == kCgRunning) {
    auto zero_or_inf = [](double v) { return v == 0.0 || isinf(v); };
    if (zero_or_inf(rho_next)) fail_dir = kCgFailRho;
    else { beta = rho_next / rho; if (zero_or_inf(beta)) fail_dir = kCgFailBeta; }
    if (!fail_dir) {
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = threadIdx.x + k * BLOCK;
        if (i < n) T.p[i] = zv[k] + beta * pv[k];
      }
    }
  }
  if (threadIdx.x == 0) {
    S.Q1 = Q1; S.zeta = zeta; S.norm_r = norm_r;
    if (status == kCgConvergedZeta) { S.status = status; return; }   // Q0 keeps its value, as in the reference (:273-284)
    S.Q0 = Q1;
    S.Q0_pp[(it + 1) & 1] = Q1;
    if (status != kCgRunning) { S.status = status; return; }
    S.rho = rho; S.rho_new = rho_next; S.beta = beta;
    S.rho_pp[(it + 1) & 1] = rho_next;
    S.fail_dir = fail_dir;
    S.iter = it + 1;
  }
}

// One tile of a long point inside a ROUND (plan.cc): the kRoundWaves waves of the workgroup each hold one tile in registers, the waves
// [w0, w0 + cnt) of one point leave their tile sums in LDS (`red`, double-buffered by round parity: one barrier per round), every
// wave adds them up in the same order and finishes its own tile.  A point of up to 512 observations is read ONCE, a tile per wave in
// flight, where one wave walked the point's tiles twice with nothing in flight (process_long_point: 0.20 - 0.25 of the HBM peak on
// graphs of long tracks).  `word`: the wave's round word (kRoundIdle: no tile — every lane is invalid, the loads were issued anyway).
// A point of more than kRoundWaves tiles (flag != 0, the round is its own: waves [0, cnt0), cnt0 from the round's first word): in its
// kRoundSum rounds every wave adds the round's total to `carry`; its kRoundApply rounds finish the (L2-warm) tiles with that sum.
// JtJx has nothing to finish: its sum rounds do all the work, the last one stores y_e.
template <int MODE, bool LDS, bool CAP = false>
__device__ __forceinline__ void compute_long_round(const BalArgs& A, const Slot& s, int lane, const StreamAux& x, uint32_t word, uint32_t word0,
                                                   int flag, int wave, double (*red)[3], double (&carry)[3], Ctx& acc, double& dot) {
  const bool active = word != kRoundIdle;
  const int w0 = flag ? 0 : (active ? int((word >> 26) & 7u) : wave);
  const int cnt = flag ? int((word0 >> 29) & 7u) + 1 : (active ? int((word >> 29) & 7u) + 1 : 1);
  if constexpr (MODE == kSx || MODE == kSpseZ) {
    double t0, t1;
    f_times(s, acc, x.xc, t0, t1);
    double u[3] = {s.e[0] * t0 + s.e[3] * t1, s.e[1] * t0 + s.e[4] * t1, s.e[2] * t0 + s.e[5] * t1};
    if (!s.valid) { u[0] = u[1] = u[2] = 0; }
    const int pt = __builtin_amdgcn_readfirstlane(s.pt);   // one segment: every valid lane holds the point (an idle wave: unused)
    if (!(flag & kRoundApply)) {
      wave_allreduce<3>(u);
      if (lane == 0) { red[wave][0] = u[0]; red[wave][1] = u[1]; red[wave][2] = u[2]; }
    }
    __syncthreads();
    if (flag & kRoundApply) {
      u[0] = carry[0]; u[1] = carry[1]; u[2] = carry[2];
      if (flag & kRoundLast) { carry[0] = carry[1] = carry[2] = 0; }
    } else {
      u[0] = u[1] = u[2] = 0;
      for (int k = 0; k < cnt; ++k) { u[0] += red[w0 + k][0]; u[1] += red[w0 + k][1]; u[2] += red[w0 + k][2]; }
      if (flag & kRoundSum) {
        carry[0] += u[0]; carry[1] += u[1]; carry[2] += u[2];
        if constexpr (MODE == kSx && LDS) {   // the point's last sum round: its sum is complete, stored once by its first wave
          if (CAP && (flag & kRoundLast) && active && wave == w0 && lane == 0) store_point_capture(A.u_out, NE * pt, carry);
        }
        return;
      }
      if constexpr (MODE == kSx && LDS) {     // a point of up to kRoundWaves tiles: its first wave stores
        if (CAP && active && wave == w0 && lane == 0) store_point_capture(A.u_out, NE * pt, u);
      }
    }
    double v[3];
    sym_mul(x.ei, u, v);
    const double ev0 = s.e[0] * v[0] + s.e[1] * v[1] + s.e[2] * v[2];
    const double ev1 = s.e[3] * v[0] + s.e[4] * v[1] + s.e[5] * v[2];
    scatter_ft<LDS>(A, s, acc, MODE == kSx ? t0 - ev0 : ev0, MODE == kSx ? t1 - ev1 : ev1);
  } else {
    static_assert(MODE == kJtJx, "streaming modes");
    if (flag & kRoundApply) { __syncthreads(); return; }
    // issue_aux with one point: lanes 0..2 hold the point's x_e and D_e
    const double xp[3] = {shfl_idx(x.xa, 0), shfl_idx(x.xa, 1), shfl_idx(x.xa, 2)};
    double z0, z1;
    f_times(s, acc, x.xc, z0, z1);
    z0 += s.e[0] * xp[0] + s.e[1] * xp[1] + s.e[2] * xp[2];
    z1 += s.e[3] * xp[0] + s.e[4] * xp[1] + s.e[5] * xp[2];
    scatter_ft<LDS>(A, s, acc, z0, z1);
    double w[3] = {s.e[0] * z0 + s.e[3] * z1, s.e[1] * z0 + s.e[4] * z1, s.e[2] * z0 + s.e[5] * z1};
    if (!s.valid) { w[0] = w[1] = w[2] = 0; }
    wave_allreduce<3>(w);
    if (lane == 0) { red[wave][0] = w[0]; red[wave][1] = w[1]; red[wave][2] = w[2]; }
    __syncthreads();
    double t = 0;   // lane j < 3: component j of the point's sum
    if (lane < 3) {
      for (int k = 0; k < cnt; ++k) t += red[w0 + k][lane];
    }
    bool store = active && wave == w0 && lane < 3;   // the point's first wave stores y_e
    if (flag & kRoundSum) {
      const double c = (lane == 0 ? carry[0] : (lane == 1 ? carry[1] : carry[2])) + t;
      if (lane == 0) carry[0] = c; else if (lane == 1) carry[1] = c; else if (lane == 2) carry[2] = c;
      store = store && (flag & kRoundLast);
      t = c;
      if (flag & kRoundLast) { carry[0] = carry[1] = carry[2] = 0; }
    }
    if (store) {
      const double yv = t + x.da * x.da * x.xa;
      A.y_e[x.base + lane] = yv;
      dot += x.xa * yv;
    }
  }
}

template <int MODE, bool LDS, bool NT, bool F32 = false, bool CAP = false>   // CAP: the instantiation that keeps the points' sums (A.u_out set)
__global__ __launch_bounds__(512) void bal_stream_kernel(BalArgs A) {
  constexpr int BLOCK = 512;
  extern __shared__ double lds_acc[];
  if (A.status && *A.status != 0) return;
  Ctx acc;  // lds: every camera's accumulator row + the strip's entries (LDS), or the hybrid rows of this workgroup + one strip per wave (scatter_ft)
  ctx_init(A, acc, lds_acc);
  double* const xh = lds_acc + A.n_acc;   // LDS copy of x_f for the popular cameras (the CG tail's scratch reuses the space afterwards)
  {
    const int n_acc = LDS ? A.n_acc : NF * A.hyb_rows;
    for (int i = threadIdx.x; i < n_acc; i += BLOCK) acc.lds[i] = 0.0;
    if constexpr (LDS) {
      // four entries per thread and trip: the camera ids, then the four values, then the stores (two dependent round trips per trip
      // instead of per entry — the whole copy is nine entries per thread on the Venice shape)
      const int nx = NF * A.n_xhot;
      for (int i0 = threadIdx.x; i0 < nx; i0 += 4 * BLOCK) {
        int c[4];
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = i0 + j * BLOCK; c[j] = A.xhot_cam[(i < nx ? i : 0) / NF]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = i0 + j * BLOCK; v[j] = A.x_f[A.cam_base + NF * int64_t(c[j]) + (i < nx ? i : 0) % NF]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = i0 + j * BLOCK; if (i < nx) xh[i] = v[j]; }
      }
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  double dot = 0.0;  // kJtJx: this lane's share of x_e . y_e
  // grid-strided over [tile_begin, tile_end); hybrid accumulation: workgroup g owns the tiles of group g (plan.cc)
  const bool grouped = !LDS && A.grp_tile_ptr != nullptr;
  const int64_t nwaves = grouped ? BLOCK / 64 : int64_t(gridDim.x) * (BLOCK / 64);
  // wave-uniform by construction; readfirstlane tells the compiler, so that the tile words are
  // scalar loads and the branches on them scalar branches
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int range = grouped ? int(blockIdx.x) : 0;   // the hybrid group, or everything (plan.cc)
  const int64_t range_end = grouped ? A.grp_tile_ptr[blockIdx.x + 1] : (A.tile_end > 0 ? A.tile_end : A.n_tiles);
  // long points sit behind the normal tiles of their range (unless the ring is chunked): the pipeline ends where they begin
  const int64_t long_begin = A.long_behind ? int64_t(A.long_ptr[range]) : range_end;
  const int64_t tile_end = min(range_end, long_begin);
  const int64_t wave_first = (grouped ? 0 : logical_workgroup() * (BLOCK / 64)) + wave;
  const int64_t wave0 = (grouped ? int64_t(A.grp_tile_ptr[blockIdx.x]) : A.tile_begin) + wave_first;
  // The pipelined loop's walk.  Default: grid-strided (all workgroups stream through one region of memory together).  BLOCKED
  // (A.flags & 2, experiment: CERES_HIP_TILE_WALK=blocked): workgroup b takes the tiles [b C, (b + 1) C), its waves in turn — the
  // point-space range a workgroup writes (JtJx's y_e) is then one contiguous run.
  const bool blocked = !grouped && (A.flags & 2) != 0;
  const int64_t chunk = blocked ? ((tile_end - A.tile_begin + gridDim.x - 1) / gridDim.x + 7) / 8 * 8 : 0;
  const int64_t pipe_end = blocked ? min(tile_end, A.tile_begin + (logical_workgroup() + 1) * chunk) : tile_end;
  const int64_t pipe0 = blocked ? A.tile_begin + logical_workgroup() * chunk + wave : wave0;
  const int64_t pstep = blocked ? BLOCK / 64 : nwaves;
  const int64_t last = pipe_end - 1;
#if CERES_HIP_AB_PIPE_DEPTH >= 2
  if (pipe0 < pipe_end) {
    // THREE register sets in rotation (round 5, an EXPERIMENT kept as an A/B switch): while tile k is computed, the loads of tiles
    // k + 1 AND k + 2 are in flight.  The SQ counters show a wave spending 9.8 k cycles per tile, 1.5 k of them issuing
    // (profiles/r05k_*), which read like "not enough bytes in flight".  Measured (profiles/r05l_pipeline_depth_ab.txt): fp64 0.245 vs
    // 0.183 ms — at two waves per SIMD a wave owns 256 registers of the unified file, the third set does not fit and goes to scratch —
    // and fp32 tiles, where it does fit, 0.134 vs 0.131 ms.  The pass is not bound by its outstanding requests; what it was waiting
    // for were the popular cameras' lines of x (take_hot_x).
    Slot sa, sb, sc;
    StreamAux xa, xb, xc;
    SlotIdx i0, i1, i2;
    int64_t tile = pipe0;
    const int64_t t1 = min(tile + pstep, last), t2 = min(tile + 2 * pstep, last);
    int kind_a = A.tile_kind[tile], aux_a = A.tile_aux[tile], kind_b = A.tile_kind[t1], aux_b = A.tile_aux[t1], kind_c = 2, aux_c = 0;
    issue_idx(A, tile, lane, i0);
    __builtin_amdgcn_sched_barrier(0);
    issue_idx(A, t1, lane, i2);
    __builtin_amdgcn_sched_barrier(0);
    issue_idx(A, t2, lane, i1);
    __builtin_amdgcn_sched_barrier(0);
    issue_pairs<NT, F32>(A, tile, lane, sa);
    __builtin_amdgcn_sched_barrier(0);
    sa.cam = i0.cam; sa.seg = i0.seg;
    finish_slot(sa, lane, A.tile_pt0[tile]);
    issue_aux<MODE>(A, sa, lane, kind_a == 0 ? aux_a >> 8 : 0, xa);
    __builtin_amdgcn_sched_barrier(0);
    issue_pairs<NT, F32>(A, t1, lane, sb);
    __builtin_amdgcn_sched_barrier(0);
    sb.cam = i2.cam; sb.seg = i2.seg;
    finish_slot(sb, lane, A.tile_pt0[t1]);
    issue_aux<MODE>(A, sb, lane, kind_b == 0 ? aux_b >> 8 : 0, xb);
    __builtin_amdgcn_sched_barrier(0);
    bool more = true;
    // one stage: everything of tile k + 2 is issued into the set tile k - 1 left (index words of k + 3 with it), then tile k is computed
    auto stage = [&](Slot& c, StreamAux& cx, int ckind, int caux, Slot& f, StreamAux& fx, int& fkind, int& faux) {
      const int64_t far = min(tile + 2 * pstep, last);   // past the end: re-issue, the load count stays the same
      more = tile + pstep < pipe_end;
      fkind = A.tile_kind[far];
      faux = A.tile_aux[far];
      issue_idx(A, min(far + pstep, last), lane, i2);
      __builtin_amdgcn_sched_barrier(0);
      issue_pairs<NT, F32>(A, far, lane, f);
      __builtin_amdgcn_sched_barrier(0);
      f.cam = i1.cam; f.seg = i1.seg;
      finish_slot(f, lane, A.tile_pt0[far]);
      issue_aux<MODE>(A, f, lane, fkind == 0 ? faux >> 8 : 0, fx);
      __builtin_amdgcn_sched_barrier(0);
      if (ckind != 0) c.valid = false;  // long points are handled below; their seg words carry no store bits
      widen_slot<F32>(c);
      if constexpr (LDS) take_hot_x(A, c, xh, cx);
      compute_stream<MODE, LDS, CAP ? 1 : 2>(A, c, lane, caux & 0xff, ckind == 0 ? caux >> 8 : 0, cx, acc, dot);
      __builtin_amdgcn_sched_barrier(0);
      i1 = i2;
      tile = min(tile + pstep, last);
    };
    while (true) {
      stage(sa, xa, kind_a, aux_a, sc, xc, kind_c, aux_c);
      if (!more) break;
      stage(sb, xb, kind_b, aux_b, sa, xa, kind_a, aux_a);
      if (!more) break;
      stage(sc, xc, kind_c, aux_c, sb, xb, kind_b, aux_b);
      if (!more) break;
    }
  }
#else
  if (pipe0 < pipe_end) {
    // Two register sets in ping-pong: copying "next" into "current" would need the loaded
    // values to have arrived, which is exactly the wait this kernel exists to avoid.  (The
    // three index words are the exception: they are copied a stage after they were issued.)
    Slot sa, sb;
    StreamAux xa, xb;
    SlotIdx i1, i2;
    int64_t tile = pipe0;
    int kind_a = A.tile_kind[tile], aux_a = A.tile_aux[tile], kind_b = 2, aux_b = 0;
    // prologue in the steady-state issue order: index words (1), pairs (0), aux (0)
    issue_idx(A, tile, lane, i2);
    __builtin_amdgcn_sched_barrier(0);
    issue_idx(A, min(tile + pstep, last), lane, i1);
    __builtin_amdgcn_sched_barrier(0);
    issue_pairs<NT, F32>(A, tile, lane, sa);
    __builtin_amdgcn_sched_barrier(0);
    sa.cam = i2.cam; sa.seg = i2.seg;
    finish_slot(sa, lane, A.tile_pt0[tile]);
    issue_aux<MODE>(A, sa, lane, kind_a == 0 ? aux_a >> 8 : 0, xa);
    __builtin_amdgcn_sched_barrier(0);
    bool more = true;
    // one pipeline stage: everything of the next tile is issued, then this one is computed from `c`
    auto stage = [&](Slot& c, StreamAux& cx, int ckind, int caux, Slot& n, StreamAux& nx, int& nkind, int& naux) {
      const int64_t next = min(tile + pstep, last);  // past the end: re-issue, the load count stays the same
      more = tile + pstep < pipe_end;
#if CERES_HIP_AB_ABLATE & 16
      nkind = 0;
      naux = (13 << 8) | 8;
      const int npt0 = int(next) * 13;
#else
      nkind = A.tile_kind[next];
      naux = A.tile_aux[next];
      const int npt0 = A.tile_pt0[next];
#endif
      issue_idx(A, min(next + pstep, last), lane, i2);
      __builtin_amdgcn_sched_barrier(0);
      issue_pairs<NT, F32>(A, next, lane, n);
      __builtin_amdgcn_sched_barrier(0);
      n.cam = i1.cam; n.seg = i1.seg;
      finish_slot(n, lane, npt0);
      issue_aux<MODE>(A, n, lane, nkind == 0 ? naux >> 8 : 0, nx);
      __builtin_amdgcn_sched_barrier(0);
      if (ckind != 0) c.valid = false;  // long points are handled below; their seg words carry no store bits
      widen_slot<F32>(c);
      if constexpr (LDS) take_hot_x(A, c, xh, cx);
      compute_stream<MODE, LDS, CAP ? 1 : 2>(A, c, lane, caux & 0xff, ckind == 0 ? caux >> 8 : 0, cx, acc, dot);
      __builtin_amdgcn_sched_barrier(0);
      i1 = i2;
      tile = next;
    };
    while (true) {
      stage(sa, xa, kind_a, aux_a, sb, xb, kind_b, aux_b);
      if (!more) break;
      stage(sb, xb, kind_b, aux_b, sa, xa, kind_a, aux_a);
      if (!more) break;
    }
  }
#endif
  // Points with more than 64 observations own whole tiles (kind 3 / 1 = head, 2 = continuation).  Those of up to kRoundWaves
  // tiles (kind 3) are taken in ROUNDS, one tile per wave, with the same one-stage-ahead pipeline as above.
  __shared__ double round_red[2][kRoundWaves][3];
  if (A.round_word) {
    // this workgroup's SEQUENCES of rounds (plan.cc): one packed round, or all rounds of one point of more than kRoundWaves tiles
    const int64_t qe = grouped ? int64_t(A.round_ptr[range + 1]) : int64_t(A.n_seq);
    const int64_t qstride = grouped ? 1 : int64_t(gridDim.x);
    int64_t it_q = grouped ? int64_t(A.round_ptr[range]) : logical_workgroup();
    if (it_q < qe) {   // (workgroup-uniform: the rounds have barriers)
      // (a hybrid group's sequences are all its workgroup's: one run of rounds, no table look-up on the way)
      int64_t it_r = A.seq_ptr[it_q], it_end = A.seq_ptr[grouped ? qe : it_q + 1];
      if (grouped) it_q = qe - 1;
      bool it_real = true;
      // the iterator's round, then one step on; past the end it keeps returning the last round (same load count on every path)
      auto next_round = [&](bool* real) {
        const int64_t r = it_r;
        *real = it_real;
        if (it_real) {
          if (it_r + 1 < it_end) ++it_r;
          else if (it_q + qstride < qe) { it_q += qstride; it_r = A.seq_ptr[it_q]; it_end = A.seq_ptr[it_q + 1]; }
          else it_real = false;
        }
        return r;
      };
      Slot sa, sb;
      StreamAux xa, xb;
      SlotIdx i1, i2;
      double carry[3] = {0, 0, 0};
      // an idle wave issues the loads of the round's first tile, with every lane invalid
      auto word_at = [&](int64_t r) { return A.round_word[r * kRoundWaves + wave]; };
      auto tile_at = [&](int64_t r, uint32_t w) { return int64_t((w != kRoundIdle ? w : A.round_word[r * kRoundWaves]) & 0x3FFFFFFu); };
      auto finish = [&](Slot& c, const SlotIdx& i, int64_t tile, uint32_t w) {
        c.cam = i.cam; c.seg = i.seg;
        finish_slot(c, lane, A.tile_pt0[tile]);
        if (w == kRoundIdle) { c.valid = false; c.nocam = false; c.cam = 0; c.pt = 0; c.acc = kSlotSpill; }
      };
      bool real_c, real_n, real_nn;
      int64_t rc = next_round(&real_c), rn = next_round(&real_n);
      uint32_t wa = word_at(rc), wb = kRoundIdle;
      // the round's first word and flag travel with the pipeline (scalar loads a stage ahead of their use)
      uint32_t w0a = A.round_word[rc * kRoundWaves], w0b = kRoundIdle;
      int fa = A.round_flag[rc], fb = 0;
      int par = 0;
      {
        const int64_t tile = tile_at(rc, wa);
        issue_idx(A, tile, lane, i2);
        __builtin_amdgcn_sched_barrier(0);
        issue_idx(A, tile_at(rn, word_at(rn)), lane, i1);
        __builtin_amdgcn_sched_barrier(0);
        issue_pairs<NT, F32>(A, tile, lane, sa);
        __builtin_amdgcn_sched_barrier(0);
        finish(sa, i2, tile, wa);
        issue_aux<MODE>(A, sa, lane, 1, xa);
        __builtin_amdgcn_sched_barrier(0);
      }
      auto stage = [&](Slot& c, StreamAux& cx, uint32_t cw, uint32_t cw0, int cf, Slot& n, StreamAux& nx, uint32_t& nw, uint32_t& nw0, int& nf) {
        const int64_t rnn = next_round(&real_nn);
        nw = word_at(rn);
        nw0 = A.round_word[rn * kRoundWaves];
        nf = A.round_flag[rn];
        const int64_t next = int64_t((nw != kRoundIdle ? nw : nw0) & 0x3FFFFFFu);
        issue_idx(A, tile_at(rnn, word_at(rnn)), lane, i2);
        __builtin_amdgcn_sched_barrier(0);
        issue_pairs<NT, F32>(A, next, lane, n);
        __builtin_amdgcn_sched_barrier(0);
        finish(n, i1, next, nw);
        issue_aux<MODE>(A, n, lane, 1, nx);
        __builtin_amdgcn_sched_barrier(0);
        widen_slot<F32>(c);
        if constexpr (LDS) take_hot_x(A, c, xh, cx);
        compute_long_round<MODE, LDS, CAP>(A, c, lane, cx, cw, cw0, cf, wave, round_red[par], carry, acc, dot);
        __builtin_amdgcn_sched_barrier(0);
        par ^= 1;
        i1 = i2;
        rc = rn; real_c = real_n;
        rn = rnn; real_n = real_nn;
      };
      while (true) {
        stage(sa, xa, wa, w0a, fa, sb, xb, wb, w0b, fb);
        if (!real_c) break;
        stage(sb, xb, wb, w0b, fb, sa, xa, wa, w0a, fa);
        if (!real_c) break;
      }
    }
  }
  // Long points outside the rounds (kind 1: the ring is chunked — they sit among the normal tiles then — or the plan has more
  // tiles than a round word holds): one wave per point, two sweeps (process_long_point).
  for (int64_t tile = (A.long_behind ? long_begin + wave_first : wave0); tile < range_end; tile += nwaves) {
    if (A.tile_kind[tile] == 1) process_long_point<MODE, LDS, F32>(A, tile, A.tile_aux[tile], lane, acc, dot);
  }
  if (MODE == kJtJx && A.pq_out) {  // one partial of x_e . y_e per workgroup
    __shared__ double red[BLOCK / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if (lane == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0;
      for (int i = 0; i < BLOCK / 64; ++i) t += red[i];
      if (A.pq_accumulate) t += A.pq_out[blockIdx.x];
      A.pq_out[blockIdx.x] = t;
    }
  }
  if constexpr (LDS) {
    flush_shared_sums(A, acc);
    __syncthreads();
    double* out = A.partials + int64_t(blockIdx.x) * A.n_acc;
    const bool tail = kHasCgTail && MODE == kSx && A.tail.enabled;   // (launch-uniform)
    if (!tail) {
      for (int i = threadIdx.x; i < A.n_acc; i += BLOCK) out[i] = acc.lds[i];
    } else {
      // write-through stores (device scope): the partial sums must be readable from another XCD when the ticket is taken, and a
      // release fence instead — an L2 write-back per workgroup, queued behind those of the XCD's other workgroups — cost 12 us
      for (int i = threadIdx.x; i < A.n_acc; i += BLOCK) asm volatile("global_store_dwordx2 %0, %1, off sc1" : : "v"(out + i), "v"(acc.lds[i]) : "memory");
      asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    }
    if constexpr (MODE == kSx && kHasCgTail) {
      if (tail) {
        __shared__ int last;
        __syncthreads();      // the workgroup's partial sums are out ...
        if (threadIdx.x == 0) last = atomicAdd(A.tail.ticket, 1u) == gridDim.x - 1 ? 1 : 0;   // ... before its ticket is
        __syncthreads();
        if (last) {
          __threadfence();    // and every other workgroup's are in before they are read
          cg_iteration_tail<BLOCK>(A, acc.lds);
          if (threadIdx.x == 0) *A.tail.ticket = 0u;
        }
      }
    }
  } else {
    flush_shared_sums_global(A, acc);
    if (A.hyb_rows > 0) {  // this workgroup's accumulator rows join the spilled rows in the ring: the second pass sums both
      __syncthreads();
      double* out = A.zbuf + NF * (A.z_flush_row0 + int64_t(blockIdx.x) * A.hyb_rows);
      for (int i = threadIdx.x; i < NF * A.hyb_rows; i += BLOCK) out[i] = acc.lds[i];
    }
  }
}

#endif   // CERES_HIP_PIPELINED

// y_f[pos(i)] = sum over workgroup partials (+ D_f^2 x_f).  One thread per F scalar.
// Workgroup = 64 consecutive scalars x 8 waves, wave w sums partials w, w+8, w+16, ...; the eight
// wave sums are combined through LDS in a fixed order (deterministic).  A workgroup takes every
// gridDim.x-th group of 64 scalars.  pq_out: also the partial inner product x_f . y_f of the scalars this
// workgroup finished (CG's p.q, camera part: x_f and the finished y_f are both in registers here).
// accumulator entry i (camera c = i / NF, scalar i % NF; behind the cameras: the strip) -> its place in the F-space vectors
__device__ __forceinline__ int f_position(const FMap& m, int i) {
  if (NS > 0 && i >= m.n_cam_scalars) return m.sh_pos[i - m.n_cam_scalars];   // (-1: a padding entry of the strip)
  return m.cam_pos ? m.cam_pos[i / NF] + i % NF : m.cam_base + i;
}

__global__ __launch_bounds__(512) void bal_reduce_partials_kernel(const double* __restrict__ partials, int nparts, int n_f9,
                                           FMap map, const double* __restrict__ D_f,
                                           const double* __restrict__ x_f, double* __restrict__ y_f,
                                           const int* __restrict__ status, double* __restrict__ pq_out,
                                           const double* __restrict__ sum_in, int n_sum_in, double* __restrict__ sum_out) {
  __shared__ double sh[8][64];
  if (status && *status != 0) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // sharded CGNR: this rank's point-space share of p.q (the tile pass's per-workgroup partials) collapsed into ONE double that
  // travels with the camera vector through the same all-reduce (sum_out = the element after the vector); fixed order
  if (sum_out && blockIdx.x == gridDim.x - 1 && wv == 7) {
    double v = 0;
    for (int k = lane; k < n_sum_in; k += 64) v += sum_in[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) *sum_out = v;
  }
  const int ngroups = (n_f9 + 63) / 64;
  double dot = 0;
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int i = g * 64 + lane;
    double s0 = 0, s1 = 0;
    if (i < n_f9) {
      // sixteen rows per trip, all requested before the first is added (round 5: one memory round trip per 16 rows instead of per
      // pair — 32 MB of partial sums on the Venice shape, 10 us as a chain of sixteen trips); the order of the additions is the old one
      int w = wv;
      for (; w + 120 < nparts; w += 128) {
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = partials[int64_t(w + 8 * j) * n_f9 + i];
#pragma unroll
        for (int j = 0; j < 16; j += 2) { s0 += v[j]; s1 += v[j + 1]; }
      }
      for (; w + 8 < nparts; w += 16) {
        s0 += partials[int64_t(w) * n_f9 + i];
        s1 += partials[int64_t(w + 8) * n_f9 + i];
      }
      if (w < nparts) s0 += partials[int64_t(w) * n_f9 + i];
    }
    sh[wv][lane] = s0 + s1;
    __syncthreads();
    if (wv == 0 && i < n_f9) {
      double s = ((sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane])) + ((sh[4][lane] + sh[5][lane]) + (sh[6][lane] + sh[7][lane]));
      const int o = f_position(map, i);
      if (o >= 0) {
        if (D_f) { const double d = D_f[o]; s += d * d * x_f[o]; }
        y_f[o] = s;
        if (pq_out) dot += x_f[o] * s;
      }
    }
    __syncthreads();  // sh is reused by the next group
  }
  if (pq_out && wv == 0) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if (lane == 0) pq_out[blockIdx.x] = dot;
  }
}

// bal_reduce_partials_kernel for a SHARDED instance, with the sum over ranks inside (p2p.h): the workgroup adds up its groups of 64
// F-space POSITIONS over this rank's workgroup partials (same order as above), then every wave takes every eighth of those groups
// through the exchange — push to every rank, flags, wait, add the ranks' slots in rank order — and finishes them: + D_f^2 x_f, y_f,
// the partial x_f . y_f.  One launch for what was the reduction, the all-reduce kernel and bal_add_f_diagonal_kernel (8 + 28..46 + 5 us
// of one rank's eighth of a Venice-sized S.x whose tile pass takes 30; profiles/r06a_*).  Slot index = position in the F-space vector,
// chunk index = position / 64: the numbering of the stand-alone all-reduce of that vector (kernels_cg.hip), so that ranks which cannot
// take this kernel (rows outside their tiles to add first) still meet the others in the same slots.  sum_out (CGNR: the shard's
// point-space share of p.q) rides as position n_fv.  Needs cameras back to back in F space (map.cam_pos == nullptr).  A non-zero CG
// status word skips the arithmetic, never the handshake (p2p.h).
constexpr int kRxBatch = 16;   // groups a workgroup sums before it exchanges them
__device__ __forceinline__ int acc_of_position(const FMap& m, int o) {   // inverse of f_position for back-to-back cameras; -1: no accumulator
  const int i = o - m.cam_base;
  if (i >= 0 && i < m.n_cam_scalars) return i;
  if (NS > 0) {
#pragma unroll
    for (int j = 0; j < (NS > 0 ? NS : 1); ++j) if (m.sh_pos[j] == o) return m.n_cam_scalars + j;
  }
  return -1;
}
__global__ __launch_bounds__(512) void bal_reduce_exchange_kernel(const double* __restrict__ partials, int nparts, int n_f9, int n_fv,
                                           FMap map, const double* __restrict__ D_f,
                                           const double* __restrict__ x_f, double* __restrict__ y_f,
                                           const int* __restrict__ status, double* __restrict__ pq_out,
                                           const double* __restrict__ sum_in, int n_sum_in, double* __restrict__ sum_out, P2pComm C) {
  __shared__ double sh[8][64];
  __shared__ double res[kRxBatch][64];
  __shared__ double dots[8];
  __shared__ double extra_v;
  const bool skip = status && *status != 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_total = n_fv + (sum_out ? 1 : 0);
  const int ngroups = (n_total + 63) / 64;
  if (sum_out && int(blockIdx.x) == (n_fv / 64) % int(gridDim.x) && wv == 7) {   // the workgroup that owns position n_fv
    double v = 0;
    if (!skip) for (int k = lane; k < n_sum_in; k += 64) v += sum_in[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) extra_v = v;
  }
  __syncthreads();
  double dot = 0;
  for (int g0 = blockIdx.x; g0 < ngroups; g0 += kRxBatch * gridDim.x) {
    int nb = 0;
    for (int g = g0; g < ngroups && nb < kRxBatch; g += gridDim.x, ++nb) {
      const int o = g * 64 + lane;
      const int i = o < n_fv ? acc_of_position(map, o) : -1;
      double s0 = 0, s1 = 0;
      if (i >= 0 && !skip) {
        int w = wv;
        for (; w + 120 < nparts; w += 128) {
          double v[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = partials[int64_t(w + 8 * j) * n_f9 + i];
#pragma unroll
          for (int j = 0; j < 16; j += 2) { s0 += v[j]; s1 += v[j + 1]; }
        }
        for (; w + 8 < nparts; w += 16) {
          s0 += partials[int64_t(w) * n_f9 + i];
          s1 += partials[int64_t(w + 8) * n_f9 + i];
        }
        if (w < nparts) s0 += partials[int64_t(w) * n_f9 + i];
      }
      sh[wv][lane] = s0 + s1;
      __syncthreads();
      if (wv == 0) {
        double t = ((sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane])) + ((sh[4][lane] + sh[5][lane]) + (sh[6][lane] + sh[7][lane]));
        if (sum_out && o == n_fv) t = extra_v;
        res[nb][lane] = t;
      }
      __syncthreads();
    }
    for (int k = wv; k < nb; k += 8) {   // no barrier in here: the waves wait for their peers independently
      const int g = g0 + k * int(gridDim.x);
      const int o = g * 64 + lane;
      const bool act = o < n_total;
      double sv = p2p_exchange_wave(C, g, o, act, act ? res[k][lane] : 0.0);
      if (act && !skip) {
        if (o == n_fv) *sum_out = sv;
        else if (acc_of_position(map, o) >= 0) {
          if (D_f) { const double d = D_f[o]; sv += d * d * x_f[o]; }
          y_f[o] = sv;
          if (pq_out) dot += x_f[o] * sv;
        }
      }
    }
    __syncthreads();   // res is reused by the next batch
  }
  if (pq_out) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if (lane == 0) dots[wv] = dot;
    __syncthreads();
    if (threadIdx.x == 0) pq_out[blockIdx.x] = ((dots[0] + dots[1]) + (dots[2] + dots[3])) + ((dots[4] + dots[5]) + (dots[6] + dots[7]));
  }
}

// HBM read-stream probe: the same tile walk and 16-byte-per-lane loads as the fused kernels,
// nothing else (one double per workgroup written).  Gives the ceiling the fused kernels are
// measured against next to the 8 TB/s datasheet figure.
__global__ __launch_bounds__(1024) void bal_stream_probe_kernel(const double2* __restrict__ J, int64_t n_tiles, double* __restrict__ out) {
  __shared__ double sh[16];
  const int lane = threadIdx.x & 63;
  const int64_t wave = int64_t(blockIdx.x) * 16 + (threadIdx.x >> 6), nwaves = int64_t(gridDim.x) * 16;
  double acc = 0;
  for (int64_t tile = wave; tile < n_tiles; tile += nwaves) {
    const double2* p = J + tile * kTilePitch + lane;
    double2 v[kPairs];
#pragma unroll
    for (int j = 0; j < kPairs; ++j) v[j] = p[j * kTile];
#pragma unroll
    for (int j = 0; j < kPairs; ++j) acc += v[j].x + v[j].y;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if (lane == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0; for (int i = 0; i < 16; ++i) s += sh[i]; out[blockIdx.x] = s; }
}


// y_f += D_f^2 x_f over the camera scalars (after an all-reduce of the raw sums); pq_out: partial x_f . y_f per workgroup.
__global__ __launch_bounds__(256) void bal_add_f_diagonal_kernel(int n_f9, FMap map, const double* __restrict__ D_f,
                                          const double* __restrict__ x_f, double* __restrict__ y_f,
                                          const int* __restrict__ status, double* __restrict__ pq_out) {
  __shared__ double red[4];
  if (status && *status != 0) return;
  double dot = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_f9; i += gridDim.x * 256) {
    const int o = f_position(map, i);
    if (o < 0) continue;
    double y = y_f[o];
    if (D_f) { const double d = D_f[o]; y += d * d * x_f[o]; y_f[o] = y; }
    if (pq_out) dot += x_f[o] * y;
  }
  if (pq_out) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) pq_out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// Re-layout: caller's values (any cell.position) -> tiles.  One wavefront per tile.  (The stand-alone form of what the first pass
// of a step does on the way: A.src_values / src_b, the slot_* lists and J_out / Jf_out / b_out as use_gather_if_unpacked sets them.)
template <bool F32>
__global__ __launch_bounds__(256) void bal_pack_kernel(BalArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (tile >= A.n_tiles) return;
  const int64_t sl = tile * kTile + lane;
  const int ep = A.slot_epos[sl];
  double v[2 * kPairs];
  gather_values(A, sl, ep, v, ep >= 0 ? A.slot_fpos[sl] : -1);
  double bv[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) bv[r] = 0.0;
  if (ep >= 0 && A.src_b) {
    const int bp = A.slot_bpos[sl];
#pragma unroll
    for (int r = 0; r < NR; ++r) bv[r] = A.src_b[bp + r];
  }
  if constexpr (F32) {
    float4* o = A.Jf_out + tile * (6 * kTile) + lane;
#pragma unroll
    for (int q = 0; q < 6; ++q) tile_store(o + q * kTile, make_float4(float(v[4 * q]), float(v[4 * q + 1]), float(v[4 * q + 2]), float(v[4 * q + 3])), (A.flags & 4) != 0);
  } else {
    double2* o = A.J_out + tile * kTilePitch + lane;
#pragma unroll
    for (int j = 0; j < kPairs; ++j) tile_store(o + j * kTile, make_double2(v[2 * j], v[2 * j + 1]), (A.flags & 4) != 0);
  }
  if (A.src_b) store_b(A.b_out, tile, lane, bv);
}

// ---- camera-major passes ---------------------------------------------------------------
// Unit of work = ITEM: at most kCamChunk consecutive observations of ONE camera in the
// camera-major list (plan.cc); camera degrees are heavily skewed, so heavy cameras are split.
// One WAVEFRONT per item (4 items per workgroup): lanes stride over the item's observations,
// gather F from the caller-layout values (144 contiguous bytes per observation) and reduce
// with __shfl_xor.  A camera covered by a single item is stored directly; split cameras are
// combined with global_atomic_add_f64 into a zeroed output (rounding-level order effects
// only there).

// Per-camera 9x9 blocks: sum of F^T M F, with M = I (JACOBI: block diagonal of F^T F) or M = I - E (E^T E)^-1 E^T read
// from [slot][4] (SCHUR_JACOBI: the diagonal blocks SchurEliminator::Eliminate writes into a block-diagonal lhs).
// Every ITEM leaves its 45 upper-triangle sums (and, SCHUR, the 9 column square sums of F) in parts[item][kCamPart]:
// no atomics, no zeroed output, and the per-camera combination (bal_camera_finish_kernel, or the load phase of
// bal_invert9_kernel) adds the items of a camera in a fixed order — bit-reproducible.  The first version combined split
// cameras with global fp64 atomics: 81 per item, which on a problem with few cameras (Dubrovnik: 16) or small items
// (Ladybug) cost several times the pass itself (55 / 105 us, profiles/r02b_kernel_stats_*).
// Loads: every lane reads "its" 144-byte cell (18 loads of 8 bytes, all issued before the first use).  A naive lane-per-cell
// gather LOOP with half a million lanes in flight (tools/probes/gather_probe.hip) fetches 3-5x its useful bytes by FETCH_SIZE,
// whatever the order of the cells (profiles/r02l_gather_probe_fetch_size_calibration.txt); this kernel's few, register-heavy
// waves stay near 2.2x (1.9 GB for 0.88 GB of F and M_o on the Venice shape).  Measured, no effect (r02af): nine 16-byte loads per
// cell instead of eighteen 8-byte ones.  Measured SLOWER (r02ae, 0.46 vs 0.33 ms): forming M_o here from the E cell and the point's
// packed inverse instead of reading the M_o record (it saves kInit 0.034 ms of writes and costs this pass 0.13 ms).
// Tried and measured SLOWER (r02m, 0.65 vs 0.37 ms on the Venice shape): cooperative loading, nine lanes x 16 bytes
// per cell into an LDS strip and each lane picking its observation up from there — one line request per line, but load ->
// LDS -> compute serialise inside an iteration and the wave count drops with the 36 KB of LDS per workgroup.
template <bool SCHUR>
__global__ __launch_bounds__(256) void bal_camera_items_kernel(const double* __restrict__ values, CamItems items,
                                                               const int32_t* __restrict__ cam_fpos,
                                                               const int32_t* __restrict__ cam_slot,
                                                               const double* __restrict__ Mo, double* __restrict__ parts) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= items.count) return;
  const int beg = items.begin[item], end = items.end[item];
  double acc[kTri], sq[NF];
#pragma unroll
  for (int i = 0; i < kTri; ++i) acc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NF; ++i) sq[i] = 0.0;
  for (int q = beg + lane; q < end; q += 64) {
    const double* f = values + cam_fpos[q];
    double fr[NR][NF];   // the observation's camera cell, row by row
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
      for (int k = 0; k < NF; ++k) fr[r][k] = f[r * NF + k];
    }
    double m[kMoPitch];   // M_o, packed upper triangle (the identity for F^T F)
#pragma unroll
    for (int i = 0; i < kMoPitch; ++i) m[i] = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) m[tri_r(r, r)] = 1.0;
    if constexpr (SCHUR) {
      const double2* mo = reinterpret_cast<const double2*>(Mo + kMoPitch * int64_t(cam_slot[q]));
      // plain loads: non-temporal ones (no L1) made this pass 8 % slower (r02y)
#pragma unroll
      for (int i = 0; i < kMoPitch / 2; ++i) { const double2 a = mo[i]; m[2 * i] = a.x; m[2 * i + 1] = a.y; }
#pragma unroll
      for (int k = 0; k < NF; ++k) {   // column norms of the camera columns (the blocks hold F^T M F, not F^T F)
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) t += fr[r][k] * fr[r][k];
        sq[k] += t;
      }
    }
    int idx = 0;
#pragma unroll
    for (int a = 0; a < NF; ++a) {
      double g[NR];   // row a of (F^T M)
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < NR; ++u) t += m[u <= r ? tri_r(u, r) : tri_r(r, u)] * fr[u][a];
        g[r] = t;
      }
#pragma unroll
      for (int bb = a; bb < NF; ++bb) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) t += g[r] * fr[r][bb];
        acc[idx++] += t;
      }
    }
  }
  double* out = parts + int64_t(item) * kCamPart;
  static_assert(kCamPart <= 80, "one lane per entry is not required, but the stores below assume it fits two rounds");
#pragma unroll
  for (int i = 0; i < kTri; ++i) {
    double v = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == (i & 63)) out[i] = v;   // every lane holds every sum; lane i stores entry i: contiguous bytes per item
  }
  if constexpr (SCHUR) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      double v = sq[k];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      if (lane == ((kTri + k) & 63)) out[kTri + k] = v;
    }
  }
}

#if CERES_HIP_IS_BAL_SHAPE
// The same sums with the F cells EVALUATED (round 4; ceres_hip_bal_minimize): an item's lanes share the camera, so its record is a
// scalar load, and what a lane fetches per observation is its point's record (48 bytes of a 48 MB array the tile-order evaluator just
// wrote: on die), the pixel and the point index from camera-major lists (20 bytes, coalesced) and M_o — instead of a 144-byte cell
// of a 720 MB stream at 2.3x its size in line fetches (design/03: the over-fetch this pass could not shed while F came from memory).
// The evaluator then writes NO caller-layout copy of the Jacobian at all.
// ROBUST: the F cells are corrected by items.ev_loss before the column scaling, as the tile-order evaluator corrects its own
// (robust_loss.h) — the blocks are then those of the Jacobian the solver holds.
template <bool SCHUR, bool ROBUST>
__global__ __launch_bounds__(256) void bal_camera_items_eval_kernel(CamItems items, const int32_t* __restrict__ cam_slot,
                                                                    const double* __restrict__ Mo, double* __restrict__ parts) {
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (item >= items.count) return;
  const int beg = items.begin[item], end = items.end[item];
  const double2* cp = reinterpret_cast<const double2*>(items.ev_cam_pack + 18 * int64_t(items.cam[item]));
  double cr[18];
#pragma unroll
  for (int i = 0; i < 9; ++i) { const double2 v = cp[i]; cr[2 * i] = v.x; cr[2 * i + 1] = v.y; }
  const double cam9[9] = {cr[0], cr[1], cr[2], cr[3], cr[4], cr[5], cr[6], cr[7], cr[8]};
  double acc[kTri], sq[NF];
#pragma unroll
  for (int i = 0; i < kTri; ++i) acc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NF; ++i) sq[i] = 0.0;
  for (int q = beg + lane; q < end; q += 64) {
    const double2* pp = reinterpret_cast<const double2*>(items.ev_pt_pack + 6 * int64_t(items.ev_pt[q]));
    const double2 o = items.ev_obs[q], p0 = pp[0], p1 = pp[1];
    const double X3[3] = {p0.x, p0.y, p1.x};
    double res[2], jc[18], jp[6];
    snavely<true>(cam9, X3, o.x, o.y, res, jc, jp);
    if constexpr (ROBUST) {
      const double sq = res[0] * res[0] + res[1] * res[1];
      double rho[3];
      robust_rho(items.ev_loss, sq, rho);
      robust_correct_jacobian<9>(robust_corrector(sq, rho), res[0], res[1], jc);
    }
    double f0[NF], f1[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) { f0[k] = jc[k] * cr[9 + k]; f1[k] = jc[9 + k] * cr[9 + k]; }
    double m00 = 1.0, m01 = 0.0, m11 = 1.0;
    if constexpr (SCHUR) {
      const double2* mo = reinterpret_cast<const double2*>(Mo + 4 * int64_t(cam_slot[q]));
      const double2 a = mo[0], b = mo[1];
      m00 = a.x; m01 = a.y; m11 = b.x;
#pragma unroll
      for (int k = 0; k < NF; ++k) sq[k] += f0[k] * f0[k] + f1[k] * f1[k];
    }
    int idx = 0;
#pragma unroll
    for (int a = 0; a < NF; ++a) {
      const double g0 = m00 * f0[a] + m01 * f1[a];
      const double g1 = m01 * f0[a] + m11 * f1[a];
#pragma unroll
      for (int bb = a; bb < NF; ++bb) acc[idx++] += g0 * f0[bb] + g1 * f1[bb];
    }
  }
  double* out = parts + int64_t(item) * kCamPart;
#pragma unroll
  for (int i = 0; i < kTri; ++i) {
    double v = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == (i & 63)) out[i] = v;
  }
  if constexpr (SCHUR) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      double v = sq[k];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
      if (lane == ((kTri + k) & 63)) out[kTri + k] = v;
    }
  }
}
#endif

// The same item sums on the matrix pipe: a camera's block IS a contraction, F^T (W F) with F the (2 n) x NF stack of the item's
// observations and W = diag(M_o) (SCHUR_JACOBI) or I.  One v_mfma_f64_16x16x4_f64 takes four rows = two observations: lane l holds
// column l & 15 (zero beyond NF) of row l >> 4, which is both its A operand (F^T[col][row]) and, after the 2 x 2 weight mixes it
// with the observation's other row (lane l ^ 16), its B operand ((W F)[row][col]).  Against the lane-per-observation form above:
// a load instruction reads whole rows of two records instead of one 8-byte word of 64 records (4 instead of 2 NF line
// look-ups per observation), and there is no wavefront reduction of the sums at the end — the sums ARE the accumulator, entry
// (a, b) in register a / 4 of lane 16 (a % 4) + b.  What short items (a camera of a video-like scene has tens of observations) and
// launch-bound shapes spent their time on.  LaunchBalCameraItems picks the kernel by the mean item length.
#if CERES_HIP_NR == 2   // (four rows of an instruction = two observations of two rows each; other row heights: the lane-per-observation kernel)
typedef double cam_v4f64 __attribute__((ext_vector_type(4)));
template <bool SCHUR>
__global__ __launch_bounds__(256) void bal_camera_items_mfma_kernel(const double* __restrict__ values, CamItems items,
                                                                    const int32_t* __restrict__ cam_fpos,
                                                                    const int32_t* __restrict__ cam_slot,
                                                                    const double* __restrict__ Mo, double* __restrict__ parts) {
  static_assert(NF <= 16, "one 16 x 16 accumulator tile");
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= items.count) return;
  const int beg = items.begin[item], end = items.end[item];
  const int col = lane & 15, kk = lane >> 4, ob = kk >> 1, r = kk & 1;
  const bool cv = col < NF;
  constexpr int U = 8;  // matrix instructions (pairs of observations) per iteration: their loads are all in flight together
  cam_v4f64 acc = cam_v4f64{0.0, 0.0, 0.0, 0.0}, acc1 = cam_v4f64{0.0, 0.0, 0.0, 0.0};   // two chains: the pipe need not wait for its own result
  double sq = 0.0;
  int fp[U], sl[U];
  auto load_idx = [&](int q0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + 2 * u + ob;
      const bool ok = q < end;
      fp[u] = ok ? cam_fpos[q] : -1;
      if constexpr (SCHUR) sl[u] = ok ? cam_slot[q] : 0;
    }
  };
  load_idx(beg);
  for (int q0 = beg; q0 < end; q0 += 2 * U) {
    double a[U], wd[U], wo[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a[u] = (fp[u] >= 0 && cv) ? values[fp[u] + NF * r + col] : 0.0;
      if constexpr (SCHUR) {
        // record [m00 m01 | m11 m01]: one 16-byte load gives row r its diagonal and off-diagonal weight
        const double2 m = *reinterpret_cast<const double2*>(Mo + 4 * int64_t(sl[u]) + 2 * r);
        wd[u] = m.x;
        wo[u] = m.y;
      }
    }
    load_idx(q0 + 2 * U);   // the next iteration's index words travel while this one computes
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double b = a[u];
      if constexpr (SCHUR) {
        const double other = __shfl_xor(a[u], 16, 64);   // the observation's other row, same column
        b = wd[u] * a[u] + wo[u] * other;
        sq += a[u] * a[u];
      }
      if (u & 1) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b, acc1, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b, acc, 0, 0, 0);
    }
  }
  acc += acc1;
  double* out = parts + int64_t(item) * kCamPart;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ra = kk + 4 * i;
    if (ra <= col && col < NF) out[tri_index(ra, col)] = acc[i];
  }
  if constexpr (SCHUR) {
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    if (kk == 0 && cv) out[kTri + col] = sq;
  }
}

#endif   // CERES_HIP_NR == 2

// Row `i` of camera c's block from the per-item partial sums (packed upper triangle: entry (a, b), a <= b, at tri_index(a, b)),
// items of a camera in list order; sqsum = the camera's column-i square sum (SCHUR items only).
__device__ __forceinline__ void gather_camera_row(const double* __restrict__ parts, int item_lo, int item_hi, int i, double (&row)[NF],
                                                  double& sqsum, bool want_sq) {
#pragma unroll
  for (int k = 0; k < NF; ++k) row[k] = 0.0;
  sqsum = 0.0;
  for (int it = item_lo; it < item_hi; ++it) {
    const double* p = parts + int64_t(it) * kCamPart;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int a = k < i ? k : i, b = k < i ? i : k;
      row[k] += p[tri_index(a, b)];
    }
    if (want_sq) sqsum += p[kTri + i];
  }
}

// blocks[c] = sum of the camera's items (full symmetric NF x NF) + D_f^2 on the diagonal if D_f != nullptr; camsq likewise.
// NF lanes per camera, kPerWave cameras per wavefront.  Used when the raw sums are needed in memory (sharded all-reduce,
// not_inverted read-back); otherwise bal_invert_kernel gathers the items itself.
__global__ __launch_bounds__(64) void bal_camera_finish_kernel(const double* __restrict__ parts, const int32_t* __restrict__ cam_item_ptr,
                                                               const double* __restrict__ D_f, const int32_t* __restrict__ cam_pos, int cam_base,
                                                               const int64_t* __restrict__ cam_diag_off, double* __restrict__ blocks,
                                                               double* __restrict__ camsq, int n_cameras, const double* __restrict__ extra) {
  const int lane = threadIdx.x;
  const int grp = lane / NF, i = lane - NF * grp;
  const int c = blockIdx.x * kPerWave + grp;
  if (grp >= kPerWave || c >= n_cameras) return;
  double row[NF], sqsum;
  gather_camera_row(parts, cam_item_ptr[c], cam_item_ptr[c + 1], i, row, sqsum, camsq != nullptr);
  if (extra) {  // rows outside the tiles (no point cell): their F^T F, whose diagonal is their share of the column square sums
    const double* x = extra + int64_t(NF * NF) * c + NF * i;
#pragma unroll
    for (int k = 0; k < NF; ++k) { row[k] += x[k]; if (k == i) sqsum += x[k]; }
  }
  if (D_f) {
    const double d = D_f[(cam_pos ? cam_pos[c] : cam_base + NF * c) + i];
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == i) row[k] += d * d;
  }
  double* out = blocks + (cam_diag_off ? cam_diag_off[c] : int64_t(NF * NF) * c) + NF * i;
#pragma unroll
  for (int k = 0; k < NF; ++k) out[k] = row[k];
  if (camsq) camsq[int64_t(NF) * c + i] = sqsum;
}

// The inversion proper, by the NF lanes [g0, g0 + NF) of a wavefront: lane i holds row i of the (symmetric) block on entry and writes
// column i of the inverse to a[.][i].  All 64 lanes call it (shuffles); inactive groups work on the identity.
__device__ __forceinline__ void invert_group_rows(double (&row)[NF], int i, int g0, bool active, double* __restrict__ a, int* __restrict__ fail_flag) {
  // L row i in Lr[0..i]
  double Lr[NF];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    // pivot row j (entries k < j are final) comes from lane g0 + j
    double pj[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) pj[k] = (k < j) ? shfl_idx(Lr[k], g0 + j) : 0.0;
    // diagonal, computed by every lane the same way from row j's data: a_jj - sum L_jk^2
    double ajj = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == j) ajj = row[k];
    double d = shfl_idx(ajj, g0 + j);
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k < j) d -= pj[k] * pj[k];
    if (!(d > 0.0)) { ok = false; d = 1.0; }
    d = sqrt(d);
    const double inv = 1.0 / d;
    // symmetric block: a_ji = a_ij is in this lane's row
    double sv = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == j) sv = row[k];
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k < j) sv -= Lr[k] * pj[k];
    Lr[j] = (i == j) ? d : (i > j ? sv * inv : 0.0);
  }
  if (!ok && active && fail_flag) atomicExch(fail_flag, 1);
  // every lane needs all of L for its solve
  double L[kTri];
#pragma unroll
  for (int r = 0; r < NF; ++r) {
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k <= r) L[r * (r + 1) / 2 + k] = shfl_idx(Lr[k], g0 + r);
  }
  double col[NF];
#pragma unroll
  for (int r = 0; r < NF; ++r) {  // L y = e_i
    double sacc = (r == i) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k < r) sacc -= L[r * (r + 1) / 2 + k] * col[k];
    col[r] = sacc / L[r * (r + 1) / 2 + r];
  }
#pragma unroll
  for (int r = NF - 1; r >= 0; --r) {  // L^T x = y
    double sacc = col[r];
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k > r) sacc -= L[k * (k + 1) / 2 + r] * col[k];
    col[r] = sacc / L[r * (r + 1) / 2 + r];
  }
  if (active) {
#pragma unroll
    for (int r = 0; r < NF; ++r) a[r * NF + i] = col[r];  // column i of the inverse; lanes of a group write contiguous bytes
  }
}

constexpr int kInvertGatherWaves = 4;
// The same, ONE camera per workgroup of kInvertGatherWaves wavefronts (bal_invert_kernel's gathering phase without the inversion): lane e
// adds up entry e of every kInvertGatherWaves-th item (coalesced records, two accumulators), wave 0 combines the waves' sums in a fixed
// order and writes the rows.  The kernel above walks a camera's items with one lane per row, one dependent round trip per item: 41 us on
// one rank's eighth of the Venice shape (profiles/r06a_*), as long as the camera-major pass it finishes.
__global__ __launch_bounds__(64 * kInvertGatherWaves) void bal_camera_finish_wide_kernel(const double* __restrict__ parts, const int32_t* __restrict__ cam_item_ptr,
                                                               const double* __restrict__ D_f, const int32_t* __restrict__ cam_pos, int cam_base,
                                                               const int64_t* __restrict__ cam_diag_off, double* __restrict__ blocks,
                                                               double* __restrict__ camsq, int n_cameras, const double* __restrict__ extra) {
  __shared__ double csum[kInvertGatherWaves][kCamPart];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.x;
  const int item_lo = cam_item_ptr[c], item_hi = cam_item_ptr[c + 1];
  for (int e = lane; e < kCamPart; e += 64) {
    double s0 = 0.0, s1 = 0.0;
    int it = item_lo + wv;
    for (; it + kInvertGatherWaves < item_hi; it += 2 * kInvertGatherWaves) {
      s0 += parts[int64_t(it) * kCamPart + e];
      s1 += parts[int64_t(it + kInvertGatherWaves) * kCamPart + e];
    }
    if (it < item_hi) s0 += parts[int64_t(it) * kCamPart + e];
    csum[wv][e] = s0 + s1;
  }
  __syncthreads();
  if (wv != 0) return;
  for (int e = lane; e < kCamPart; e += 64) {
    double t = csum[0][e];
    for (int w = 1; w < kInvertGatherWaves; ++w) t += csum[w][e];
    csum[0][e] = t;
  }
  __builtin_amdgcn_wave_barrier();
  const int i = lane;
  if (i >= NF) return;
  double row[NF], sqsum = camsq ? csum[0][kTri + i] : 0.0;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int ra = k < i ? k : i, rb = k < i ? i : k;
    row[k] = csum[0][tri_index(ra, rb)];
  }
  if (extra) {
    const double* x = extra + int64_t(NF * NF) * c + NF * i;
#pragma unroll
    for (int k = 0; k < NF; ++k) { row[k] += x[k]; if (k == i) sqsum += x[k]; }
  }
  if (D_f) {
    const double d = D_f[(cam_pos ? cam_pos[c] : cam_base + NF * c) + i];
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == i) row[k] += d * d;
  }
  double* out = blocks + (cam_diag_off ? cam_diag_off[c] : int64_t(NF * NF) * c) + NF * i;
#pragma unroll
  for (int k = 0; k < NF; ++k) out[k] = row[k];
  if (camsq) camsq[int64_t(NF) * c + i] = sqsum;
}

// Camera-major pass of ONE CHUNK of tiles when the camera accumulators do not fit in LDS: the tile pass of the chunk left
// F_o^T z_o (NF doubles) per slot in a ring buffer that is small enough to still be in the Infinity Cache; a unit = up to kZUnit
// entries of one camera inside the chunk.  NF lanes per unit (lane k sums component k: the bytes of an entry are one
// contiguous access of the group), kPerWave units per wavefront, four entries in flight per lane.  A camera covered by a single
// unit in this chunk is updated with a plain read-modify-write (chunks run one after the other on the stream); split cameras
// (more than kZUnit observations inside one chunk: the popular ones) combine with global_atomic_add_f64.
__global__ __launch_bounds__(256) void bal_camera_chunk_kernel(ZUnits U, const double* __restrict__ ring, double* __restrict__ acc,
                                                               const int* __restrict__ status) {
  if (status && *status != 0) return;
  const int lane = threadIdx.x & 63;
  const int g = lane / NF, k = lane - NF * g;
  const int64_t u = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * kPerWave + g;
  if (g >= kPerWave || u >= U.count) return;
  const int unit = U.first + int(u);
  const int c = U.cam[unit], beg = U.begin[unit], end = U.end[unit];
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int e = beg;
  for (; e + 7 < end; e += 8) {  // eight index words, then eight entries in flight
    int a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = U.slot[e + i];
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = ring[int64_t(NF) * a[i] + k];
    s0 += v[0] + v[4]; s1 += v[1] + v[5]; s2 += v[2] + v[6]; s3 += v[3] + v[7];
  }
  for (; e + 3 < end; e += 4) {
    const int a0 = U.slot[e], a1 = U.slot[e + 1], a2 = U.slot[e + 2], a3 = U.slot[e + 3];
    s0 += ring[int64_t(NF) * a0 + k]; s1 += ring[int64_t(NF) * a1 + k]; s2 += ring[int64_t(NF) * a2 + k]; s3 += ring[int64_t(NF) * a3 + k];
  }
  for (; e < end; ++e) s0 += ring[int64_t(NF) * U.slot[e] + k];
  const double v = (s0 + s1) + (s2 + s3);
  double* dst = acc + int64_t(NF) * c + k;
  if (U.shared[unit]) unsafeAtomicAdd(dst, v);
  else *dst += v;
}

// In-place inverse of the NF x NF SPD camera blocks from their upper triangle (Cholesky +
// solves against I, like BlockRandomAccessDiagonalMatrix::Invert,
// I/block_random_access_diagonal_matrix.cc:90-100).
// NF lanes per camera (kPerWave cameras per wavefront): lane i of a group owns row i of the
// block.  The Cholesky factor is built column by column with the pivot row broadcast by
// shuffles; lane e then solves L L^T x = e_e for "its" column of the inverse.  Same operation
// order per entry as a scalar column-Cholesky (the reference: Eigen LLT on the upper triangle,
// I/block_random_access_diagonal_matrix.cc:106-127); one thread per camera, as this kernel first
// was, ran a ~1000-instruction dependent chain with strided accesses: 31 us for 1778 cameras.
__global__ __launch_bounds__(64 * kInvertGatherWaves) void bal_invert_kernel(double* __restrict__ blocks, const int64_t* __restrict__ cam_diag_off,
                                                         int n_cameras, int* fail_flag, LmFuse lm, CamGather gather) {
  __shared__ double csum[kInvertGatherWaves][kCamPart];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int grp = lane / NF, i = lane - NF * grp;  // the lanes behind kPerWave groups idle
  // assembled blocks: kPerWave cameras per wavefront (64-thread workgroups); per-item partial sums (gather.parts): ONE camera per
  // workgroup of kInvertGatherWaves wavefronts, whose kCamPart lanes each add up every kInvertGatherWaves-th item of the camera entry by
  // entry (coalesced rows) — the kernel lasts as long as its most popular camera, whose item list one wavefront alone
  // walked for 46 us on the Venice shape —, then wave 0 combines the partial sums in a fixed order and lanes 0..NF-1 take the rows
  // gather.few: cameras of a handful of items each (tens of thousands of cameras with tens of observations: video-like scenes) — kPerWave
  // cameras per wavefront here too, every lane adding up its row over the camera's items (a workgroup per camera was 206 us for
  // 52 800 cameras of one item each, latency from end to end)
  const bool few = gather.parts != nullptr && gather.few != 0;
  const bool gathering = gather.parts != nullptr && !few;
  const bool from_packed = gather.packed != nullptr;   // the items' sums are already added up (and summed over ranks): bal_camera_exchange_kernel
  const int c = gathering ? int(blockIdx.x) : int(blockIdx.x) * kPerWave + grp;
  const bool active = (gathering ? grp == 0 : grp < kPerWave) && c < n_cameras;
  const int cc = active ? c : 0;
  const int g0 = NF * ((!gathering && grp < kPerWave) ? grp : 0);        // first lane of the group
  double* a = blocks + (cam_diag_off ? cam_diag_off[cc] : int64_t(NF * NF) * cc);
  double row[NF], sq_from_items = 0.0;
  auto add_extra_and_diagonal = [&]() {
    if (gather.extra) {  // rows outside the tiles (no point cell): their F^T F, whose diagonal is their share of the column square sums
      const double* x = gather.extra + int64_t(NF * NF) * c + NF * i;
#pragma unroll
      for (int k = 0; k < NF; ++k) { row[k] += x[k]; if (k == i) sq_from_items += x[k]; }
    }
    if (gather.D_f) {
      const double d = gather.D_f[(gather.cam_pos ? gather.cam_pos[c] : gather.cam_base + NF * c) + i];
#pragma unroll
      for (int k = 0; k < NF; ++k) if (k == i) row[k] += d * d;
    }
  };
  if (from_packed) {
    if (active) {
      const double* p = gather.packed + int64_t(kCamPart) * c;
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        const int ra = k < i ? k : i, rb = k < i ? i : k;
        row[k] = p[tri_index(ra, rb)];
      }
      sq_from_items = p[kTri + i];
      if (gather.D_f) {
        const double d = gather.D_f[(gather.cam_pos ? gather.cam_pos[c] : gather.cam_base + NF * c) + i];
#pragma unroll
        for (int k = 0; k < NF; ++k) if (k == i) row[k] += d * d;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NF; ++k) row[k] = (k == i ? 1.0 : 0.0);
    }
  } else if (few) {
    if (active) {
      gather_camera_row(gather.parts, gather.cam_item_ptr[c], gather.cam_item_ptr[c + 1], i, row, sq_from_items, gather.want_sq != 0);
      add_extra_and_diagonal();
    } else {
#pragma unroll
      for (int k = 0; k < NF; ++k) row[k] = (k == i ? 1.0 : 0.0);
    }
  } else if (gathering) {  // the blocks are still per-item partial sums: combine them here (bal_camera_items_kernel)
    const int item_lo = gather.cam_item_ptr[blockIdx.x], item_hi = gather.cam_item_ptr[blockIdx.x + 1];
    for (int e = lane; e < kCamPart; e += 64) {
      double s0 = 0.0, s1 = 0.0;
      int it = item_lo + wv;
      for (; it + nwv < item_hi; it += 2 * nwv) {
        s0 += gather.parts[int64_t(it) * kCamPart + e];
        s1 += gather.parts[int64_t(it + nwv) * kCamPart + e];
      }
      if (it < item_hi) s0 += gather.parts[int64_t(it) * kCamPart + e];
      csum[wv][e] = s0 + s1;
    }
    __syncthreads();
    if (wv != 0) return;
    for (int e = lane; e < kCamPart; e += 64) {
      double t = csum[0][e];
      for (int w = 1; w < nwv; ++w) t += csum[w][e];
      csum[0][e] = t;
    }
    __builtin_amdgcn_wave_barrier();
    if (active) {
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        const int ra = k < i ? k : i, rb = k < i ? i : k;
        row[k] = csum[0][tri_index(ra, rb)];
      }
      sq_from_items = csum[0][kTri + i];
      add_extra_and_diagonal();
    } else {
#pragma unroll
      for (int k = 0; k < NF; ++k) row[k] = (k == i ? 1.0 : 0.0);
    }
  } else {
#pragma unroll
    for (int k = 0; k < NF; ++k) row[k] = active ? a[i * NF + k] : (k == i ? 1.0 : 0.0);
  }
  if (lm.radius > 0.0 && active) {  // fused LM diagonal of the camera columns: d = clamp(diag(F^T F)), D^2 = d / radius
    const int o = lm.cam_pos ? lm.cam_pos[c] : lm.cam_base + NF * c;
    double dii = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == i) dii = row[k];
    const double v = lm.camsq ? lm.camsq[int64_t(NF) * c + i] : (((gather.parts || gather.packed) && gather.want_sq) ? sq_from_items : dii);
    const double d = fmin(fmax(v, lm.min_d), lm.max_d), q = d / lm.radius;
    lm.diag_f[o + i] = d;
    lm.D_f[o + i] = sqrt(q);
#pragma unroll
    for (int k = 0; k < NF; ++k) if (k == i) row[k] += q;
  }
  invert_group_rows(row, i, g0, active, a, fail_flag);
}

// The camera-major pass's sums for a SHARDED instance, summed over ranks in the kernel that adds up this rank's items (p2p.h): a workgroup
// per camera as in bal_camera_finish_wide_kernel, wave 0 takes the kCamPart packed sums (upper triangle + column square sums) through
// the exchange (slot index = kCamPart c + e, chunk = kCamChunks c + e / 64) and leaves them, PACKED, in `packed`; bal_invert_kernel
// then reads them seven cameras per wavefront (CamGather::packed).  Two launches for what was bal_camera_finish_kernel, the step's
// merged all-reduce, the diagonal pass and bal_invert_kernel (41 + 46 + 6 us on one rank's eighth of the Venice shape:
// profiles/r06a_*) — and 54 instead of 99 doubles per camera and peer on the wire.  (One kernel with the inversion behind the exchange
// was tried first: 189 VGPRs for all four waves of a workgroup, two workgroups per CU, 41 us; profiles/r06d_*.)
// Workgroups take every gridDim.x-th camera (ranks that share a device must fit beside each other while they wait).
constexpr int kCamChunks = (kCamPart + 63) / 64;
__global__ __launch_bounds__(64 * kInvertGatherWaves) void bal_camera_exchange_kernel(const double* __restrict__ parts, const int32_t* __restrict__ cam_item_ptr,
                                                         int n_cameras, const double* __restrict__ extra, double* __restrict__ packed, P2pComm C) {
  __shared__ double csum[kInvertGatherWaves][kCamPart];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c = blockIdx.x; c < n_cameras; c += gridDim.x) {
    const int item_lo = cam_item_ptr[c], item_hi = cam_item_ptr[c + 1];
    for (int e = lane; e < kCamPart; e += 64) {
      double s0 = 0.0, s1 = 0.0;
      int it = item_lo + wv;
      for (; it + kInvertGatherWaves < item_hi; it += 2 * kInvertGatherWaves) {
        s0 += parts[int64_t(it) * kCamPart + e];
        s1 += parts[int64_t(it + kInvertGatherWaves) * kCamPart + e];
      }
      if (it < item_hi) s0 += parts[int64_t(it) * kCamPart + e];
      csum[wv][e] = s0 + s1;
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int q = 0; q < kCamChunks; ++q) {
        const int e = 64 * q + lane;
        const bool act = e < kCamPart;
        double t = 0.0;
        if (act) {
          t = csum[0][e];
          for (int w = 1; w < kInvertGatherWaves; ++w) t += csum[w][e];
          if (extra) {  // this rank's rows outside the tiles (no point cell): their F^T F joins the raw sums; its diagonal = their column square sums
            const double* x = extra + int64_t(NF * NF) * c;
            if (e >= kTri) t += x[(e - kTri) * (NF + 1)];
            else {
              for (int a = 0; a < NF; ++a)
                for (int b = a; b < NF; ++b) if (tri_index(a, b) == e) t += x[a * NF + b];
            }
          }
        }
        t = p2p_exchange_wave(C, kCamChunks * c + q, int64_t(kCamPart) * c + e, act, t);
        if (act) packed[int64_t(kCamPart) * c + e] = t;
      }
    }
    __syncthreads();   // csum is reused by the next camera
  }
}

// The same for cameras of a HANDFUL of items each (tens of thousands of cameras: a workgroup per camera was 267 us for 50 000 cameras on
// one rank's eighth of synthetic10M, profiles/r06e_*): a wavefront takes kCamFew consecutive cameras — lane e adds up entry e of each
// camera's items alone — through ONE exchange round trip (p2p_exchange_wave_multi: the same slots and chunks as above, which needs
// kCamChunks == 1).
constexpr int kCamFew = 4;
__global__ __launch_bounds__(256) void bal_camera_exchange_few_kernel(const double* __restrict__ parts, const int32_t* __restrict__ cam_item_ptr,
                                                         int n_cameras, const double* __restrict__ extra, double* __restrict__ packed, P2pComm C) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t n_rounds = (n_cameras + kCamFew - 1) / kCamFew;
  for (int64_t r = int64_t(blockIdx.x) * 4 + wv; r < n_rounds; r += int64_t(gridDim.x) * 4) {
    const int c0 = int(r) * kCamFew;
    double v[kCamFew];
#pragma unroll
    for (int k = 0; k < kCamFew; ++k) {
      const int c = c0 + k;
      double t = 0.0;
      if (c < n_cameras && lane < kCamPart) {
        const int item_lo = cam_item_ptr[c], item_hi = cam_item_ptr[c + 1];
        double t1 = 0.0, t2 = 0.0, t3 = 0.0;
        int it = item_lo;
        for (; it + 3 < item_hi; it += 4) {   // (a popular camera's many items: independent loads, four sums)
          t += parts[int64_t(it) * kCamPart + lane]; t1 += parts[int64_t(it + 1) * kCamPart + lane];
          t2 += parts[int64_t(it + 2) * kCamPart + lane]; t3 += parts[int64_t(it + 3) * kCamPart + lane];
        }
        for (; it < item_hi; ++it) t += parts[int64_t(it) * kCamPart + lane];
        t = (t + t1) + (t2 + t3);
        if (extra) {
          const double* x = extra + int64_t(NF * NF) * c;
          if (lane >= kTri) t += x[(lane - kTri) * (NF + 1)];
          else {
            for (int a = 0; a < NF; ++a)
              for (int b = a; b < NF; ++b) if (tri_index(a, b) == lane) t += x[a * NF + b];
          }
        }
      }
      v[k] = t;
    }
    p2p_exchange_wave_multi<kCamFew>(C, c0, int64_t(kCamPart) * c0, kCamPart, kCamPart, int64_t(kCamPart) * n_cameras, v);
#pragma unroll
    for (int k = 0; k < kCamFew; ++k)
      if (c0 + k < n_cameras && lane < kCamPart) packed[int64_t(kCamPart) * (c0 + k) + lane] = v[k];
  }
}

// The strip's matrix from the workgroups' partial sums (fixed order), cut into the shared blocks' dense diagonal blocks (+ D^2) at
// their places in the F-block store.  One workgroup.
__global__ __launch_bounds__(1024) void bal_strip_finish_kernel(const double* __restrict__ parts, int nparts, StripBlocks sb,
                                                                const double* __restrict__ D_f, double* __restrict__ blocks) {
  __shared__ double T[16][kTriSX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // wave w adds the partials w, w + 16, ... of entry `lane` (independent loads), then the sixteen wave sums in a fixed order
  for (int i = lane; i < kTriS; i += 64) {
    double t0 = 0, t1 = 0;
    int w = wv;
    for (; w + 16 < nparts; w += 32) { t0 += parts[int64_t(w) * kTriS + i]; t1 += parts[int64_t(w + 16) * kTriS + i]; }
    if (w < nparts) t0 += parts[int64_t(w) * kTriS + i];
    T[wv][i] = t0 + t1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTriS; i += 1024) {
    double t = T[0][i];
    for (int w = 1; w < 16; ++w) t += T[w][i];
    T[0][i] = t;
  }
  __syncthreads();
  for (int q = 0; q < sb.count; ++q) {
    const int w = sb.width[q], o = sb.off[q];
    for (int e = threadIdx.x; e < w * w; e += 1024) {
      const int a = e / w, b = e - a * w;
      const int lo = o + (a < b ? a : b), hi = o + (a < b ? b : a);
      double v = T[0][lo * (2 * NS + 1 - lo) / 2 + (hi - lo)];
      if (a == b && D_f) { const double d = D_f[sb.pos[q] + a]; v += d * d; }
      blocks[sb.out[q] + e] = v;
    }
  }
}

// The point tail of a short ITERATIVE_SCHUR solve that began at x = 0 (PointTailArgs, device.h; design/20_point_tail.md).  CG built
// z = sum_k alpha_k p_k, and S.x pass k kept u_k[p] = sum over the point's observations of E^T F p_k, so E_p^T F z = U_p = sum_k alpha_k u_k[p]
// (ascending k) and the point part of the solution is y_p = Ei_p (t_p - U_p), t_p = E_p^T b, Ei_p = (E_p^T E_p + D_p^2)^-1: no pass over J.
// Model cost change of the step -(y, z), with g = J^T b, rhs = F^T b - sum_p F^T E Ei_p t_p and r = rhs - S z (CG's residual):
//   (y.t + z.rhs + sum_p U_p.(Ei_p t_p) + z.r + |D_e y|^2 + |D_f z|^2) / 2
// since (J^T J + D^2) (y, z) = g - (0, r) — the point rows hold exactly — and z.F^T b = z.rhs + sum_p U_p.(Ei_p t_p).  Every term is a sum
// of products of like sign or small.  One partial per workgroup (its points' and its camera scalars' share of all six terms, halved),
// summed by the host in index order.
__global__ __launch_bounds__(kPointTailBlock) void bal_point_tail_kernel(PointTailArgs T) {
  const int status = T.S->status, n = T.S->n_updates;
  if (!PointTailTakes(status, n)) return;
  double al[kPointTailMaxIterations];
#pragma unroll
  for (int k = 0; k < kPointTailMaxIterations; ++k) al[k] = k < n ? T.S->alpha_hist[k] : 0.0;
  const double sg = T.negate ? -1.0 : 1.0;
  const int64_t tid = int64_t(blockIdx.x) * kPointTailBlock + threadIdx.x, nthreads = int64_t(gridDim.x) * kPointTailBlock;
  double cost = 0.0;
  int bad = 0;
  for (int64_t p = tid; p < T.n_points; p += nthreads) {
    const int po = T.pt_pos ? T.pt_pos[p] : NE * int(p);
    const double2* q = reinterpret_cast<const double2*>(T.etei + p * kEteiPitch);
    double2 rec[kEteiPitch / 2];
#pragma unroll
    for (int j = 0; j < kEteiPitch / 2; ++j) rec[j] = q[j];
    double ei[kTriE], U[NE], t[NE], w[NE], y[NE], eit[NE];
#pragma unroll
    for (int i = 0; i < kTriE; ++i) ei[i] = (i & 1) ? rec[i / 2].y : rec[i / 2].x;
#pragma unroll
    for (int j = 0; j < NE; ++j) { U[j] = 0.0; t[j] = T.etb[po + j]; }
#pragma unroll
    for (int k = 0; k < kPointTailMaxIterations; ++k) {
      if (k < n) {   // (launch-uniform; buffers beyond n hold an earlier solve's sums, or nothing)
#pragma unroll
        for (int j = 0; j < NE; ++j) U[j] += al[k] * T.u_hist[k * T.u_stride + NE * p + j];
      }
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) w[j] = t[j] - U[j];
    sym_mul(ei, w, y);
    double fin = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) { T.y_e[po + j] = sg * y[j]; fin += y[j]; }
    if (!isfinite(fin)) ++bad;
    if (T.cost_out) {
      sym_mul(ei, t, eit);
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const double d = T.D_e ? T.D_e[po + j] * y[j] : 0.0;
        cost += y[j] * t[j] + U[j] * eit[j] + d * d;
      }
    }
  }
  for (int64_t i = tid; i < T.n_f; i += nthreads) {   // the camera part: x_f = z, and the camera-space terms
    const double z = T.z[i];
    T.y_f[i] = sg * z;
    if (!isfinite(z)) ++bad;
    if (T.cost_out) {
      const double d = T.D_f ? T.D_f[i] * z : 0.0;
      cost += z * T.rhs[i] + z * T.r[i] + d * d;
    }
  }
  if (bad && T.negate) atomicAdd(T.nonfinite, bad);
  if (T.cost_out) {
    __shared__ double red[kPointTailBlock / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cost += __shfl_xor(cost, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < kPointTailBlock / 64; ++i) s += red[i];
      T.cost_out[blockIdx.x] = 0.5 * s;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Launchers (this shape's; solver.hip reaches them through the BalOps table at the end of the file)
// ---------------------------------------------------------------------------
template <int MODE, int BLOCK, bool F32>
static hipError_t launch_fused2(const BalArgs& A, bool lds, int grid, hipStream_t stream) {
  if (lds) {
    const size_t bytes = size_t(A.n_acc) * sizeof(double);
    auto k = bal_fused_kernel<MODE, true, BLOCK, F32>;
    if (hipError_t e = AllowMaxLds(reinterpret_cast<const void*>(k)); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), bytes, stream, A);
  } else {
    // scattering modes: the hybrid accumulator rows (none without a hybrid plan) + one 64 x NF strip per wave for the spilled rows
    constexpr bool kScatters = (MODE == kSx || MODE == kJtJx || MODE == kJtb || MODE == kInit || MODE == kCgnrInit || MODE == kColNorm || MODE == kSpseZ);
    const size_t bytes = kScatters ? (size_t(A.hyb_rows) * NF + size_t(BLOCK / 64) * kTile * NF) * sizeof(double)
                                   : ((MODE == kBackSub || MODE == kJx) ? size_t(A.x_lds_scalars) * sizeof(double) : 0);
    auto k = bal_fused_kernel<MODE, false, BLOCK, F32>;
    if (bytes > 0)
      if (hipError_t e = AllowMaxLds(reinterpret_cast<const void*>(k)); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), bytes, stream, A);
  }
  return hipGetLastError();
}
template <int MODE, int BLOCK>
static hipError_t launch_fused(const BalArgs& A, bool lds, int grid, hipStream_t stream) {
  if constexpr (kHasF32) {
    if (A.Jf) return launch_fused2<MODE, BLOCK, true>(A, lds, grid, stream);
  } else {
    if (A.Jf) return hipErrorInvalidValue;   // fp32 tiles exist for the BAL shape only (solver.hip refuses the option for the others)
  }
  return launch_fused2<MODE, BLOCK, false>(A, lds, grid, stream);
}

#if CERES_HIP_PIPELINED
template <int MODE, bool NT, bool F32 = false, bool CAP = false>
static hipError_t launch_stream2(const BalArgs& A, bool lds, int grid, hipStream_t stream) {
  if (lds) {
    auto k = bal_stream_kernel<MODE, true, NT, F32, CAP>;
    if (hipError_t e = AllowMaxLds(reinterpret_cast<const void*>(k)); e != hipSuccess) return e;
    // (+ the scratch of the CG iteration tail: cg_iteration_tail)
    const size_t tail_bytes = (kHasCgTail && MODE == kSx && A.tail.enabled) ? size_t(512 + kCgTailMax) * sizeof(double) : 0;
    // the plan sized the staged x for a fixed reserve of static LDS (plan.cc: 1 KiB); what this kernel really has is its attribute —
    // a launch that would not fit runs without the staged x (every consumer masks the slot word's row field: finish_slot) instead of failing
    static const size_t static_lds = [&] { hipFuncAttributes fa{}; return hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k)) == hipSuccess ? size_t(fa.sharedSizeBytes) : size_t(1024); }();
    BalArgs B = A;
    if (size_t(B.n_acc) * sizeof(double) + size_t(B.n_xhot) * NF * sizeof(double) + static_lds > kMaxLdsBytes) B.n_xhot = 0;
    const size_t xhot_bytes = size_t(B.n_xhot) * NF * sizeof(double);   // (the tail runs when the tiles are done: the two share the space)
    hipLaunchKernelGGL(k, dim3(grid), dim3(512), size_t(B.n_acc) * sizeof(double) + std::max(tail_bytes, xhot_bytes), stream, B);
  } else {
    auto k = bal_stream_kernel<MODE, false, NT, F32>;
    if (hipError_t e = AllowMaxLds(reinterpret_cast<const void*>(k)); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(512), (size_t(A.hyb_rows) * NF + size_t(512 / 64) * kTile * NF) * sizeof(double), stream, A);
  }
  return hipGetLastError();
}
template <int MODE>
static hipError_t launch_stream(const BalArgs& A, bool lds, int grid, hipStream_t stream) {
  // tiles that fit the 256 MiB Infinity Cache are read with plain loads (see issue_pairs)
  if (A.Jf) {   // fp32 tiles (round 5: pipelined as well)
    if constexpr (kHasF32) {
      const bool nt32 = A.n_tiles * int64_t(6 * kTile) * int64_t(sizeof(float4)) > (int64_t(kNonTemporalTileMiB) << 20);
      return nt32 ? launch_stream2<MODE, true, true>(A, lds, grid, stream) : launch_stream2<MODE, false, true>(A, lds, grid, stream);
    } else {
      return hipErrorInvalidValue;   // fp32 tiles exist for the BAL shape only (solver.hip refuses the option for the others)
    }
  }
  const bool nt = A.n_tiles * int64_t(kTilePitch) * int64_t(sizeof(double2)) > (int64_t(kNonTemporalTileMiB) << 20);
  if constexpr (MODE == kSx) {   // the capturing instantiation (point tail): every camera's accumulator in LDS, fp64 tiles
    if (A.u_out && lds) return nt ? launch_stream2<MODE, true, false, true>(A, lds, grid, stream) : launch_stream2<MODE, false, false, true>(A, lds, grid, stream);
  }
  return nt ? launch_stream2<MODE, true>(A, lds, grid, stream) : launch_stream2<MODE, false>(A, lds, grid, stream);
}

#endif   // CERES_HIP_PIPELINED

// CERES_HIP_PIPELINE=0 falls back to the unpipelined kernels (A/B measurements).
static bool UsePipeline() {
  static int v = [] { const char* e = getenv("CERES_HIP_PIPELINE"); return e ? atoi(e) : 1; }();
  return CERES_HIP_PIPELINED && v != 0;
}

// CERES_HIP_F32_PIPELINE=0: fp32 tiles on the unpipelined kernels, as until round 4 (A/B measurements)
static bool F32Pipelined() {
  static int v = [] { const char* e = getenv("CERES_HIP_F32_PIPELINE"); return e ? atoi(e) : 1; }();
  return kHasF32 && v != 0;
}
static bool SxRunsPipelined(const BalArgs& A) { return UsePipeline() && (!A.Jf || F32Pipelined()) && !A.src_values && !A.cam_pos && !(A.flags & 1); }

static hipError_t Fused(int mode, const BalArgs& A0, bool lds, int grid, hipStream_t stream) {
  BalArgs A = A0;
  if ((mode != kBackSub && mode != kJx) || lds) A.x_lds_scalars = 0;   // (only the modes whose LDS is free: load_xc)
  // a workgroup stages its copy of x once per launch: that pays from about a hundred tiles per workgroup on — of THIS launch's tiles and
  // workgroups (Ladybug-sized problems, 41 tiles per workgroup, lose 3 us of a 42 us pass to it: profiles/r05n_*)
  if ((A.tile_end > 0 ? A.tile_end - A.tile_begin : A.n_tiles) < int64_t(kStagedXMinTilesPerWg) * grid) { A.n_xhot = 0; A.x_lds_scalars = 0; }
  const bool big = BalBlockFor(mode) == 1024;
  // A few dozen tiles per workgroup (one rank's eighth of the Venice shape: 38; the Ladybug shape: 41): a wave of the software-pipelined
  // kernel gets five tiles, hardly more than the pipeline's fill and drain — the plain 512-thread kernels are 10 us per S.x faster there
  // (0.367 -> 0.345 ms per step on that shard, profiles/r06m_*); from about 76 tiles per workgroup on the pipeline wins.  (Not where the
  // S.x pass finishes the CG iteration: that tail lives in the pipelined kernel.)
  // At 41 (Ladybug) the two are level in a step (0.320 vs 0.328 ms) while back-to-back launches of the pipelined kernel are 13 % faster
  // (0.041 vs 0.047 ms per S.x: its code is warm in the instruction cache then): the line is drawn at kPipelineMinTilesPerWg = 40.
  const bool few_tiles = (A.tile_end > 0 ? A.tile_end - A.tile_begin : A.n_tiles) < int64_t(kPipelineMinTilesPerWg) * grid && !A.tail.enabled && lds;
  const bool big_s = big && (lds || A.hyb_rows == 0) && !few_tiles;  // scattering modes with hybrid rows: the rows are sized for 8 waves' strips
#if CERES_HIP_PIPELINED
  if (UsePipeline() && !few_tiles && (!A.Jf || F32Pipelined()) && !A.src_values && !A.cam_pos && !(A.flags & 1)) {
    // (S.x and the power-series operator index nothing of the caller's by point: pt_pos may be set — renumbered points, plan.cc)
    if (mode == kSx) return launch_stream<kSx>(A, lds, grid, stream);
    if (mode == kJtJx && A.D_e && !A.pt_pos) return launch_stream<kJtJx>(A, lds, grid, stream);
    if (mode == kSpseZ) return launch_stream<kSpseZ>(A, lds, grid, stream);
  }
#endif
  switch (mode) {
    case kSx: return big_s ? launch_fused<kSx, 1024>(A, lds, grid, stream) : launch_fused<kSx, 512>(A, lds, grid, stream);
    case kJtJx: return big_s ? launch_fused<kJtJx, 1024>(A, lds, grid, stream) : launch_fused<kJtJx, 512>(A, lds, grid, stream);
    case kJtb: return (big_s && !A.src_values) ? launch_fused<kJtb, 1024>(A, lds, grid, stream) : launch_fused<kJtb, 512>(A, lds, grid, stream);
    case kInit: return launch_fused<kInit, 512>(A, lds, grid, stream);
    case kEte: return big ? launch_fused<kEte, 1024>(A, false, grid, stream) : launch_fused<kEte, 512>(A, false, grid, stream);
    case kBackSub: return big ? launch_fused<kBackSub, 1024>(A, false, grid, stream) : launch_fused<kBackSub, 512>(A, false, grid, stream);
    case kCgnrInit: return launch_fused<kCgnrInit, 512>(A, lds, grid, stream);
    case kColNorm: return launch_fused<kColNorm, 512>(A, true, grid, stream);
    case kJx: return launch_fused<kJx, 1024>(A, false, grid, stream);
    case kSpseZ: return big_s ? launch_fused<kSpseZ, 1024>(A, lds, grid, stream) : launch_fused<kSpseZ, 512>(A, lds, grid, stream);
    case kShBlocks:
      if constexpr (NS > 0) return launch_fused2<kShBlocks, 256, false>(A, false, grid, stream);   // (256: one wave per SIMD, the sums of a wide strip then live in registers instead of scratch)
      else return hipErrorInvalidValue;
  }
  return hipErrorInvalidValue;
}

static hipError_t StripFinish(const double* parts, int nparts, const StripBlocks& sb, const double* D_f, double* blocks, hipStream_t stream) {
  if constexpr (NS > 0) {
    hipLaunchKernelGGL(bal_strip_finish_kernel, dim3(1), dim3(1024), 0, stream, parts, nparts, sb, D_f, blocks);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

static hipError_t ReducePartials(const double* partials, int nparts, int n_acc, const FMap& map,
                                 const double* D_f, const double* x_f, double* y_f, const int* status,
                                 double* pq_out, int* n_pq, hipStream_t stream, const double* sum_in, int n_sum_in,
                                 double* sum_out) {
  const int grid = std::max(1, std::min((n_acc + 63) / 64, kMaxVecGrid));
  if (!x_f) pq_out = nullptr;
  if (n_pq) *n_pq = pq_out ? grid : 0;
  hipLaunchKernelGGL(bal_reduce_partials_kernel, dim3(grid), dim3(512), 0, stream, partials, nparts,
                     n_acc, map, D_f, x_f, y_f, status, pq_out, sum_in, n_sum_in, sum_out);
  return hipGetLastError();
}

// sharded: reduction + exchange over ranks + D_f^2 x_f + partial x_f . y_f in one launch; grid_cap bounds the workgroups (ranks that SHARE
// a device must all fit beside each other while they wait for one another)
static hipError_t ReduceExchange(const double* partials, int nparts, int n_acc, int n_fv, const FMap& map,
                                 const double* D_f, const double* x_f, double* y_f, const int* status,
                                 double* pq_out, int* n_pq, hipStream_t stream, const double* sum_in, int n_sum_in,
                                 double* sum_out, const P2pComm& comm, int grid_cap) {
  if (map.cam_pos) return hipErrorNotSupported;   // cameras scattered over F space: the caller takes the separate launches
  const int grid = std::max(1, std::min(std::min((n_fv + 64) / 64, kMaxVecGrid), std::max(1, grid_cap)));
  if (!x_f) pq_out = nullptr;
  if (n_pq) *n_pq = pq_out ? grid : 0;
  hipLaunchKernelGGL(bal_reduce_exchange_kernel, dim3(grid), dim3(512), 0, stream, partials, nparts,
                     n_acc, n_fv, map, D_f, x_f, y_f, status, pq_out, sum_in, n_sum_in, sum_out, comm);
  return hipGetLastError();
}

static hipError_t StreamProbe(const double2* J, int64_t n_tiles, int grid, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(bal_stream_probe_kernel, dim3(grid), dim3(1024), 0, stream, J, n_tiles, out);
  return hipGetLastError();
}

static hipError_t AddFDiagonal(int n_acc, const FMap& map, const double* D_f, const double* x_f, double* y_f,
                               const int* status, double* pq_out, int* n_pq, hipStream_t stream) {
  const int grid = std::max(1, std::min((n_acc + 255) / 256, kMaxVecGrid));
  if (!x_f) pq_out = nullptr;
  if (n_pq) *n_pq = pq_out ? grid : 0;
  if (!D_f && !pq_out) return hipSuccess;
  hipLaunchKernelGGL(bal_add_f_diagonal_kernel, dim3(grid), dim3(256), 0, stream, n_acc, map, D_f,
                     x_f, y_f, status, pq_out);
  return hipGetLastError();
}

static hipError_t Pack(const BalArgs& A, hipStream_t stream) {
  if (A.n_tiles == 0) return hipSuccess;
  const dim3 grid(unsigned((A.n_tiles + 3) / 4));
  if (A.Jf_out) {
    if constexpr (kHasF32) hipLaunchKernelGGL((bal_pack_kernel<true>), grid, dim3(256), 0, stream, A);
    else return hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((bal_pack_kernel<false>), grid, dim3(256), 0, stream, A);
  }
  return hipGetLastError();
}

static hipError_t Invert(double* blocks, const int64_t* cam_diag_off, int n_cameras, int* fail_flag, const LmFuse& lm,
                         const CamGather& gather, hipStream_t stream) {
  const bool wg_per_camera = gather.parts && !gather.few && !gather.packed;
  if (n_cameras > 0) hipLaunchKernelGGL(bal_invert_kernel, dim3(wg_per_camera ? n_cameras : (n_cameras + kPerWave - 1) / kPerWave), dim3(wg_per_camera ? 64 * kInvertGatherWaves : 64), 0, stream, blocks, cam_diag_off, n_cameras, fail_flag, lm, gather);
  return hipGetLastError();
}

// sharded: this rank's items of every camera added up and summed over ranks, packed (kCamPart per camera) into `packed`
static hipError_t CameraExchange(const double* parts, const int32_t* cam_item_ptr, int n_cameras, const double* extra, double* packed,
                                 const P2pComm& comm, int grid_cap, hipStream_t stream, bool few) {
  if (n_cameras <= 0) return hipSuccess;
  if (few && kCamChunks == 1) {   // cameras of a handful of items: four cameras per wavefront and round trip
    const int64_t rounds = (n_cameras + kCamFew - 1) / kCamFew;
    const int grid = int(std::max<int64_t>(1, std::min<int64_t>((rounds + 3) / 4, std::max(1, std::min(grid_cap, 4096)))));
    hipLaunchKernelGGL(bal_camera_exchange_few_kernel, dim3(grid), dim3(256), 0, stream, parts, cam_item_ptr, n_cameras, extra, packed, comm);
    return hipGetLastError();
  }
  const int grid = std::max(1, std::min(n_cameras, std::max(1, grid_cap)));
  hipLaunchKernelGGL(bal_camera_exchange_kernel, dim3(grid), dim3(64 * kInvertGatherWaves), 0, stream, parts, cam_item_ptr, n_cameras, extra, packed, comm);
  return hipGetLastError();
}

static hipError_t CameraItems(bool schur, const double* values, const CamItems& items, const int32_t* cam_fpos,
                              const int32_t* cam_slot, const double* Mo, double* parts, hipStream_t stream) {
  if (items.count == 0) return hipSuccess;
  const dim3 grid((items.count + 3) / 4);
  if (items.ev_cam_pack) {   // the F cells are evaluated, not read (values may be nullptr)
#if CERES_HIP_IS_BAL_SHAPE
    const bool robust = items.ev_loss.type != kLossNone;
    if (schur && robust) hipLaunchKernelGGL((bal_camera_items_eval_kernel<true, true>), grid, dim3(256), 0, stream, items, cam_slot, Mo, parts);
    else if (schur) hipLaunchKernelGGL((bal_camera_items_eval_kernel<true, false>), grid, dim3(256), 0, stream, items, cam_slot, Mo, parts);
    else if (robust) hipLaunchKernelGGL((bal_camera_items_eval_kernel<false, true>), grid, dim3(256), 0, stream, items, cam_slot, Mo, parts);
    else hipLaunchKernelGGL((bal_camera_items_eval_kernel<false, false>), grid, dim3(256), 0, stream, items, cam_slot, Mo, parts);
    return hipGetLastError();
#else
    return hipErrorInvalidValue;
#endif
  }
  // Items of a few hundred observations at most (small problems: plan.cc cuts them short so that they spread over the chip; cameras
  // of video-like scenes: tens of observations): the matrix-pipe kernel — Ladybug shape 0.079 -> 0.060 ms, Dubrovnik 0.034 -> 0.026,
  // 52 800 cameras of 38 observations 0.42 -> 0.19 (profiles/r03zj_*).  Full-length items (kCamChunk = 512 observations, the Venice
  // shape): the lane-per-observation kernel keeps 64 records in flight per wavefront and is 8 % ahead there.
  // CERES_HIP_CAM_ITEMS_MFMA=0 / 1 forces one of them (A/B).
  static const int forced = [] { const char* e = getenv("CERES_HIP_CAM_ITEMS_MFMA"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
  const bool mfma = NR == 2 && (forced >= 0 ? forced == 1 : items.observations < int64_t(kCamItemLaneMinMean) * items.count);
  if (mfma) {
#if CERES_HIP_NR == 2
    if (schur) hipLaunchKernelGGL((bal_camera_items_mfma_kernel<true>), grid, dim3(256), 0, stream, values, items, cam_fpos, cam_slot, Mo, parts);
    else hipLaunchKernelGGL((bal_camera_items_mfma_kernel<false>), grid, dim3(256), 0, stream, values, items, cam_fpos, cam_slot, Mo, parts);
#endif
  } else {
    if (schur) hipLaunchKernelGGL((bal_camera_items_kernel<true>), grid, dim3(256), 0, stream, values, items, cam_fpos, cam_slot, Mo, parts);
    else hipLaunchKernelGGL((bal_camera_items_kernel<false>), grid, dim3(256), 0, stream, values, items, cam_fpos, cam_slot, Mo, parts);
  }
  return hipGetLastError();
}

static hipError_t CameraFinish(const double* parts, const int32_t* cam_item_ptr, const double* D_f, const int32_t* cam_pos, int cam_base,
                               const int64_t* cam_diag_off, double* blocks, double* camsq, int n_cameras, hipStream_t stream, const double* extra, bool few) {
  if (n_cameras > 0 && !few) {   // cameras of many items: a workgroup per camera
    hipLaunchKernelGGL(bal_camera_finish_wide_kernel, dim3(n_cameras), dim3(64 * kInvertGatherWaves), 0, stream, parts, cam_item_ptr, D_f, cam_pos,
                       cam_base, cam_diag_off, blocks, camsq, n_cameras, extra);
    return hipGetLastError();
  }
  if (n_cameras > 0) hipLaunchKernelGGL(bal_camera_finish_kernel, dim3((n_cameras + kPerWave - 1) / kPerWave), dim3(64), 0, stream, parts, cam_item_ptr, D_f, cam_pos,
                                        cam_base, cam_diag_off, blocks, camsq, n_cameras, extra);
  return hipGetLastError();
}

static hipError_t CameraChunk(const ZUnits& units, const double* ring, double* acc, const int* status, hipStream_t stream) {
  if (units.count == 0) return hipSuccess;
  const int waves = (units.count + kPerWave - 1) / kPerWave;
  hipLaunchKernelGGL(bal_camera_chunk_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, units, ring, acc, status);
  return hipGetLastError();
}

static hipError_t PointTail(const PointTailArgs& T, int* n_parts, hipStream_t stream) {
  const int64_t work = std::max<int64_t>(T.n_points, T.n_f);
  const int grid = int(std::max<int64_t>(1, std::min<int64_t>((work + kPointTailBlock - 1) / kPointTailBlock, kPointTailMaxGrid)));
  if (n_parts) *n_parts = T.cost_out ? grid : 0;
  hipLaunchKernelGGL(bal_point_tail_kernel, dim3(grid), dim3(kPointTailBlock), 0, stream, T);
  return hipGetLastError();
}

}  // namespace CERES_HIP_SHAPE

// the table solver.hip dispatches through (GetBalOps, kernels_bal_common.hip)
#define CERES_HIP_CAT2(a, b) a##b
#define CERES_HIP_CAT(a, b) CERES_HIP_CAT2(a, b)
const BalOps* CERES_HIP_CAT(BalOps_, CERES_HIP_SHAPE)() {
  namespace sh = CERES_HIP_SHAPE;
  static const BalOps ops = {sh::NR, sh::NE, sh::NF, sh::NS, sh::kPairs, sh::kTilePitch, sh::kCamPart, sh::kEteiPitch, sh::kBPairs, sh::kMoPitch, sh::kHasF32 ? 1 : 0, sh::kHasCgTail ? 1 : 0,
                             sh::Fused, sh::SxRunsPipelined, sh::ReducePartials, sh::ReduceExchange, sh::StreamProbe, sh::AddFDiagonal, sh::Pack, sh::Invert, sh::CameraExchange,
                             sh::CameraItems, sh::CameraFinish, sh::CameraChunk, sh::StripFinish, sh::PointTail};
  return &ops;
}

}  // namespace chip
