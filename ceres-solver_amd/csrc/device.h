// device.h — kernel argument structs and launcher declarations shared by the .hip files.
#ifndef CERES_HIP_DEVICE_H_
#define CERES_HIP_DEVICE_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace chip {

int BalBlockFor(int mode);                   // threads per workgroup of the fused kernels (512 | 1024)
constexpr size_t kMaxLdsBytes = 160 * 1024;  // LDS per CU on gfx950
constexpr int kVecBlock = 256;
constexpr int kMaxVecGrid = 512;             // partial sums per inner product
// Grid caps of the BAL front end's kernels (a kernel walks what lies beyond its grid in a grid-stride loop; tests/test_frontend_scale_cpu.py
// reads them from here): the evaluators — kVecBlock rows per workgroup in row order, four tiles per workgroup in tile order, four
// 64-row chunks per workgroup in the gradient-only point pass (one cost partial per workgroup) — and the gradient-only camera pass
// (four camera chunks per workgroup)
constexpr int kMaxEvalGrid = 2048;
constexpr int kMaxLsCameraGrid = 4096;

// ---- one-shot peer-to-peer exchange (p2p.h: the device side; kernels_cg.hip: the stand-alone all-reduce) ----
constexpr int kP2pMaxWorld = 8;    // one node: 8 GPUs on the xGMI mesh
constexpr int kP2pChunk = 512;     // slot capacity is rounded up to a multiple of this
constexpr int kP2pFlagChunk = 8;   // arrival flags per (parity, rank): cap / 8 — a chunk of p2p_exchange_wave is at most one wavefront of slots,
                                   // and may be as few as the 8 packed sums of a 2-wide camera block (bal_invert_exchange_kernel: a chunk per camera)
constexpr int kP2pMaxGrid = 256;   // workgroups of one all-reduce (each takes every kP2pMaxGrid-th chunk): never the whole device spinning
struct P2pPeers {
  double* slots[kP2pMaxWorld];               // rank q's receive slots [2][world][cap], as mapped into THIS process
  unsigned long long* flags[kP2pMaxWorld];   // rank q's arrival flags [2][world][chunks_cap]
};
struct P2pComm {   // what a kernel needs of the communicator (by value)
  P2pPeers peers;
  int rank = 0, world = 1;
  unsigned long long epoch = 0;
  long long cap = 0;          // doubles per slot
  int chunks_cap = 0;         // flags per (parity, source rank)
  int* error_flag = nullptr;  // mapped host memory
  int* error_seen = nullptr;  // device memory
  long long timeout_ticks = 0;
  int fences = 0;             // 1: system-scope release / acquire fences around the flags as well (p2p.h)
};

// ---- fused <2,3,9> kernels (kernels_bal.hip) ------------------------------
enum BalMode { kBalSx = 0, kBalJtJx = 1, kBalJtb = 2, kBalInit = 3, kBalEte = 4, kBalBackSub = 5, kBalCgnrInit = 6, kBalColNorm = 7, kBalJx = 8, kBalSpseZ = 9,
               kBalShBlocks = 10 /* the strip's own diagonal block sums, per workgroup into BalArgs::scalar_out (shapes with a shared strip) */ };

struct CgScalars;
// The rest of a CG iteration at the end of the S.x pass, for camera spaces of at most kCgTailMax scalars (run_cg, solver.hip): the
// workgroup that flushes its partial sums LAST (an atomic ticket; nobody waits for anybody) adds the partials up, and does what
// bal_reduce_partials_kernel, cg_update_kernel and cg_finalize_direction_kernel do for such a vector in three more launches of
// ~5 us each — most of a CG iteration on a problem like problem-16-22106 (BASELINE.json configs[0]: 144 camera scalars).
constexpr int kCgTailMax = 512;     // 56 cameras: at least one thread of the last workgroup per camera scalar
constexpr int kCgTailLoads = 64;    // partial sums one thread of the last workgroup adds up (all in flight at once): workgroups <=
                                    // kCgTailLoads * (512 / camera scalars), or the iteration runs as the usual three kernels
struct CgTail {
  int enabled = 0, it = 0;
  unsigned int* ticket = nullptr;   // zero between launches
  double *x = nullptr, *r = nullptr, *p = nullptr;   // (q = S p arrives in BalArgs::y_f... the caller's z, which becomes M^-1 r)
  double* z = nullptr;
  const double* rhs = nullptr;
  const double* blocks = nullptr;   // M^-1: 81 doubles per camera, back to back
  const double* D_f = nullptr;
  CgScalars* S = nullptr;
};

struct BalArgs {
  // packed problem
  const double2* J = nullptr;   // [n_tiles][3 + nf + ns][64]
  const float4* Jf = nullptr;   // [n_tiles][6][64]  fp32 storage mode (then J is unused)
  const double2* b = nullptr;   // [n_tiles][b_pairs][64]: the slot's nr residuals (2-high rows: one double2 per slot)
  // fused re-layout: when src_values != nullptr the kernel gathers from the caller's layout and
  // writes the tiles (J_out, b_out) as it goes (first pass of a step)
  const double* src_values = nullptr;
  const double* src_b = nullptr;
  const int32_t *slot_epos = nullptr, *slot_fpos = nullptr, *slot_bpos = nullptr;   // slot_fpos < 0: a row without a camera cell
  // shapes with a shared strip: the row's shared cells (value offset, -1 none; strip offset | width << 8), common.h
  const int32_t* slot_hpos[kMaxSharedCellsPerRow] = {};
  const int32_t* slot_hdesc[kMaxSharedCellsPerRow] = {};
  double2* J_out = nullptr;
  float4* Jf_out = nullptr;
  double2* b_out = nullptr;
  const int32_t* slot_cam = nullptr;
  const int32_t* tile_pt0 = nullptr;  // first point id of each tile (points of a tile are consecutive ids)
  const uint32_t* slot_seg = nullptr;
  const int32_t* tile_kind = nullptr;
  const int32_t* tile_aux = nullptr;
  int64_t n_tiles = 0, n_slots = 0;
  // tiles this launch walks: [tile_begin, tile_end); tile_end = 0 means all.  Chunked launches (cameras not in LDS) write their
  // per-slot F^T z into a ring buffer indexed by slot - z_slot0.
  int64_t tile_begin = 0, tile_end = 0;
  // cameras not in LDS (plan.cc): tile_zbase = ring row of each tile's first spilled slot; hybrid accumulation: workgroup g walks the
  // tiles [grp_tile_ptr[g], grp_tile_ptr[g + 1]) with hyb_rows accumulator rows in LDS, flushed to ring rows z_flush_row0 + g hyb_rows ..
  const int32_t* tile_zbase = nullptr;
  const int32_t* grp_tile_ptr = nullptr;
  int hyb_rows = 0;
  // long points (plan.cc): the tiles of range g (the hybrid group, or 0 = everything) from long_ptr[g] on belong to points of more
  // than 64 observations; the streaming kernels take them in rounds of kRoundWaves words, sequence by sequence (common.h, plan.cc)
  int long_behind = 0;   // 0: long points sit among the normal tiles (chunked ring), no rounds
  const int32_t* long_ptr = nullptr;
  const int32_t* round_ptr = nullptr;    // per range: its sequences
  const int32_t* seq_ptr = nullptr;      // per sequence: its rounds
  int n_seq = 0;                         // sequences of all ranges
  const int32_t* round_flag = nullptr;
  const uint32_t* round_word = nullptr;
  int64_t z_flush_row0 = 0;
  int pq_accumulate = 0;       // kJtJx chunked: pq_out[workgroup] += instead of = (later chunks of one application)
  const int32_t* pt_pos = nullptr;   // nullptr => ne*p (ne: the shape's point width)
  const int32_t* cam_pos = nullptr;  // nullptr => cam_base + nf*c   (relative to the F base pointer)
  int cam_base = 0;
  int sh_pos[kMaxSharedScalars] = {};   // the strip's scalars in the F-space vectors (shapes with a shared strip)
  // CGNR on internally numbered points: x_e / y_e / point_blocks are internal (pt_pos == nullptr) while D_e, lm_diag_e, lm_D_e are the
  // caller's: d_pos[p] = the caller's offset of internal point p (nullptr: the same offsets as x_e); D_int_out: D_e in the internal order
  const int32_t* d_pos = nullptr;
  double* D_int_out = nullptr;
  // vectors: *_e indexed by pt_pos, *_f by cam_pos
  const double* x_e = nullptr;
  const double* x_f = nullptr;
  int flags = 0;                    // 1: per-lane point-space accesses in JtJx, 2: blocked tile walk (experiments); 4: plain (not non-temporal) tile stores
  double* y_e = nullptr;
  const double* D_e = nullptr;  // nullptr => no regularisation on the point part
  // fused LM diagonal (lm_radius > 0): D_e is formed in the kernel from the point block's own diagonal
  double lm_radius = 0.0, lm_min = 0.0, lm_max = 0.0;
  double* lm_diag_e = nullptr;  // clamped diag(J^T J), point part (indexed like x_e)
  double* lm_D_e = nullptr;     // D, point part
  // per-point ne x ne inverses, packed upper triangle at a pitch of BalOps::etei_pitch doubles (3-wide points: 6 doubles / point)
  double* etei = nullptr;
  double* point_blocks = nullptr;         // dense ne x ne output (CGNR JACOBI) or nullptr
  const int64_t* pt_diag_off = nullptr;   // offsets into point_blocks; nullptr => ne*ne*p
  double* Mo = nullptr;                   // [n_slots][mo_pitch] symmetric nr x nr per observation, packed upper triangle (2-high rows: m00 m01 m11 m01) (kInit)
  const int32_t* mo_index = nullptr;      // record of each slot in Mo (nullptr: the slot itself; hybrid plans: the slot's row)
  int have_b = 0;
  // camera accumulation
  double* partials = nullptr;    // [grid][n_acc]   (LDS mode)
  double* zbuf = nullptr;        // [rows][nf]     (cameras do not fit in LDS: the ring of spilled / flushed F^T z rows, second pass by camera)
  double* strip_sums = nullptr;  // accumulators outside LDS, shapes with a strip: the strip's ns entries of the global sums (zeroed per application)
  int n_acc = 0;                 // nf * n_cameras + ns: the camera-space accumulator entries (the strip's behind the cameras')
  // LDS mode, streaming kernels: x_f of the n_xhot most observed cameras staged in LDS behind the accumulators (BalPlan::xhot_cam;
  // the slot word's row field = row + 1)
  const int32_t* xhot_cam = nullptr;
  int n_xhot = 0;
  // kBackSub / kJx (no accumulators in LDS): the whole camera part of x staged in LDS, nf * n_cameras scalars (0: gathered from
  // memory; the dispatcher clears it for every other mode)
  int x_lds_scalars = 0;
  double* scalar_out = nullptr;  // kJx: one partial sum per workgroup
  // kBackSub: the reduced solution z is also the camera part of x (ImplicitSchurComplement::BackSubstitute copies it): done by the kernel
  const double* copy_src = nullptr;
  double* copy_dst = nullptr;
  int copy_n = 0;
  // kBackSub as the last kernel of an LM step: store -x (the step) instead of x and raise *nonfinite if an entry is not
  // finite (LevenbergMarquardtStrategy::ComputeStep's IsArrayValid + negation, I/levenberg_marquardt_strategy.cc:123-153)
  int negate_out = 0;
  int* nonfinite = nullptr;
  // Speculative tail of an LM step: the kernel is enqueued BEFORE the host knows whether CG has ended, and does nothing
  // unless *run_after_cg is a terminal status that lets the solution be used (CgStatusAllowsSolution)
  const int* run_after_cg = nullptr;
  double* pq_out = nullptr;      // kJtJx: partial x_e . y_e of the point part, one per workgroup (CG's p.q without a pass of its own)
  const int* status = nullptr;   // CG status word; non-zero => kernel returns immediately
  // first pass of a solve (kInit / kCgnrInit; neither raises them): the step's finite-step and factorization flags, two adjacent ints,
  // are cleared here instead of by a memset command in front of the pass (a fill kernel and its launch per step)
  int* clear_flags = nullptr;
  // Point tail (design/20_point_tail.md).  kSx: the lane or wave that holds a point's finished sum E^T F x stores it at
  // u_out[ne * pt ..], the plan's point order (nullptr: off).  kInit: likewise the point's E^T b into etb_out.  kBackSub gated by run_after_cg: the
  // pass also stays out when the point tail takes the solve (PointTailTakes of *run_after_cg and *skip_updates; nullptr: no such test)
  double* u_out = nullptr;
  double* etb_out = nullptr;
  const int* skip_updates = nullptr;
  CgTail tail;                   // kSx, pipelined kernel, every camera's accumulator in LDS: finish the CG iteration (see CgTail)
};

// Fused LM diagonal of the camera columns, applied by bal_invert_kernel (radius > 0 to enable).
struct LmFuse {
  double radius = 0.0, min_d = 0.0, max_d = 0.0;
  const double* camsq = nullptr;     // [nf c + k] column norms; nullptr => the block's own diagonal (F^T F blocks)
  const int32_t* cam_pos = nullptr;  // nullptr => cam_base + nf c
  int cam_base = 0;
  double* diag_f = nullptr;
  double* D_f = nullptr;
};

// The robust loss of the BAL front end (robust_loss.h; ceres_hip_bal_set_loss).  type: CERES_HIP_LOSS_* of include/ceres_hip.h, or
// kLossNone; a, b, c: the constants the reference's constructor of that loss derives from its parameters (include/ceres/loss_function.h);
// k: ScaledLoss's factor.  Kernels that take one are instantiated twice: kLossNone runs the squared-loss instantiation.
constexpr int kLossNone = -1, kLossTrivial = 0, kLossHuber = 1, kLossSoftLOne = 2, kLossCauchy = 3, kLossArctan = 4, kLossTolerant = 5,
              kLossTukey = 6;
struct LossParams {
  int32_t type = kLossNone;
  double a = 0.0, b = 0.0, c = 0.0, k = 1.0;
};

// Work items of the camera-block kernel: <= kCamChunk consecutive observations of one camera.
struct CamItems {
  const int32_t *cam = nullptr, *begin = nullptr, *end = nullptr;
  int count = 0;
  int64_t observations = 0;   // of all items together (the launcher picks the kernel by the mean item length)
  // <2,3,9> with the device evaluator (bal_frontend.inc): the pass EVALUATES its F cells instead of reading them — the records the
  // tile-order evaluator left ([state | scale] per camera / point), and the point and pixel of every entry of the camera-major list
  const double *ev_cam_pack = nullptr, *ev_pt_pack = nullptr;
  const int32_t* ev_pt = nullptr;
  const double2* ev_obs = nullptr;
  LossParams ev_loss;   // the evaluated F cells are corrected by this loss (kLossNone: the squared loss)
};
struct CamGather {
  const double* parts = nullptr;          // nullptr: the blocks are already assembled in memory
  const int32_t* cam_item_ptr = nullptr;
  const double* D_f = nullptr;            // added squared to the diagonal (indexed through cam_pos)
  const int32_t* cam_pos = nullptr;
  int cam_base = 0;                       // cam_pos == nullptr: camera c at cam_base + nf c
  int want_sq = 0;                        // SCHUR items: the fused LM diagonal takes the camera columns' square sums from the items
  int few = 0;                            // every camera has a handful of items at most: seven cameras per wavefront gather their own
  const double* extra = nullptr;          // [nf nf c + nf a + b] raw sums added to the camera's block (rows outside the tiles: LaunchRemCameraBlocks)
  const double* packed = nullptr;         // [cam_part c + e] the cameras' item sums already added up, and summed over ranks (camera_exchange); parts unused
};
// Camera-major pass of one chunk (cameras not in LDS): acc[nf c + k] += sum over the unit's entries of ring[nf slot + k].
struct ZUnits {
  const int32_t *cam = nullptr, *begin = nullptr, *end = nullptr, *shared = nullptr;  // units [first, first + count)
  const int32_t* slot = nullptr;                                                       // entry -> ring row (chunk-relative)
  int first = 0, count = 0;
};

// accumulator entry -> place in the F-space vectors (bal_reduce_partials_kernel): camera c's scalars at cam_pos[c] (nullptr: cam_base +
// nf c), behind them the shared strip's at sh_pos
struct FMap {
  const int32_t* cam_pos = nullptr;
  int cam_base = 0, n_cam_scalars = 0;
  int sh_pos[kMaxSharedScalars] = {};
};

// the shared column blocks of a plan: strip offset, width, where the block goes in the F-block store, the F-space position of its first scalar
struct StripBlocks {
  int count = 0;
  int off[kMaxSharedScalars] = {}, width[kMaxSharedScalars] = {}, pos[kMaxSharedScalars] = {};
  int64_t out[kMaxSharedScalars] = {};
};

// The point tail of a short ITERATIVE_SCHUR solve (design/20_point_tail.md): U_p = sum_k alpha_k u_k[p] over the S.x passes' captured
// sums, y_p = (E^T E + D^2)^-1 (E^T b - U_p), x = (y, z) (negated for an LM step), and the model cost change from point-space and
// camera-space vectors alone.  Runs only if PointTailTakes(S->status, S->n_updates).
struct PointTailArgs {
  int n_points = 0, n_f = 0;
  const int32_t* pt_pos = nullptr;   // nullptr: ne * p
  const double* etei = nullptr;      // packed inverses, BalOps::etei_pitch doubles per point
  const double* etb = nullptr;       // E^T b, indexed like y_e
  const double* u_hist = nullptr;    // [kPointTailMaxIterations][u_stride], ne doubles per point in the PLAN's point order (ne * p)
  int64_t u_stride = 0;
  const double *D_e = nullptr, *D_f = nullptr;   // nullptr: no regularisation
  const double *z = nullptr, *rhs = nullptr, *r = nullptr;   // camera space: CG's solution, right-hand side and residual
  double *y_e = nullptr, *y_f = nullptr;
  int negate = 0;
  int* nonfinite = nullptr;          // negate: raised when an entry of the step is not finite
  const CgScalars* S = nullptr;
  double* cost_out = nullptr;        // one partial of the model cost change per workgroup (nullptr: not wanted)
};
constexpr int kPointTailBlock = 256;
constexpr int kPointTailMaxGrid = 1023;   // partials that fit the read-back image beside the remainder's (2 kMaxVecGrid)

// The fused kernels are compiled once per SHAPE (camera width nf, shared strip ns: common.h, kernels_bal.inc — one translation unit
// per shape); this is one shape's launchers.
struct BalOps {
  // tile_pitch: double2 elements per tile; cam_part: doubles per item of the camera-major pass; etei_pitch: doubles per point in the store
  // of packed (E^T E)^-1; b_pairs: double2 per slot of the residual tiles; mo_pitch: doubles per M_o record
  int nr, ne, nf, ns, pairs, tile_pitch, cam_part, etei_pitch, b_pairs, mo_pitch, has_f32, has_cg_tail;
  hipError_t (*fused)(int mode, const BalArgs& A, bool lds, int grid, hipStream_t stream);
  // whether fused(kBalSx, A, lds, ..) runs the pipelined kernel — the one that can finish a CG iteration (A.tail)
  bool (*sx_runs_pipelined)(const BalArgs& A);
  // y_f[pos(i)] = sum over the workgroups' partials (+ D_f^2 x_f); pq_out != nullptr: also partial x_f . y_f, one per workgroup (*n_pq of
  // them; needs x_f); sum_out: *sum_out = sum(sum_in[0 .. n_sum_in)), see the kernel
  hipError_t (*reduce_partials)(const double* partials, int nparts, int n_acc, const FMap& map, const double* D_f, const double* x_f,
                                double* y_f, const int* status, double* pq_out, int* n_pq, hipStream_t stream, const double* sum_in,
                                int n_sum_in, double* sum_out);
  // the same for a SHARDED instance with the sum over ranks inside (p2p.h; one launch instead of reduction, all-reduce kernel and
  // add_f_diagonal): y_f = sum over ranks (sum over the workgroups' partials) + D_f^2 x_f over the n_fv F-space positions; *sum_out
  // (position n_fv) likewise summed over ranks.  Cameras back to back in F space only (map.cam_pos == nullptr).
  hipError_t (*reduce_exchange)(const double* partials, int nparts, int n_acc, int n_fv, const FMap& map, const double* D_f, const double* x_f,
                                double* y_f, const int* status, double* pq_out, int* n_pq, hipStream_t stream, const double* sum_in,
                                int n_sum_in, double* sum_out, const P2pComm& comm, int grid_cap);
  hipError_t (*stream_probe)(const double2* J, int64_t n_tiles, int grid, double* out, hipStream_t stream);
  hipError_t (*add_f_diagonal)(int n_acc, const FMap& map, const double* D_f, const double* x_f, double* y_f, const int* status,
                               double* pq_out, int* n_pq, hipStream_t stream);
  hipError_t (*pack)(const BalArgs& A, hipStream_t stream);   // A.src_values / src_b / slot_* / J_out (Jf_out) / b_out set
  hipError_t (*invert)(double* blocks, const int64_t* cam_diag_off, int n_cameras, int* fail_flag, const LmFuse& lm, const CamGather& gather,
                       hipStream_t stream);
  // sharded: every camera's items added up and summed over ranks (p2p.h: slots cam_part c + e, chunks ceil(cam_part / 64) c + q), left
  // packed — cam_part doubles per camera — for invert (CamGather::packed)
  hipError_t (*camera_exchange)(const double* parts, const int32_t* cam_item_ptr, int n_cameras, const double* extra, double* packed,
                                const P2pComm& comm, int grid_cap, hipStream_t stream, bool few /* a handful of items per camera */);
  // Per-camera blocks in two steps: every item (<= kCamChunk observations of one camera) leaves its upper-triangle sums + nf column
  // square sums in parts[item][cam_part]; the items of a camera (cam_item_ptr) are then added in list order either by camera_finish
  // (raw sums to memory, + D_f^2 if given) or by the load phase of invert (CamGather).
  hipError_t (*camera_items)(bool schur, const double* values, const CamItems& items, const int32_t* cam_fpos, const int32_t* cam_slot,
                             const double* Mo, double* parts, hipStream_t stream);
  hipError_t (*camera_finish)(const double* parts, const int32_t* cam_item_ptr, const double* D_f, const int32_t* cam_pos, int cam_base,
                              const int64_t* cam_diag_off, double* blocks, double* camsq, int n_cameras, hipStream_t stream, const double* extra,
                              bool few /* every camera has a handful of items at most: kPerWave cameras per wavefront */);
  hipError_t (*camera_chunk)(const ZUnits& units, const double* ring, double* acc, const int* status, hipStream_t stream);
  // shapes with a shared strip: the packed upper triangle of the strip's ns x ns matrix from the workgroups' partial sums (kBalShBlocks),
  // cut into the shared blocks' dense diagonal blocks (+ D^2) in the F-block store
  hipError_t (*strip_finish)(const double* parts, int nparts, const StripBlocks& sb, const double* D_f, double* blocks, hipStream_t stream);
  // *n_parts: the partials it leaves in T.cost_out when it runs (0 without cost_out)
  hipError_t (*point_tail)(const PointTailArgs& T, int* n_parts, hipStream_t stream);
};
const BalOps* GetBalOps(int nr, int ne, int nf, int ns);   // nullptr: not compiled (common.h: BalShapeCompiled)
// the dynamic-LDS ceiling of a kernel, raised once per (kernel, device)
hipError_t AllowMaxLds(const void* kernel);

// ---- generic kernels (kernels_generic.hip) --------------------------------
// Work ITEMS of the grouped generic kernels over heavy column blocks (the cameras of a BAL-like problem): at most kGenItem consecutive
// cells of ONE block's transpose list, never cutting the cells a block has inside one chunk apart.  A wave per item leaves the item's
// partial result in `scratch` ([item][kGenItemValues]); a second kernel adds a block's items in list order (deterministic).  Without
// them one wave walks a popular camera's thousands of cells alone and the kernel lasts as long as that chain (1.3 ms on the Ladybug shape).
constexpr int kGenItem = 128;
constexpr int kGenItemValues = 55;   // a 10 x 10 upper triangle
struct GenItems {
  int count = 0, first_block = 0, nblocks = 0;
  const int32_t *block = nullptr, *t0 = nullptr, *t1 = nullptr;   // per item
  const int32_t* block_ptr = nullptr;                             // per block of the range: its items [block_ptr[q], block_ptr[q + 1])
  double* scratch = nullptr;
};
struct GenStructure {
  int nrb = 0, ncb = 0, nelim = 0, nrbe = 0, num_rows = 0, num_cols = 0, nce = 0, ncf = 0;
  const int32_t *rsz = nullptr, *rpos = nullptr, *rptr = nullptr, *ccol = nullptr, *cval = nullptr;
  const int32_t *csz = nullptr, *cpos = nullptr;
  const int32_t *tptr = nullptr, *trow = nullptr, *tcell = nullptr;
  // per transpose entry, what the itemized kernels would otherwise chase through three more arrays: the cell's value offset, its row
  // block's first scalar row, and the row block's height | (1 << 8 if the cell is the E cell of its row)
  const int32_t *tval = nullptr, *trpos = nullptr, *tinfo = nullptr;
  const int32_t *row_block_of = nullptr, *col_block_of = nullptr, *row_e_block = nullptr;
  const int64_t *diag_off_all = nullptr, *diag_off_e = nullptr, *diag_off_f = nullptr;
  // chunk = the (contiguous) rows of one E block: SchurEliminator's unit of work (I/schur_eliminator_impl.h:87-181)
  const int32_t *chunk_start = nullptr, *chunk_size = nullptr;
  // hints for the GROUPED kernels (L lanes per column block / chunk, kernels_generic.hip): largest block sizes per part, lanes per group
  // chosen from the average number of cells per block (power of two, 4 .. 64); 0 = use the thread-per-scalar kernels
  int max_csz_e = 0, max_csz_f = 0, max_csz = 0, max_rsz = 0;
  int lanes_e = 0, lanes_f = 0, lanes_all = 0, lanes_chunk = 0;
  GenItems items;   // over the F blocks (all blocks without an elimination order); count == 0: none
};
enum GenPart { kAll = 0, kE = 1, kF = 2 };

// y += A_part x   (x, y are the base pointers of the part's own index space)
hipError_t LaunchGenRightMultiply(const GenStructure& G, const double* values, int part, const double* x, double* y,
                                  const int* status, hipStream_t stream);
// y += A_part^T x
hipError_t LaunchGenLeftMultiply(const GenStructure& G, const double* values, int part, const double* x, double* y,
                                 const int* status, hipStream_t stream);
// blocks = blockdiag(A_part^T A_part) (+ D^2 if D != nullptr; D is the FULL num_cols vector)
hipError_t LaunchGenBlockDiagonal(const GenStructure& G, const double* values, int part, const double* D,
                                  double* blocks, int64_t total_entries, hipStream_t stream);
// x[j] = |A_j|^2
hipError_t LaunchGenSquaredColumnNorm(const GenStructure& G, const double* values, double* x, hipStream_t stream);
// In-place SPD inverse (upper triangle authoritative) of nblocks dense blocks; blocks
// [first_block, first_block + nblocks) of the column-block list, offsets relative to off[0].
hipError_t LaunchGenInvertBlocks(const GenStructure& G, int first_block, int nblocks, const int64_t* diag_off,
                                 double* blocks, int* fail_flag, hipStream_t stream);
// Per chunk (E block e, rows of the chunk): w = (E^T E + D^2)^-1 E^T t over the chunk's rows (ete_inv: the inverted blocks), then
// t_r -= E_r w on those rows (update_t) and / or x_e[cpos(e) ..] = w (x_e != nullptr).  One launch for what LeftMultiplyE, the block
// diagonal apply and RightMultiplyE do in ImplicitSchurComplement::RightMultiplyAndAccumulate / UpdateRhs / BackSubstitute
// (I/implicit_schur_complement.cc:106-144, 208-276).  Returns hipErrorNotSupported when the block sizes exceed the grouped kernels'
// (the caller then runs the separate passes).
hipError_t LaunchGenChunkProject(const GenStructure& G, const double* values, const double* ete_inv, double* t_rows, int update_t,
                                 double* x_e, const int* status, hipStream_t stream);
// z_rows (rows of the chunks) = F x_f - E (E^T E)^-1 E^T F x_f in one launch (the row-space half of S x); hipErrorNotSupported beyond the
// compiled block sizes.  Rows WITHOUT an E block are not touched: LaunchGenRightMultiplyFrom(first_row = their first scalar row).
hipError_t LaunchGenChunkSx(const GenStructure& G, const double* values, const double* ete_inv, const double* x_f, double* z_rows,
                            const int* status, hipStream_t stream);
// LaunchGenRightMultiply over the scalar rows [first_row, num_rows)
hipError_t LaunchGenRightMultiplyFrom(const GenStructure& G, const double* values, int part, int first_row, const double* x, double* y,
                                      const int* status, hipStream_t stream);
// y += blockdiag x over column blocks [first_block, first_block+nblocks); vectors start at that block.
hipError_t LaunchGenBlockDiagonalApply(const GenStructure& G, int first_block, int nblocks, const int64_t* diag_off,
                                       const double* blocks, const double* x, double* y, const int* status,
                                       hipStream_t stream);
// blocks(j)(a,a) += D[col]^2 over column blocks [first_block, first_block+nblocks); D is the FULL vector.
hipError_t LaunchAddBlockDiagonalSquares(const GenStructure& G, int first_block, int nblocks, const int64_t* diag_off,
                                         const double* D, double* blocks, hipStream_t stream);
// Diagonal blocks of the Schur complement (SchurEliminator::Eliminate into a
// block-diagonal lhs): needs the inverted E^T E blocks.  D may be nullptr; add_f_diag
// controls whether D_f^2 is added (sharded runs add it after the all-reduce).
hipError_t LaunchGenSchurJacobi(const GenStructure& G, const double* values, const double* ete_inv, const double* D,
                                int add_f_diag, double* blocks, int64_t total_entries, hipStream_t stream);
// Dense S (upper block triangle) and nothing else; rhs comes from the ISC path.
// explicit Schur complement (f2): mirror the stored upper block triangle; y = S x; diagonal blocks of S
hipError_t LaunchGenSymmetrizeDense(const GenStructure& G, double* lhs, hipStream_t stream);
hipError_t LaunchGenDenseSymv(const double* S, int n, const double* x, double* y, const int* status, hipStream_t stream);
hipError_t LaunchGenExtractDiagBlocks(const GenStructure& G, const double* S, const int64_t* diag_off_f, double* blocks,
                                      hipStream_t stream);
hipError_t LaunchGenSchurDense(const GenStructure& G, const double* values, const double* ete_inv, const double* D,
                               double* lhs, hipStream_t stream);

// ---- remainder rows of the fused path: rows without a point cell, R = their own GenStructure (kernels_generic.hip); nf = the camera width ----
hipError_t LaunchRemCameraBlocks(const GenStructure& R, const double* values, const int32_t* cam_block, int n_cameras, int nf, double* out, hipStream_t stream);
// y_f[pos(c) ..] += F_R^T t over the remainder rows' cells on the nf-wide camera blocks (one wavefront per camera)
// (cam_pos: each camera's offset in the F-space vectors, or nullptr: back to back from cam_base)
hipError_t LaunchRemLeftMultiply(const GenStructure& R, const double* values, const int32_t* cam_block, const int32_t* cam_pos, int cam_base, int n_cameras,
                                 int nf, const double* t_rows, double* y_f, const int* status, hipStream_t stream);
hipError_t LaunchRemAddDiag(const double* blocks, const int32_t* cam_pos, int cam_base, int n_cameras, int nf, double* y, hipStream_t stream);
hipError_t LaunchGatherRows(const double* in, const int32_t* map, int n, double* out, hipStream_t stream);   // out[r] = in[map[r]]
hipError_t LaunchRemModelCost(const double* m, const double* f, int n, int mode, double* out, hipStream_t stream);

// ---- explicit Schur complement solvers (kernels_schur.hip) ------------------
struct SchurPairs {  // device image of SchurStorage (common.h)
  int npairs = 0;
  const int32_t *pair_i = nullptr, *pair_j = nullptr, *row_ptr = nullptr, *col_ptr = nullptr, *col_pair = nullptr;
  const int64_t *pair_off = nullptr, *trip_ptr = nullptr;
  const int32_t *trip_e = nullptr, *trip_k1 = nullptr, *trip_k2 = nullptr, *cell_row = nullptr;
  // work items of the elimination (common.h): item -> pair, triples [t0, t1), offset of its partial block in `scratch`
  int n_items = 0;
  const int32_t *item_pair = nullptr, *pair_item_ptr = nullptr;
  const int64_t *item_t0 = nullptr, *item_t1 = nullptr, *item_off = nullptr;
  double* scratch = nullptr;
  int64_t total_values = 0;   // values of the block-sparse S
};
// S (block-sparse, upper block triangle) = SchurEliminator::Eliminate; D may be nullptr (then no D_f^2 on the diagonal)
hipError_t LaunchSchurSparseEliminate(const GenStructure& G, const SchurPairs& P, const double* values, const double* ete_inv,
                                      const double* D, double* S, hipStream_t stream);
// dense lhs (num_cols_f^2, zeroed by the caller) <- the stored blocks of S (`total` values): DENSE_SCHUR eliminates into the block-sparse
// storage (a gather per block) and factors the dense image
hipError_t LaunchSchurBlocksToDense(const GenStructure& G, const SchurPairs& P, const double* S, int64_t total, double* lhs, hipStream_t stream);
// y (+)= S x   BlockRandomAccessSparseMatrix::SymmetricRightMultiplyAndAccumulate
hipError_t LaunchSchurSparseSymv(const GenStructure& G, const SchurPairs& P, const double* S, const double* x, double* y,
                                 const int* status, int accumulate, hipStream_t stream);
hipError_t LaunchSchurSparseDiag(const GenStructure& G, const SchurPairs& P, const double* S, const int64_t* diag_off_f, double* blocks,
                                 int64_t total, hipStream_t stream);
// dense SPD n x n, upper triangle authoritative: in-place factor (L in the lower triangle), then x <- A^-1 x
hipError_t LaunchDenseCholesky(double* A, int n, int* fail_flag, hipStream_t stream);
hipError_t LaunchDenseCholeskySolve(const double* A, int n, double* x, hipStream_t stream);

// ---- covariance (kernels_covariance.hip, covariance.inc; design/17_covariance.md) ------------------
// C_p (9 doubles per free point, symmetric) -> C_p^-1 in place by the Cholesky factorisation of the unit-diagonal-scaled block;
// pivot[p] = its smallest pivot, 0 where a diagonal entry or a pivot is not positive (the block is then zeroed: never a NaN)
hipError_t LaunchCovPointFactor(int n_points, double* blocks, double* pivot, hipStream_t stream);
// out[0] = min over i < count of v[i stride] (squared if square != 0), out[1] = the first index that attains it; one workgroup, fixed order
hipError_t LaunchCovMin(const double* v, int64_t count, int64_t stride, int square, double* out, hipStream_t stream);
// lam = diag(S)^-1/2, S <- Lambda S Lambda (every entry); *flag = 1 when a diagonal entry is not positive and finite (its lam is 0)
hipError_t LaunchCovScale(double* S, int n, double* lam, int* flag, hipStream_t stream);
// A: the factor L of LaunchDenseCholesky in its lower triangle (overwritten by L^-1).  W (n x n) <- Lambda (L L^T)^-1 Lambda, exactly
// symmetric; W is also the scratch of the triangular inversion.
hipError_t LaunchCovInverseFromFactor(double* A, int n, const double* lam, double* W, hipStream_t stream);
enum CovBlockKind { kCovConstPoint = 0, kCovPoint = 1, kCovCamera = 2, kCovConstCamera = 3 };
struct CovBlocksArgs {
  int n_pairs = 0, n = 0;                   // n = num_cols_f, the pitch of sinv
  const int32_t *code_a = nullptr, *code_b = nullptr;   // per pair: 4 x (index among the free points / cameras) + CovBlockKind
  const int64_t* out_off = nullptr;         // per pair: where its dim(a) x dim(b) row-major block starts in out
  double* out = nullptr;
  const double *values = nullptr, *cinv = nullptr, *sinv = nullptr;   // caller-layout Jacobian, C_p^-1 (9 per free point), S^-1
  // per free point its observations by free cameras, entries [pt_ptr[q], pt_ptr[q + 1]): E cell, F cell, column of the camera
  const int32_t *pt_ptr = nullptr, *ent_epos = nullptr, *ent_fpos = nullptr, *ent_ccol = nullptr;
};
// one wavefront per pair; cw = 9 or 10 (hipErrorInvalidValue otherwise)
hipError_t LaunchCovBlocks(const CovBlocksArgs& P, int cw, hipStream_t stream);
// The blocks pass of a handle with shared intrinsics (kernels_covariance_shared.hip; design/28_shared_covariance.md): three block kinds,
// points (3), poses (6) and groups (3), and per row two camera-side cells — a pose cell (none when the pose is constant) and a group cell.
enum CovSharedKind { kCovSharedPoint = 0, kCovSharedPose = 1, kCovSharedConstPose = 2, kCovSharedGroup = 3 };
struct CovSharedBlocksArgs {
  int n_pairs = 0, n = 0;                   // n = num_cols_f = 6 (free cameras) + 3 (groups), the pitch of sinv
  // per pair: 4 x index + CovSharedKind; the index of a point is the point, of a pose or a group its first scalar column in sinv
  const int32_t *code_a = nullptr, *code_b = nullptr;
  const int64_t* out_off = nullptr;         // per pair: where its dim(a) x dim(b) row-major block starts in out
  double* out = nullptr;
  const double *values = nullptr, *cinv = nullptr, *sinv = nullptr;   // caller-layout Jacobian, C_p^-1 (9 per point), S^-1
  // per point EVERY row of it, entries [pt_ptr[q], pt_ptr[q + 1]): E cell; pose cell and its first column in sinv (-1, -1: the pose is
  // constant); group cell and its first column in sinv
  const int32_t *pt_ptr = nullptr, *ent_epos = nullptr, *ent_ppos = nullptr, *ent_pcol = nullptr, *ent_gpos = nullptr, *ent_gcol = nullptr;
};
// one wavefront per pair
hipError_t LaunchCovSharedBlocks(const CovSharedBlocksArgs& P, hipStream_t stream);

// ---- CLUSTER_JACOBI (kernels_cluster.hip): one dense factor per cluster of F blocks ------------------
// Clusters of at most kClusterLdsDim scalars are factored and applied one workgroup per cluster with the matrix in LDS
// (128 x 129 doubles = 129 KiB of the CU's 160); larger ones go through LaunchDenseCholesky / LaunchDenseCholeskySolve.
constexpr int kClusterLdsDim = 128;
struct ClusterLayout {   // device image of ClusterLayoutHost (common.h)
  int num_clusters = 0, n = 0;   // n = num_cols_f
  const int32_t *perm = nullptr, *cl_off = nullptr, *block_cluster = nullptr, *block_loc = nullptr;
  const int64_t* mat_off = nullptr;
  const int32_t* small_list = nullptr;   // the clusters of at most kClusterLdsDim scalars
  int n_small = 0, small_max_dim = 0;
};
// mats (zeroed by the caller) <- the stored blocks of the cluster pairs, both triangles of every cluster's matrix
hipError_t LaunchClusterAssemble(const GenStructure& G, const SchurPairs& P, const ClusterLayout& C, const double* S, int64_t total,
                                 double* mats, hipStream_t stream);
// in-place Cholesky of the small clusters (L in the lower triangle); a pivot that is not positive raises *fail_flag
hipError_t LaunchClusterFactorSmall(const ClusterLayout& C, double* mats, int* fail_flag, hipStream_t stream);
// y[perm] = (L L^T)^-1 x[perm] over the small clusters; status: CG status word (no-op once it is non-zero), may be nullptr
hipError_t LaunchClusterSolveSmall(const ClusterLayout& C, const double* mats, const double* x, double* y, const int* status,
                                   hipStream_t stream);
// xc[q] = x[perm[q]] / y[perm[q]] = xc[q] for q in [q0, q0 + len)
hipError_t LaunchClusterGather(const int32_t* perm, int q0, int len, const double* x, double* xc, hipStream_t stream);
hipError_t LaunchClusterScatter(const int32_t* perm, int q0, int len, const double* xc, double* y, hipStream_t stream);

// ---- vector kernels + device-resident CG (kernels_cg.hip) ------------------
hipError_t LaunchSet(double* x, double v, int64_t n, hipStream_t stream);
hipError_t LaunchAxpby(double a, const double* x, double b, const double* y, double* z, int64_t n, hipStream_t stream);
// y = D^2 .* x  (D may be nullptr => y = 0)
hipError_t LaunchSquareScale(const double* D, const double* x, double* y, int64_t n, const int* status, hipStream_t stream);
// y += D^2 .* x
hipError_t LaunchAddSquareScale(const double* D, const double* x, double* y, int64_t n, const int* status, hipStream_t stream);
// out[0] = x . y  (two-stage, deterministic); partials has kMaxVecGrid doubles
hipError_t LaunchDot(const double* x, const double* y, int64_t n, double* partials, double* out, hipStream_t stream);
// D = sqrt(clamp(diag, lo, hi) / radius); diag is clamped in place (LevenbergMarquardtStrategy::ComputeStep,
// I/levenberg_marquardt_strategy.cc:84-96)
hipError_t LaunchLmDiagonal(double* diag, double lo, double hi, double radius, double* D, int64_t n, hipStream_t stream);
// x = -x and *nonfinite += number of non-finite entries (IsArrayValid + negation, :124-132)
// CGNR: y.g + y.r + |D y|^2 over [begin, end) as per-workgroup partials (nparts <= kMaxVecGrid)
// neg_out (optional): also neg_out[i] = -y[i] over the range and *nonfinite += (entries that are not finite) — the LM step's
// finite check + negation, read from the CG solution in the same pass
// gate (optional): a CG status word; the kernel does nothing unless CgStatusAllowsSolution(*gate) (speculative LM tail)
// CGNR on internally numbered points (solver.hip): the CG vectors hold internal point p at [3 p, 3 p + 3), the caller's vectors at
// pt_pos[p]; D_e = the point part of D in the internal order
struct PointPerm {
  const int32_t* pt_pos = nullptr;
  const double* D_e = nullptr;
  int64_t n_e = 0;
};
hipError_t LaunchCgnrModelCost(const double* y, const double* g, const double* r, const double* D, int64_t begin, int64_t end,
                               double* partials, int* nparts, hipStream_t stream, double* neg_out = nullptr, int* nonfinite = nullptr,
                               const int* gate = nullptr, const PointPerm& perm = PointPerm());
// the 3-wide point blocks [0, n_e) between the caller's order and the internal one (to_internal: out[i] = in[pos(i)]); [n_e, n) copied
hipError_t LaunchPermutePoints(const double* in, double* out, const int32_t* pt_pos, int64_t n_e, int64_t n, bool to_internal, hipStream_t stream);
hipError_t LaunchNegateAndCheck(double* x, int64_t n, int* nonfinite, hipStream_t stream);
// values(cell)[r][c] *= scale[col]: BlockSparseMatrix::ScaleColumns (I/block_sparse_matrix.cc:403-450)
hipError_t LaunchGenScaleColumns(const GenStructure& G, double* values, const double* scale, hipStream_t stream);
// dense[off[p] ..] (ne x ne) = the symmetric matrix whose packed upper triangle sits at packed[p * pitch ..]
hipError_t LaunchExpandSym(const double* packed, int ne, int pitch, double* dense, const int64_t* pt_diag_off, int n_points, hipStream_t stream);
// out[off[p] + k] = in[9 p + k], k < 9 (in and out must not overlap)
hipError_t LaunchScatterBlocks9(const double* in, double* out, const int64_t* off, int n_points, hipStream_t stream);

// Status word values (device side) — 0 means "keep iterating".
enum CgStatus {
  kCgRunning = 0,
  kCgConvergedZeta = 1,
  kCgConvergedResidual = 2,
  kCgMaxIterations = 3,
  kCgFailRho = 4,
  kCgFailBeta = 5,
  kCgIndefinite = 6,
  kCgFailAlpha = 7,
  kCgZeroRhs = 8,          // |b| = 0: x = 0, SUCCESS
  kCgInitialResidual = 9,  // min_num_iterations == 0 and |r0| <= tol
  kCgSetupFailed = 10,     // the preconditioner blocks could not be factorized (flag checked by the init kernels, no host round trip)
};
// Terminal CG states whose solution the caller uses: SUCCESS and NO_CONVERGENCE (solve_loaded back-substitutes for these and
// for no others; fill_summary maps the rest to FAILURE).
__host__ __device__ inline bool CgStatusAllowsSolution(int st) {
  return st != kCgRunning && st != kCgFailRho && st != kCgFailBeta && st != kCgFailAlpha && st != kCgSetupFailed;
}

struct CgScalars {
  double norm_rhs, tol_r, q_tol;
  double rho, rho_new, beta, pq, alpha, Q0, Q1, zeta, norm_r, norm_p, norm_q;
  int iter, status, min_it, max_it;
  int fail_dir, fail_step;  // failures staged by direction / step, committed by finalize
  // Fused iteration (cg_update_kernel + cg_finalize_direction_kernel): rho_i and the Q0 that iteration i tests
  // against live at index i & 1, so that no multi-workgroup kernel reads a scalar another workgroup of the same
  // launch writes (iteration i reads [i & 1] and writes [(i + 1) & 1]).
  double rho_pp[2], Q0_pp[2];
  // Point tail (design/20_point_tail.md): alpha of the first kPointTailMaxIterations completed x-updates of a solve that began at x = 0, and
  // how many x-updates the solve has completed (a failed iteration leaves x alone and is not counted); written by cg_update_kernel
  // and cg_iteration_tail where they write alpha, zeroed where the solve begins
  double alpha_hist[kPointTailMaxIterations];
  int n_updates, reserved;
};
// Does the point tail finish this solve (status and n_updates of its CgScalars)?  CG ended with a solution after at most
// kPointTailMaxIterations x-updates.  The back-substitution pass over J takes every other terminal state that lets the solution be used.
__host__ __device__ inline bool PointTailTakes(int status, int updates) {
  return (status == kCgConvergedZeta || status == kCgConvergedResidual || status == kCgMaxIterations) && updates >= 1 &&
         updates <= kPointTailMaxIterations;
}

struct CgBuffers {
  int64_t n = 0;
  // Sharded CGNR: the first n_local elements (this rank's points) are a shard, the rest
  // (cameras) are replicated.  Workgroups [0, grid_e) cover the shard, [grid_e, grid) the
  // rest; the shard's share of every inner product is collapsed into comm[slot], summed
  // over ranks by the host (ncclAllReduce) and added by the consumers.  Unsharded:
  // n_local = 0, grid_e = 0 and comm is ignored.
  int64_t n_local = 0;
  int grid = 1, grid_e = 0;
  double *x = nullptr, *r = nullptr, *p = nullptr, *z = nullptr;
  const double* rhs = nullptr;
  double* partials = nullptr;  // 4 slots * kMaxVecGrid doubles
  double* comm = nullptr;      // 4 doubles
  CgScalars* S = nullptr;      // device
  const int* setup_fail = nullptr;  // optional device flag: non-zero => CG starts in kCgSetupFailed
  // p.q of the current iteration as n_pq partial sums (written by the operator's own kernels where they have p and q
  // in registers, otherwise by cg_dot_pq_kernel into slot 1); summed in index order by cg_update_kernel
  const double* pq_parts = nullptr;
  int n_pq = 0;
  // sharded CGNR, fused iteration: one more term of p.q — the shard's share, already summed over ranks (it travelled with
  // the camera vector through the operator's all-reduce); nullptr otherwise
  const double* pq_extra = nullptr;
};
constexpr int kMaxPqParts = 2048;

// z = M^-1 r (block-diagonal, or copy when blocks == nullptr) and partial r.z
// slot 0 <- partial |rhs|^2
hipError_t LaunchCgRhsNorm(const CgBuffers& B, hipStream_t stream);
// x = 0, r = rhs, scalars initialised from slot 0 (I/conjugate_gradients_solver.h:130-159 with x0 = 0)
hipError_t LaunchCgInit(const CgBuffers& B, double q_tol, double r_tol, int min_it, int max_it, hipStream_t stream);
// z = M^-1 r (block diagonal over column blocks [first_block, ..), vectors start at scalar
// column col_begin; blocks == nullptr => identity) and slot 0 <- partial r.z
hipError_t LaunchCgPrecondition(const CgBuffers& B, const GenStructure& G, int first_block, int col_begin, int nblocks,
                                int n_local_blocks, const int64_t* diag_off, const double* blocks, hipStream_t stream);
// slot <- partial x.y over the CG vectors' range (used when the preconditioner is an operator)
hipError_t LaunchCgDotSlot(const CgBuffers& B, const double* x, const double* y, int slot, hipStream_t stream);
// Non-zero initial guess (use_spse_initialization): x is kept, r = rhs - tmp, slots 2,3 <- partial -x.(rhs + r), |r|^2
hipError_t LaunchCgInitFromGuess(const CgBuffers& B, const double* tmp, double q_tol, double r_tol, int min_it, int max_it,
                                 hipStream_t stream);
// rho = sum(slot 0); beta; p = z + beta p
hipError_t LaunchCgDirection(const CgBuffers& B, hipStream_t stream);
// slot 1 <- partial p.q  (q lives in z)
hipError_t LaunchCgDotPq(const CgBuffers& B, hipStream_t stream);
// pq = sum(slot 1); alpha; x += alpha p; unless reset: r -= alpha q, slots 2,3 <- partial Q1, |r|^2
hipError_t LaunchCgStep(const CgBuffers& B, int reset, hipStream_t stream);
// r = rhs - tmp; slots 2,3
hipError_t LaunchCgResidualReset(const CgBuffers& B, const double* tmp, hipStream_t stream);
// termination tests in the reference's order (:273-302); iter++
hipError_t LaunchCgFinalize(const CgBuffers& B, hipStream_t stream);
// Fused iteration, second half of iteration `it` (I/conjugate_gradients_solver.h:196-249 + :162-167 of the next one):
// pq = sum(pq_parts), alpha; x += alpha p; unless reset: r -= alpha q, partial Q1 / |r|^2 -> slots 2, 3 and, block by block,
// z = M^-1 r with partial r.z -> slot 0 (the next iteration's rho).  One thread per column block.
// nine_from: blocks [nine_from, nblocks) of the range are all 9 wide (handled nine lanes per block); nblocks if unknown.
// Sharded (B.grid_e > 0): the caller guarantees that blocks [0, nine_from) are exactly the shard; workgroups [0, grid_e) then take
// them and [grid_e, grid) the replicated 9-wide blocks, so that the partial sums split the way total_of() expects.
hipError_t LaunchCgUpdate(const CgBuffers& B, const GenStructure& G, int first_block, int col_begin, int nblocks,
                          const int64_t* diag_off, const double* blocks, int reset, int it, int nine_from, hipStream_t stream);
// Start of a solve with x0 = 0 in two launches: LaunchCgUpdate(..., it = 0) [x = 0, r = rhs, z = M^-1 r, partial |rhs|^2 and r.z] and
// LaunchCgBegin [scalars as LaunchCgInit sets them, p = z] — instead of rhs-norm, init, precondition, direction.
hipError_t LaunchCgBegin(const CgBuffers& B, double q_tol, double r_tol, int min_it, int max_it, hipStream_t stream);
// Fused: the termination tests of iteration `it` in the reference's order (:273-302) and, if CG goes on, the
// direction of iteration it + 1: rho = sum(slot 0), beta = rho / rho_it, p = z + beta p (:167-191).
hipError_t LaunchCgFinalizeDirection(const CgBuffers& B, int it, hipStream_t stream);
// comm[slot] = sum over the shard's workgroups of partials[slot] for slot in [first, first+count)
hipError_t LaunchCgCollapse(const CgBuffers& B, int first_slot, int count, hipStream_t stream);
// ... summed over ranks in the same launch (p2p.h)
hipError_t LaunchCgCollapseExchange(const CgBuffers& B, int first_slot, int count, const P2pComm& comm, hipStream_t stream);

// out[0] = (*flag != 0), out[1] = sum of parts[0 .. n) (one workgroup, fixed order)
hipError_t LaunchCollectScalars(const int* flag, const double* parts, int n, double* out, hipStream_t stream);
// ... summed over ranks in the same launch (p2p.h)
// image != nullptr: also the mailbox read-back of image[0 .. n_image) (out must lie inside it), stamped with `stamp`
hipError_t LaunchCollectScalarsExchange(const int* flag, const double* parts, int n, double* out, const P2pComm& comm, hipStream_t stream,
                                        const double* image = nullptr, int n_image = 0, double* host_dst = nullptr,
                                        unsigned long long* host_stamp = nullptr, unsigned long long stamp = 0);

// ---- one-shot peer-to-peer all-reduce (kernels_cg.hip) ----
// out = sum over ranks of in (n <= cap; in may alias out); comm.epoch counts this communicator's exchanges from 1 (solver.hip: next_exchange).
hipError_t LaunchP2pAllReduce(const double* in, double* out, int64_t n, const P2pComm& comm, int grid_cap, hipStream_t stream);

// host_dst[0 .. n) = src[0 .. n), then *host_stamp = stamp (both in mapped host memory): the solver's read-back "mailbox"
hipError_t LaunchMailbox(const double* src, int n, double* host_dst, unsigned long long* host_stamp, unsigned long long stamp, hipStream_t stream);

// ---- f4: BAL evaluator (kernels_evaluator.hip) ----
struct BalEvalArgs {
  int64_t n_rows = 0;                 // observations (= residual row blocks), grouped by point
  const int32_t* row_cam = nullptr;
  const int32_t* row_pt = nullptr;
  const double2* row_obs = nullptr;   // observed pixel of the row
  const double* state = nullptr;      // [3 n_p | 9 n_c]
  int64_t cam_base = 0;               // 3 n_p
  const double* scale = nullptr;      // Jacobi column scaling or nullptr
  double* residuals = nullptr;        // 2 per row, or nullptr
  double* values = nullptr;           // E cell at 6 r, F cell at 6 n_rows + 18 r
  double* partials = nullptr;         // cost partial per workgroup (<= 2048)
  LossParams loss;                    // cost = sum rho / 2, corrected residuals and Jacobian (kLossNone: the squared loss)
};
// A reduced program (constant parameter blocks, ceres_hip_bal_create_with_constant_blocks; the kernel's CONST instantiations): row_cam /
// row_pt still index the full state; a row's F cell starts at row_fpos (-1: constant camera, no cell), its E cell at 6 r when the point
// is free; row_scam / row_spt: where the block's entries start in the reduced scale vector (-1: constant block).  An argument type of
// its own: the existing instantiations keep their kernel arguments byte for byte (the tile-order evaluator sits at the SGPR limit —
// three more pointers in its arguments cost its robust instantiations two VGPRs and 16 bytes of scratch).
struct BalEvalConstArgs : BalEvalArgs {
  const int32_t* row_fpos = nullptr;
  const int32_t* row_scam = nullptr;
  const int32_t* row_spt = nullptr;
};
// Camera models of the BAL front end (CERES_HIP_CAMERA_* of include/ceres_hip.h): state doubles / Jacobian columns per camera 9 / 9,
// 10 / 10 and 10 / 9.  The quaternion cameras are [q_w q_x q_y q_z | t(3) | f k1 k2] (snavely.h, snavely_quat).
enum : int { kCamAngleAxis = 0, kCamQuaternion = 1, kCamQuaternionManifold = 2 };
// camera_model != kCamAngleAxis: 10 state doubles per camera, F cells of 2 x 10 (kCamQuaternion) or 2 x 9 (the manifold's tangent) at
// 6 n_rows + 2 width r; A.scale then indexes the tangent vector
hipError_t LaunchBalEvaluate(const BalEvalArgs& A, bool jacobian, int* nparts, hipStream_t stream, int camera_model = kCamAngleAxis);
// the Jacobian evaluation of a reduced program: a missing cell is neither scaled nor stored (cost only: LaunchBalEvaluate — it stores no cell)
hipError_t LaunchBalEvaluateConst(const BalEvalConstArgs& A, int* nparts, hipStream_t stream, int camera_model);
hipError_t LaunchBalEvaluateConstQuat(const BalEvalConstArgs& A, int grid, hipStream_t stream, int camera_model);
// the quaternion cameras' instantiations of the same kernel on `grid` workgroups (kernels_quaternion.hip; LaunchBalEvaluate calls it)
hipError_t LaunchBalEvaluateQuat(const BalEvalArgs& A, bool jacobian, int grid, hipStream_t stream, int camera_model);
// The same in TILE order for the <2,3,9> fused path: the Jacobian lands in the solver's tiles (J_out, b_out: BalArgs' layout), the F
// cells also at slot_fpos of e.values (nullptr: not), the residuals in e.residuals; e.values' E cells are NOT written.
struct BalEvalTilesArgs {
  BalEvalArgs e;
  int64_t n_tiles = 0;
  const int32_t* slot_bpos = nullptr;   // 2 x row of the slot, -1: padding
  const int32_t* slot_fpos = nullptr;   // where the row's F cell starts in e.values
  const int32_t* slot_cam = nullptr;    // the slot's camera / point (state order) / observed pixel: e.row_* in slot order
  const int32_t* slot_pt = nullptr;
  const double2* slot_obs = nullptr;
  double* pt_pack = nullptr;            // scratch: [state 3 | scale 3] per point, [state 9 | scale 9] per camera (filled by the launch)
  double* cam_pack = nullptr;
  int debug_flags = 0;                  // timing experiments only (ceres_hip_debug_bal_evaluate_tiles_timing): 1 no F copy, 2 no tile J, 4 no b / residuals, 16 plain (not non-temporal) F copy
  double2* J_out = nullptr;
  int64_t tile_pitch = 0;               // double2 elements from one tile to the next
  double2* b_out = nullptr;
};
hipError_t LaunchBalEvaluateTiles(const BalEvalTilesArgs& T, int64_t n_points, int64_t n_cameras, int* nparts, hipStream_t stream);
// Constant cameras (the kernel's CONST instantiations; an argument type of its own for the reason given at BalEvalConstArgs).  cam_pack
// holds n_pack_cams records — the free cameras in the solver's order, the constant ones behind them — record k from camera pack_cam[k]
// of e.state and from e.scale + pack_scale[k] (-1: constant); slot_cam indexes the records; a slot whose slot_fpos is negative has no
// F cell: zeros in the tile, its F copy goes to `scrap` (one double2 per slot, never read).  debug_flags must be 0.
struct BalEvalTilesConstArgs : BalEvalTilesArgs {
  const int32_t* pack_cam = nullptr;
  const int32_t* pack_scale = nullptr;
  int64_t n_pack_cams = 0;
  double2* scrap = nullptr;
};
hipError_t LaunchBalEvaluateTilesConst(const BalEvalTilesConstArgs& T, int64_t n_points, int* nparts, hipStream_t stream);
// delta = step .* scale, cand = x + delta; partials[0..g) = |x|^2, [g..2g) = |delta|^2 partial sums
hipError_t LaunchBalCandidate(const double* x, const double* step, const double* scale, double* delta, double* cand, int64_t n,
                              double* partials, int* nparts, hipStream_t stream);
// kCamQuaternionManifold: delta = step .* scale (tangent, 3 n_p + 9 n_c), cand = Plus(x, delta) (ambient, 3 n_p + 10 n_c); the same
// partials (|x|^2 ambient, |delta|^2 tangent)
hipError_t LaunchBalCandidateQuat(const double* x, const double* step, const double* scale, double* delta, double* cand, int64_t n_points,
                                  int64_t n_cameras, double* partials, int* nparts, hipStream_t stream);
// kCamQuaternionManifold: partial maxima of |x - Plus(x, -g)| (ambient), g = gradient / scale (tangent)
hipError_t LaunchBalGradientMaxQuat(const double* g, const double* scale, const double* x, int64_t n_points, int64_t n_cameras,
                                    double* partials, int* nparts, hipStream_t stream);
// partial maxima of |g_i / scale_i|
hipError_t LaunchBalGradientMax(const double* g, const double* scale, int64_t n, double* partials, int* nparts, hipStream_t stream);
hipError_t LaunchBalJacobiScale(const double* colnorm2, double* scale, int64_t n, hipStream_t stream);
// partials[0..g) = |a - b|^2 partial sums (the outer loop's step norm |x - candidate| after an inner pass)
hipError_t LaunchBalDiffNorm(const double* a, const double* b, int64_t n, double* partials, int* nparts, hipStream_t stream);

// ---- the loop's vector kernels on a reduced program (kernels_constant.hip; ceres_hip_bal_create_with_constant_blocks) ----
// The free blocks: n_free_points then n_free_cameras entries of `block` (the block's first double in the full state); block i's tangent
// entries start at 3 i (points) or 3 n_free_points + cw (i - n_free_points) (cameras).
struct BalFreeBlocks {
  const int64_t* block = nullptr;
  int64_t n_free_points = 0, n_free_cameras = 0;
};
// delta = step .* scale (reduced), cand = Plus(x, delta) on the free blocks only (cand's constant blocks are not touched);
// partials[0..g) = |x|^2 over the free blocks, [g..2g) = |delta|^2
hipError_t LaunchBalCandidateFree(const BalFreeBlocks& B, int camera_model, const double* x, const double* step, const double* scale,
                                  double* delta, double* cand, double* partials, int* nparts, hipStream_t stream);
// kCamQuaternionManifold on a reduced program: LaunchBalGradientMaxQuat over the free blocks
hipError_t LaunchBalGradientMaxQuatFree(const BalFreeBlocks& B, const double* g, const double* scale, const double* x, double* partials,
                                        int* nparts, hipStream_t stream);

// ---- fixed camera intrinsics (kernels_subset.hip; ceres_hip_bal_create_with_fixed_intrinsics) ----
// mask: bit k set — coordinate 6 + k of every angle-axis camera is constant (1 .. 7); the tangent width of a camera is cw = 9 - bits.
// The Jacobian evaluation with the marked columns removed after the Corrector and before the scale: F cells of 2 x cw where
// BalEvalConstArgs says (always the reduced-program form; nothing constant: the identity reduction); A.scale indexes the tangent vector.
hipError_t LaunchBalEvaluateSubset(const BalEvalConstArgs& A, int mask, int* nparts, hipStream_t stream);
// delta = step .* scale (tangent), cand = x + delta on the free coordinates of the free blocks, marked coordinates copied from x;
// B.block == nullptr: every block is free (B.n_free_points = n_points); partials as LaunchBalCandidateFree's
hipError_t LaunchBalCandidateSubset(const BalFreeBlocks& B, int mask, int64_t n_points, const double* x, const double* step, const double* scale,
                                    double* delta, double* cand, double* partials, int* nparts, hipStream_t stream);

// ---- shared camera intrinsics (kernels_shared.hip; ceres_hip_bal_create_with_shared_intrinsics) ----
// The Jacobian evaluation of a program whose column blocks are points (3), free cameras' poses (6) and intrinsics groups (3): columns
// 0 .. 5 of the corrected 2 x 9 camera Jacobian go to the pose cell at row_fpos (-1: a constant camera, no pose cell; scale from
// row_scam), columns 6 .. 8 to the group cell at row_gpos (scale from row_sgrp).  An argument type of its own, as BalEvalConstArgs is.
struct BalEvalSharedArgs : BalEvalConstArgs {
  const int32_t* row_gpos = nullptr;
  const int32_t* row_sgrp = nullptr;
};
hipError_t LaunchBalEvaluateShared(const BalEvalSharedArgs& A, int* nparts, hipStream_t stream);
// Plus on such a handle: one work item per block, n_points points (all free, tangent entries at 3 i) then n_cameras cameras.  Camera c:
// pose += step .* scale at cam_pose[c] (-1: constant — the pose is copied), intrinsics += the group's scaled step at cam_group[c], the
// same arithmetic for every member; cam_first[c] != 0: the camera writes its group's delta and adds its |x|^2 and |delta|^2 terms.
struct BalSharedCameras {
  int64_t n_points = 0, n_cameras = 0;
  const int32_t* cam_pose = nullptr;
  const int32_t* cam_group = nullptr;
  const int32_t* cam_first = nullptr;
};
// partials as LaunchBalCandidateFree's: [0..g) = |x|^2 over the program's parameter blocks, [g..2g) = |delta|^2
hipError_t LaunchBalCandidateShared(const BalSharedCameras& B, const double* x, const double* step, const double* scale, double* delta,
                                    double* cand, double* partials, int* nparts, hipStream_t stream);

// ---- bound constraints (kernels_bounds.hip; bounds.inc: ceres_hip_bal_set_bounds) ----
// Problem::SetParameterLowerBound / SetParameterUpperBound: lower / upper in the state's (ambient) layout, no bound = -inf / +inf.  Plus
// is x + delta on every handle that takes bounds (angle-axis and Euclidean quaternion cameras), so a coordinate's ambient and tangent
// offsets inside its block coincide.  Two forms of every kernel: B.block == nullptr — every block is free, ambient index = tangent
// index, n = B.n_free_points (the whole state's length then); otherwise one work item per free block of `camera_width` (9 | 10) or 3
// doubles.  Constant blocks are neither read nor written.  No floating-point atomics: per-workgroup partials, *nparts of each.
struct BalBounds {
  const double* lower = nullptr;
  const double* upper = nullptr;
  BalFreeBlocks B;         // block == nullptr: the plain form, n_free_points = the state's length
  int camera_width = 9;
};
// Program::Plus(x, 0) in place: x = clamp(x) on the free blocks; counts[b], b < *nparts: the coordinates workgroup b moved
hipError_t LaunchBoundsProject(const BalBounds& K, double* x, unsigned long long* counts, int* nparts, hipStream_t stream);
// delta = step .* scale (fold: t (step .* scale)), out = clamp(x + t delta) (fold: clamp(x + delta)) on the free blocks; partials[k g + b],
// g = *nparts: workgroup b's share of |x|^2 (k = 0), |out - x|^2 (1), max |delta| (2) and (grad ./ scale) . delta (3; grad == nullptr: 0).
// scale may be nullptr (ones).  Products and sums are rounded one by one (no contraction), as the restatement's.
hipError_t LaunchBoundsTrialPoint(const BalBounds& K, const double* x, const double* step, const double* scale, const double* grad, double t,
                                  bool fold, double* delta, double* out, double* partials, int* nparts, hipStream_t stream);
// partial maxima of |x - clamp(x - g ./ scale)| over the free blocks (I/trust_region_minimizer.cc:281-302)
hipError_t LaunchBoundsGradientMax(const BalBounds& K, const double* x, const double* g, const double* scale, double* partials, int* nparts,
                                   hipStream_t stream);

// ---- dogleg trust region of the BAL front end (kernels_dogleg.hip; dogleg.inc) ----
constexpr int kDoglegGrid = 256;   // workgroups (and partial sums per scalar) of the two kernels below
// partials[5 q + k], q < *nparts: workgroup q's share of |J a|^2, (J a).(J b), |J b|^2, (J a).f, (J b).f (k = 0 .. 4), one walk over
// the caller-layout values; f == nullptr: the last two are 0
hipError_t LaunchJacobianGram(const GenStructure& G, const double* values, const double* a, const double* b, const double* f,
                              double* partials, int* nparts, hipStream_t stream);
// a = J^T f / dsq (the strategy's gradient over its diagonal sqrt(dsq)); partials[3 q + k]: |gradient|^2, gradient.gn, |gn|^2 with
// gn = sqrt(dsq) * b
hipError_t LaunchDoglegPrep(const double* dsq, const double* jtf, const double* b, double* a, int64_t n, double* partials, int* nparts,
                            hipStream_t stream);

// ---- inner iterations of the BAL front end (kernels_inner.hip; ceres_hip_bal_inner_iterate) ----
// One launch solves a list of parameter blocks of ONE group, each with its own Levenberg-Marquardt loop (CoordinateDescentMinimizer::Solve,
// I/coordinate_descent_minimizer.cc:213-240), all other blocks held at their values in `state`.  Block b's observations are the entries
// [ptr[b], ptr[b+1]): `other` names the camera (a point's rows) or the point (a camera's camera-major entries), `obs` the pixel.
enum InnerForm { kInnerPointLane = 0, kInnerPointWave = 1, kInnerCameraWave = 2 };
struct InnerArgs {
  double* state = nullptr;            // [3 n_p | 9 n_c], in / out (the blocks of the list are updated in place)
  int64_t cam_base = 0;               // 3 n_p
  const int32_t* blocks = nullptr;    // point or camera numbers to solve
  int32_t n_blocks = 0;
  const int32_t* ptr = nullptr;       // per point / camera: its entries
  const int32_t* other = nullptr;
  const double2* obs = nullptr;
  int32_t* iterations = nullptr;      // per point / camera: the iterations its loop took (nullptr: not written)
  LossParams loss;
};
hipError_t LaunchInnerBlocks(const InnerArgs& A, int form, hipStream_t stream);

// ---- line search minimizer of the BAL front end (kernels_line_search.hip, kernels_line_search_quat.hip; line_search.inc) ----
// Cost and gradient without a Jacobian in memory (line_search_gradient.h states the two passes and the order of every sum).
constexpr int kLsChunkPitch = 10;   // doubles per chunk partial of the camera pass (the widest camera)
struct LsGradArgs {
  int64_t n_rows = 0;                  // the rows of BalEvalArgs, grouped by point
  const int32_t *row_cam = nullptr, *row_pt = nullptr;
  const double2* row_obs = nullptr;
  const int32_t* row_pdst = nullptr;   // where the row's point starts in the tangent vector, -1: a constant point
  const double* state = nullptr;
  int64_t cam_base = 0;
  double* grad = nullptr;              // tangent: free points, then free cameras
  double* cost_partials = nullptr;     // one per workgroup of the point pass (<= 2048)
  double* wave_parts = nullptr;        // 6 per chunk of 64 rows: the sums of the chunk's first and last run
  int32_t n_long = 0;                  // points whose rows cross a chunk boundary: tangent position, first and last chunk
  const int32_t *long_dst = nullptr, *long_w0 = nullptr, *long_w1 = nullptr;
  // the camera pass: chunks of at most 64 entries of one camera's list; chunk_dst >= 0: the camera's only chunk, its tangent position;
  // otherwise -(partial + 1)
  int32_t n_chunks = 0;
  const int32_t *chunk_cam = nullptr, *chunk_start = nullptr, *chunk_len = nullptr, *chunk_dst = nullptr;
  const int32_t* cm_pt = nullptr;      // point and pixel of every entry of the camera-major list
  const double2* cm_obs = nullptr;
  double* chunk_parts = nullptr;       // kLsChunkPitch per partial
  int32_t n_fin = 0;                   // cameras of more than one chunk: tangent position, first partial, number of partials
  const int32_t *fin_dst = nullptr, *fin_first = nullptr, *fin_count = nullptr;
  LossParams loss;
};
// gradient == false: the cost alone.  *nparts cost partials.
hipError_t LaunchLsGradient(const LsGradArgs& A, bool gradient, int camera_model, int* nparts, hipStream_t stream);
hipError_t LaunchLsGradientQuat(const LsGradArgs& A, bool gradient, int camera_model, int grid_points, int grid_cameras, hipStream_t stream);
// out = Plus(x, t direction) on the free blocks (out's constant blocks are not touched); partials[0 .. g) = |x|^2 over the free blocks,
// [g .. 2 g) = |out - x|^2 (ambient)
hipError_t LaunchLsTrialPoint(const BalFreeBlocks& B, int camera_model, const double* x, const double* direction, double t, double* out,
                              double* partials, int* nparts, hipStream_t stream);
// x - Plus(x, -g) over the free blocks (EvaluateGradientNorms, I/line_search_minimizer.cc:67-83): partials[0 .. g) = its squared norm,
// [g .. 2 g) = its max norm
hipError_t LaunchLsGradientNorms(const BalFreeBlocks& B, int camera_model, const double* x, const double* g, double* partials, int* nparts,
                                 hipStream_t stream);
// partials[k g + b], k < 3: workgroup b's share of a.b, a.c (c == nullptr: 0) and its max |a|
hipError_t LaunchLsDots(const double* a, const double* b, const double* c, int64_t n, double* partials, int* nparts, hipStream_t stream);
// z = alpha x + beta y - gamma w (y, w may be nullptr)
hipError_t LaunchLsCombine(double alpha, const double* x, double beta, const double* y, double gamma, const double* w, double* z, int64_t n,
                           hipStream_t stream);

// L-BFGS on the device (LowRankInverseHessian, I/low_rank_inverse_hessian.cc:87-177): the history and every scalar between the vector
// operations stay in device memory — an update and a whole two-loop recursion run without a host synchronisation.
struct LbfgsArgs {
  int64_t n = 0;
  int32_t rank = 0, use_scaling = 0;
  double *S = nullptr, *Y = nullptr;   // rank x n each: delta_x and delta_gradient of slot k at k n
  double* sy = nullptr;                // per slot: delta_x . delta_gradient
  double* alpha = nullptr;             // per slot: the first loop's coefficient
  double* scale = nullptr;             // approximate_eigenvalue_scale_
  int32_t* order = nullptr;            // the live slots, oldest first
  int32_t* count = nullptr;            // how many
  double* parts = nullptr;             // 4 kMaxVecGrid: two alternating sets of dot partials, then d . g and max |d|
  int32_t* accepted = nullptr;         // accepted[k] = 1 / 0: what update k did
};
hipError_t LaunchLbfgsReset(const LbfgsArgs& A, hipStream_t stream);
// Update(a sv, y1 - y0) (y0 may be nullptr): the secant test, the circular buffer; accepted[log_index] records the decision
hipError_t LaunchLbfgsUpdate(const LbfgsArgs& A, double a, const double* sv, const double* y1, const double* y0, int log_index, hipStream_t stream);
// d = -H g with at most max_live live slots (the caller's bound on *count); parts[2 kMaxVecGrid + b], b < *nparts: d . g partials,
// parts[3 kMaxVecGrid + b]: max |d| partials
hipError_t LaunchLbfgsDirection(const LbfgsArgs& A, const double* g, double* d, int max_live, int* nparts, hipStream_t stream);

}  // namespace chip
#endif
