/*
 * ceres_hip.h — C ABI of the MI355X-native Levenberg–Marquardt linear-solve path.
 *
 * This is the drop-in boundary.  Everything behind it is hand-written HIP for
 * gfx950; everything in front of it is host code (the Ceres-side adapter shown
 * in INTEGRATION.md, the C++ mirror in ceres-solver_amd/host/, or the ctypes
 * binding in ceres-solver_amd/__init__.py).  Plain C types only: pointers,
 * sizes, POD structs.  No torch types, no C++ types, no exceptions.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * ceres-solver tree, "I/" = internal/ceres/):
 *
 *   ceres_hip_create / _destroy      LinearSolver::Create(options)              I/linear_solver.cc:75-126
 *                                    (cases CGNR :80-88, ITERATIVE_SCHUR :111-116)
 *   ceres_hip_set_structure          the CompressedRowBlockStructure a solver   I/block_structure.h:52-182
 *                                    reads through A->block_structure(); one
 *                                    instance sees constant sparsity            I/linear_solver.h:137-142
 *   ceres_hip_solve                  LinearSolver::Solve(A, b, per_solve, x)    I/linear_solver.h:339-342
 *                                    = CgnrSolver::SolveImpl                    I/cgnr_solver.cc:146-207
 *                                    = IterativeSchurComplementSolver::SolveImpl I/iterative_schur_complement_solver.cc:64-157
 *   ceres_hip_lm_compute_step*       LevenbergMarquardtStrategy::ComputeStep + the model cost change of
 *                                    TrustRegionMinimizer::ComputeTrustRegionStep
 *                                                                               I/levenberg_marquardt_strategy.cc:69-157
 *   options.use_explicit_schur_complement   SparseSchurComplementSolver's CG path (f2)  I/schur_complement_solver.cc:337-408
 *   SCHUR_POWER_SERIES_EXPANSION     PowerSeriesExpansionPreconditioner (f3)    I/power_series_expansion_preconditioner.cc:57-89
 *   ceres_hip_bal_*                  Evaluator::Evaluate and TrustRegionMinimizer::Minimize for bundle
 *                                    adjustment in BAL form (f4)                I/evaluator.h:116-124, I/trust_region_minimizer.cc:68-845
 *   ceres_hip_op_*                   the individual operators of SURVEY.md §8(a), exported so
 *                                    that parity tests and roofline runs can address them one
 *                                    at a time (file:line given next to each declaration).
 *
 * Conventions
 *   - every function returning int returns CERES_HIP_OK (0) or a negative
 *     CERES_HIP_E_* code; on error ceres_hip_last_error() holds a message.  A
 *     non-zero return from ceres_hip_solve maps to
 *     LinearSolverTerminationType::FATAL_ERROR on the Ceres side.
 *   - "host" pointers are ordinary (or pinned) host memory owned by the caller
 *     and not retained past the call; "dev" pointers are HIP device pointers on
 *     the solver's device, also caller-owned.
 *   - all scalars on this path are IEEE fp64, all indices int32, exactly as in
 *     the reference (SURVEY.md §8 header).
 *   - a solver handle is not thread-safe (same contract as the reference,
 *     I/implicit_schur_complement.h:88-91); distinct handles are independent.
 */
#ifndef CERES_HIP_H_
#define CERES_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): ceres_hip_info grew by collectives_last_step (128 -> 136 bytes); ceres_hip_lm_options.reserved became values_unchanged */
#define CERES_HIP_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------- */
#define CERES_HIP_OK 0
#define CERES_HIP_E_INVALID (-1)     /* bad argument / call order               */
#define CERES_HIP_E_UNSUPPORTED (-2) /* structure or option not implemented     */
#define CERES_HIP_E_HIP (-3)         /* a HIP runtime call failed               */
#define CERES_HIP_E_COMM (-4)        /* an RCCL call failed, or a peer never arrived (p2p timeout) */
#define CERES_HIP_E_NODEVICE (-5)    /* no usable gfx950 device                 */

/* ---- enums: numeric values equal the reference's -------------------------
 * solver_type         ceres::LinearSolverType          include/ceres/types.h:57-91
 * preconditioner_type ceres::PreconditionerType        include/ceres/types.h:93-141
 * termination_type    LinearSolverTerminationType      I/linear_solver.h:57-74     */
#define CERES_HIP_DENSE_SCHUR 3 /* DenseSchurComplementSolver: dense S, Cholesky; num_cols_f <= CERES_HIP_MAX_EXPLICIT_SCHUR_COLS */
#define CERES_HIP_ITERATIVE_SCHUR 5
#define CERES_HIP_CGNR 6

#define CERES_HIP_IDENTITY 0
#define CERES_HIP_JACOBI 1
#define CERES_HIP_SCHUR_JACOBI 2
#define CERES_HIP_SCHUR_POWER_SERIES_EXPANSION 3 /* ITERATIVE_SCHUR only */
#define CERES_HIP_CLUSTER_JACOBI 4 /* ITERATIVE_SCHUR only: VisibilityBasedPreconditioner, I/visibility_based_preconditioner.cc (design/14_cluster_jacobi.md) */

/* visibility_clustering_type ceres::VisibilityClusteringType       include/ceres/types.h (read with CLUSTER_JACOBI only) */
#define CERES_HIP_CANONICAL_VIEWS 0
#define CERES_HIP_SINGLE_LINKAGE 1

#define CERES_HIP_SUCCESS 0
#define CERES_HIP_NO_CONVERGENCE 1
#define CERES_HIP_FAILURE 2
#define CERES_HIP_FATAL_ERROR 3

/* Which device code path set_structure selected (ceres_hip_info.kernel_path). */
#define CERES_HIP_PATH_GENERIC 0 /* any block sizes, multi-pass kernels          */
#define CERES_HIP_PATH_BAL 1     /* fused single-pass kernels: bundle-adjustment structures — one point cell (2, 3 or 4 wide), at most one
                                  * camera cell and a few shared blocks per row, rows 2, 3 or 4 high; every static specialisation of
                                  * internal/ceres/generate_template_specializations.py:55-75 (csrc/common.h: BalShapeCompiled) */

/* ---- flattened CompressedRowBlockStructure (I/block_structure.h:52-182) ---
 * cols[j] = {col_block_size[j], col_block_pos[j]}
 * rows[i].block = {row_block_size[i], row_block_pos[i]}
 * rows[i].cells = cells[row_cell_ptr[i] .. row_cell_ptr[i+1])
 * cells[k] = {cell_col_block[k] (Cell::block_id), cell_value_pos[k] (Cell::position)}
 * Cell values are row-major row_size x col_size at values + position
 * (I/block_sparse_matrix.cc:239-274).  Nothing about the value layout is
 * assumed: E|F-split (I/block_jacobian_writer.cc:68-167), row-sequential and
 * interleaved layouts are all accepted because every access goes through
 * cell_value_pos.                                                           */
typedef struct ceres_hip_block_structure {
  int32_t num_row_blocks;
  int32_t num_col_blocks;
  const int32_t* row_block_size; /* [num_row_blocks]   */
  const int32_t* row_block_pos;  /* [num_row_blocks]   */
  const int32_t* col_block_size; /* [num_col_blocks]   */
  const int32_t* col_block_pos;  /* [num_col_blocks]   */
  const int32_t* row_cell_ptr;   /* [num_row_blocks+1] */
  const int32_t* cell_col_block; /* [num_cells]        */
  const int32_t* cell_value_pos; /* [num_cells]        */
} ceres_hip_block_structure;

/* ---- LinearSolver::Options subset that this path reads --------------------
 * I/linear_solver.h:148-230; defaults as there (max_num_iterations = 1!).   */
typedef struct ceres_hip_options {
  int32_t solver_type;           /* CERES_HIP_CGNR | CERES_HIP_ITERATIVE_SCHUR             */
  int32_t preconditioner_type;   /* IDENTITY | JACOBI | SCHUR_JACOBI | SPSE | CLUSTER_JACOBI */
  int32_t min_num_iterations;    /* LinearSolver::Options::min_num_iterations              */
  int32_t max_num_iterations;    /* LinearSolver::Options::max_num_iterations              */
  int32_t residual_reset_period; /* LinearSolver::Options::residual_reset_period (10)      */
  int32_t num_eliminate_blocks;  /* elimination_groups[0]; 0 for CGNR                      */
  int32_t device;                /* HIP device ordinal                                     */
  int32_t force_generic_path;    /* 1: never select the fused BAL kernels (testing)        */
  int32_t cg_check_interval;     /* CG iterations enqueued between host polls of the
                                    device-side termination flag; <=0 -> adaptive 2,4,8,16 */
  int32_t jacobian_storage;      /* <2,3,9> path: 0 = fp64 tiles (parity mode); 1 = Jacobian rounded
                                    to fp32 in the tiles, fp64 arithmetic (NOT parity: accuracy mode,
                                    SURVEY.md §7 item 6; halves the HBM traffic of the hot kernels)  */
  /* SCHUR_POWER_SERIES_EXPANSION (LinearSolver::Options, I/linear_solver.h:168-185) */
  int32_t max_num_spse_iterations; /* 0 -> 5 (the reference's default)                       */
  int32_t use_spse_initialization; /* start CG from the power-series estimate of S^-1 rhs    */
  double spse_tolerance;           /* for the initialisation; the preconditioner uses 0     */
  /* ITERATIVE_SCHUR with LinearSolver::Options::use_explicit_schur_complement:
   * LinearSolver::Create then returns SparseSchurComplementSolver (I/linear_solver.cc:104-109), which
   * forms S with SchurEliminator::Eliminate and runs SCHUR_JACOBI-preconditioned CG on it
   * (SolveReducedLinearSystemUsingConjugateGradients, I/schur_complement_solver.cc:337-408).
   * Here: on one rank S is stored block-sparse like the reference's BlockRandomAccessSparseMatrix (any size that fits in
   * HBM); a sharded run stores it DENSE (num_cols_f <= CERES_HIP_MAX_EXPLICIT_SCHUR_COLS) and all-reduces it.
   * preconditioner_type must be SCHUR_JACOBI (the reference CHECKs the same).                */
  int32_t use_explicit_schur_complement;
  /* CLUSTER_JACOBI: how the F blocks ("cameras") are clustered by the E blocks they see — CERES_HIP_CANONICAL_VIEWS (0, Ceres' default)
   * or CERES_HIP_SINGLE_LINKAGE; any other value fails ceres_hip_create with CERES_HIP_E_INVALID.  Ignored by the other
   * preconditioners.  (The field was `reserved`, which every caller passed as 0.)
   * Where the reference leaves the result to the iteration order of its hash sets, this library pins it: candidates are scanned and a
   * candidate's neighbours summed in ascending F-block index, only a strictly greater score replaces the best (the lowest index wins a
   * tie), and the clusters are numbered by ascending first member.  Every such result is one the reference can produce. */
  int32_t visibility_clustering_type;
} ceres_hip_options;
#define CERES_HIP_MAX_EXPLICIT_SCHUR_COLS 8192

/* ---- LinearSolver::Summary (I/linear_solver.h:320-326) ------------------- */
typedef struct ceres_hip_summary {
  double residual_norm;     /* -1, as the reference's iterative solvers leave it */
  int32_t num_iterations;
  int32_t termination_type; /* CERES_HIP_SUCCESS ... CERES_HIP_FATAL_ERROR      */
  char message[256];
} ceres_hip_summary;

/* What set_structure derived; all counts in scalars unless noted. */
typedef struct ceres_hip_info {
  int32_t kernel_path;      /* CERES_HIP_PATH_*                                        */
  int32_t num_rows, num_cols;
  int32_t num_cols_e, num_cols_f;
  int32_t num_row_blocks_e; /* rows whose first cell is an E block (PMV ctor :60-66)   */
  int32_t num_e_blocks, num_f_blocks;
  int32_t row_block_size, e_block_size, f_block_size; /* DetectStructure; -1 = dynamic */
  int64_t num_nonzeros;
  int64_t num_observations; /* BAL path: rows with one E and one F cell; else 0        */
  int64_t num_tiles;        /* BAL path: 64-slot tiles after packing                   */
  int64_t device_bytes;     /* HBM held by this handle                                 */
  int32_t camera_accum_in_lds; /* BAL path: 1 if the F-space accumulators fit in LDS   */
  int32_t world_size, rank;
  int32_t p2p_enabled;      /* the one-shot peer-to-peer all-reduce is connected AND passed its self-test */
  int32_t p2p_fine_grained; /* its receive buffer is a fine-grained allocation (0: the runtime could only export a
                               coarse-grained one — fine between ranks that share a device, self-tested otherwise)  */
  /* BAL path with more cameras than LDS rows (camera_accum_in_lds == 0): hybrid accumulation (csrc/plan.cc) — the popular cameras
   * in every workgroup's LDS, every other camera in the windows of a few workgroups, points grouped accordingly                  */
  int32_t camera_accum_hybrid;        /* 1: hybrid plan; 0: every observation's F^T z is spilled (or camera_accum_in_lds)          */
  int32_t hybrid_popular_rows;        /* accumulator rows every workgroup gives to the popular cameras                             */
  int64_t num_observations_in_lds;    /* observations summed in LDS by the tile pass (the others are spilled to the ring)          */
  int32_t points_renumbered;          /* 1: the tiles hold the points in an internal order (fuller tiles, hybrid groups)           */
  int32_t cg_iteration_in_operator; /* 1: camera space of at most 512 scalars — the S.x pass finishes the CG iteration itself (one launch) */
  int32_t collectives_last_step;    /* sharded instances: all-reduces this rank issued since its last ceres_hip_lm_compute_step began      */
} ceres_hip_info;

typedef struct ceres_hip_solver ceres_hip_solver; /* opaque */

/* ---- lifetime ------------------------------------------------------------ */
int ceres_hip_abi_version(void);
/* Number of visible HIP devices whose arch is gfx950 (0 => nothing will run). */
int ceres_hip_device_count(void);
/* Create a solver; returns NULL on failure (see ceres_hip_last_error(NULL)). */
ceres_hip_solver* ceres_hip_create(const ceres_hip_options* options);
void ceres_hip_destroy(ceres_hip_solver* s);
/* Message for the most recent error on s (or, with s == NULL, of create). */
const char* ceres_hip_last_error(const ceres_hip_solver* s);

/* Upload the (constant) sparsity once per solver instance.  For a sharded run
 * each rank passes the structure of ITS rows only: E (point) column blocks are
 * disjoint across ranks, F (camera) column blocks are the same on every rank
 * (SURVEY.md §8e).  On a sharded instance (a communicator is connected) the call
 * is COLLECTIVE: the ranks agree on the kernel path and the fused shape — a shard
 * can look like bundle adjustment to one rank alone — and on where the exchanges
 * run; every rank must make it, in the same order among its collective calls.  */
int ceres_hip_set_structure(ceres_hip_solver* s, const ceres_hip_block_structure* bs);
int ceres_hip_get_info(const ceres_hip_solver* s, ceres_hip_info* info);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ----------------------
 * Rank 0 obtains an id, the host distributes the 128 bytes by any means
 * (torch.distributed broadcast in bench.py), every rank calls comm_init.
 * After that ceres_hip_solve / the op_* entry points sum F-space (camera)
 * quantities over ranks with ncclAllReduce on the solver's stream, and the
 * CGNR inner products over the E-space (point) part likewise.               */
#define CERES_HIP_UNIQUE_ID_BYTES 128
int ceres_hip_comm_get_unique_id(uint8_t id[CERES_HIP_UNIQUE_ID_BYTES]);
int ceres_hip_comm_init(ceres_hip_solver* s, const uint8_t id[CERES_HIP_UNIQUE_ID_BYTES],
                        int32_t rank, int32_t world_size);

/* Alternative (or additional) communicator: a one-shot peer-to-peer all-reduce over buffers mapped with hipIpc
 * — xGMI between the GPUs of a node, plain device memory between two ranks that share one GPU.  The sums a
 * sharded solve exchanges are 9 or 81 doubles per camera: latency-bound, several per step, so the collective is a
 * single kernel (push to every peer, flag, wait, sum in rank order = identical bits on every rank) instead of an
 * RCCL call.  Step 1: every rank calls _prepare (before set_structure) with the largest vector it will sum
 * (99 * num_f_blocks covers a step: blocks, rhs and column norms are summed in ONE all-reduce) and receives a 64-byte hipIpc handle; the host gathers the handles of all
 * ranks in rank order by any means; step 2: every rank calls _connect.  With both communicators present, messages
 * longer than max_elements go to RCCL; with only this one they are cut into pieces.  world_size <= 8.       */
#define CERES_HIP_IPC_HANDLE_BYTES 64
int ceres_hip_comm_p2p_prepare(ceres_hip_solver* s, int32_t rank, int32_t world_size, int64_t max_elements,
                               uint8_t handle_out[CERES_HIP_IPC_HANDLE_BYTES]);
/* _connect is collective and ENDS WITH THE SELF-TEST below: it returns non-zero, with the path disabled on this rank, unless known
 * values made it through every peer's buffer.  Callers never get an untested peer-to-peer path.                         */
int ceres_hip_comm_p2p_connect(ceres_hip_solver* s, const uint8_t* all_handles /* world_size x 64 bytes */);
/* Collective self-test (six all-reduces of multi-chunk vectors with values that change every round — a receive slot is
 * re-used every second epoch, so stale cached lines show from the third round on; 5 s timeout): non-zero leaves the
 * path disabled on this rank; ranks then agree on the verdict out of band and call _disable everywhere if any failed
 * (RCCL takes over).                                                                                               */
int ceres_hip_comm_p2p_selftest(ceres_hip_solver* s);
int ceres_hip_comm_p2p_disable(ceres_hip_solver* s);
/* Debug / measurement (collective): average microseconds of `iters` back-to-back all-reduces of n doubles. */
int ceres_hip_debug_allreduce_timing(ceres_hip_solver* s, int64_t n, int32_t iters, double* avg_us);
/* Debug: how the last ITERATIVE_SCHUR solve of the handle got the point part of its solution — 0: the back-substitution pass over the
 * Jacobian, 1: the point tail (short CG solves on the fused one-GPU path, formed from the S.x passes' per-point sums; CERES_HIP_POINT_TAIL=0
 * in the environment of ceres_hip_set_structure switches it off).  Negative: no handle.                              */
int ceres_hip_debug_last_backsub_route(const ceres_hip_solver* s);

/* ---- the boundary call ----------------------------------------------------
 * LinearSolver::Solve (I/linear_solver.h:339-342).  values: num_nonzeros
 * doubles in the caller's layout; b: num_rows; D: num_cols or NULL
 * (PerSolveOptions::D, :237-257); x: num_cols, fully overwritten unless the
 * termination type is FAILURE/FATAL_ERROR
 * (I/iterative_schur_complement_solver.cc:150-154).                          */
int ceres_hip_solve(ceres_hip_solver* s, const double* host_values, const double* host_b,
                    const double* host_D, double q_tolerance, double r_tolerance,
                    double* host_x, ceres_hip_summary* summary);
/* LinearSolver::Solve again on the values and b of the previous ceres_hip_solve / ceres_hip_load on this handle, with a new D (the
 * retry after a rejected trust-region step: I/levenberg_marquardt_strategy.cc:164-176 shrinks the radius, the minimizer calls
 * ComputeStep on the same Jacobian, I/trust_region_minimizer.cc:381-461).  Nothing but D goes up, the tiles are not rebuilt.      */
int ceres_hip_solve_unchanged_values(ceres_hip_solver* s, const double* host_D, double q_tolerance, double r_tolerance,
                                     double* host_x, ceres_hip_summary* summary);
/* Same, all four arrays already resident in HBM (used by bench.py so that the
 * timed region holds no PCIe traffic; also the form a device evaluator uses).
 * STREAM ORDER of every *_device entry point: the work runs on the handle's own stream, created hipStreamNonBlocking — it does NOT
 * wait for the legacy default stream or for any stream of the caller.  Whatever produced dev_values / dev_b / dev_D, and whatever
 * last wrote the output array (a fill, say), must have COMPLETED before the call (hipStreamSynchronize or an event the host waited
 * for); when the call returns, its device work has completed and the output may be read from any stream.  (Found by
 * tools/fuzz_sequence.py --threads: a NaN fill of the output queued on a busy default stream landed after the step.)           */
int ceres_hip_solve_device(ceres_hip_solver* s, const double* dev_values, const double* dev_b,
                           const double* dev_D, double q_tolerance, double r_tolerance,
                           double* dev_x, ceres_hip_summary* summary);

/* ---- operator-level entry points (parity tests, roofline runs) ------------
 * All of them act on the state loaded by ceres_hip_load.  Vector arguments are
 * HOST pointers; results are copied back synchronously.                      */

/* Upload values/b/D (b, D may be NULL) and run the per-step re-layout kernel. */
int ceres_hip_load(ceres_hip_solver* s, const double* host_values, const double* host_b,
                   const double* host_D);
int ceres_hip_load_device(ceres_hip_solver* s, const double* dev_values, const double* dev_b,
                          const double* dev_D);

/* y += A x      BlockSparseMatrix::RightMultiplyAndAccumulate  I/block_sparse_matrix.cc:239-274 */
int ceres_hip_op_right_multiply(ceres_hip_solver* s, const double* x, double* y);
/* y += A^T x    BlockSparseMatrix::LeftMultiplyAndAccumulate   I/block_sparse_matrix.cc:278-349 */
int ceres_hip_op_left_multiply(ceres_hip_solver* s, const double* x, double* y);
/* PartitionedMatrixView<kRow,kE,kF> products: E = the first cell of each of the first
 * num_row_blocks_e rows, F = all other cells.  x / y live in the part's own column space
 * (E: num_cols_e doubles, F: num_cols_f doubles indexed at col_block_pos - num_cols_e), rows in the
 * full row space; all four accumulate into y.
 *   y += E x    RightMultiplyAndAccumulateE        I/partitioned_matrix_view_impl.h:112-139
 *   y += F x    RightMultiplyAndAccumulateF        :141-190
 *   y += E^T x  LeftMultiplyAndAccumulateE(Single|Multi)Threaded  :192-250
 *   y += F^T x  LeftMultiplyAndAccumulateF(Single|Multi)Threaded  :252-375                       */
int ceres_hip_op_right_multiply_e(ceres_hip_solver* s, const double* x, double* y);
int ceres_hip_op_right_multiply_f(ceres_hip_solver* s, const double* x, double* y);
int ceres_hip_op_left_multiply_e(ceres_hip_solver* s, const double* x, double* y);
int ceres_hip_op_left_multiply_f(ceres_hip_solver* s, const double* x, double* y);
/* blockdiag(E^T E) / blockdiag(F^T F), dense row-major blocks in column-block order (no D).
 * UpdateBlockDiagonalEtE / UpdateBlockDiagonalFtF                  :446-658                       */
int ceres_hip_op_block_diagonal_ete(ceres_hip_solver* s, double* blocks, int64_t capacity);
int ceres_hip_op_block_diagonal_ftf(ceres_hip_solver* s, double* blocks, int64_t capacity);
/* x[j] = |A_j|^2  BlockSparseMatrix::SquaredColumnNorm           I/block_sparse_matrix.cc:351-401 */
int ceres_hip_op_squared_column_norm(ceres_hip_solver* s, double* x);
/* y = (A^T A + D^2) x, one fused pass.  CgnrLinearOperator::RightMultiplyAndAccumulate
 * with y zeroed first, as CG calls it                           I/cgnr_solver.cc:98-114        */
int ceres_hip_op_jtjx(ceres_hip_solver* s, const double* x, double* y);
/* y = A^T b     CgnrSolver::SolveImpl rhs                        I/cgnr_solver.cc:188-191       */
int ceres_hip_op_jtb(ceres_hip_solver* s, double* y);
/* out[5] = |J a|^2, (J a).(J b), |J b|^2, (J a).f, (J b).f on the loaded J and right-hand side f (f not loaded: the last two are 0);
 * a, b: host vectors of num_cols.  One pass over the caller-layout values: what the dogleg strategy of ceres_hip_bal_minimize reads
 * per Jacobian (DoglegStrategy's Cauchy point, subspace model and model cost change, I/dogleg_strategy.cc:185-199, 648-719). */
int ceres_hip_op_jacobian_gram(ceres_hip_solver* s, const double* a, const double* b, double* out);

/* ImplicitSchurComplement::Init: block_diagonal (E^T E + D_e^2)^-1 and
 * rhs = F^T (b - E (E^T E)^-1 E^T b)                             I/implicit_schur_complement.cc:49-97,179-204,251-276 */
int ceres_hip_op_schur_init(ceres_hip_solver* s);
/* rhs of the reduced system: num_cols_f doubles. */
int ceres_hip_get_schur_rhs(ceres_hip_solver* s, double* rhs);
/* Inverse E^T E blocks, dense row-major e x e each, in E-block order. */
int ceres_hip_get_ete_inverse(ceres_hip_solver* s, double* blocks, int64_t capacity);
/* y = S x       ImplicitSchurComplement::RightMultiplyAndAccumulate (assigns y)
 *                                                                I/implicit_schur_complement.cc:106-144 */
int ceres_hip_op_schur_sx(ceres_hip_solver* s, const double* x, double* y);
/* ImplicitSchurComplement::BackSubstitute: z (num_cols_f) -> x (num_cols)
 *                                                                I/implicit_schur_complement.cc:208-243 */
int ceres_hip_op_back_substitute(ceres_hip_solver* s, const double* z, double* x);

/* y += (F^T F + D_f^2)^-1 F^T E (E^T E + D_e^2)^-1 E^T F x
 * ImplicitSchurComplement::InversePowerSeriesOperatorRightMultiplyAccumulate    I/implicit_schur_complement.cc:146-174
 * (call after ceres_hip_op_schur_init; computes the F^T F inverse blocks on first use) */
int ceres_hip_op_power_series_operator(ceres_hip_solver* s, const double* x, double* y);
/* y = sum_{k=0..n} Z^k (F^T F)^-1 x, stopping early when |term| < tolerance * |first term|
 * PowerSeriesExpansionPreconditioner::RightMultiplyAndAccumulate  I/power_series_expansion_preconditioner.cc:57-84 */
int ceres_hip_op_spse_apply(ceres_hip_solver* s, const double* x, double* y, int32_t max_num_spse_iterations,
                            double spse_tolerance);

/* BlockSparseJacobiPreconditioner::UpdateImpl                    I/block_jacobi_preconditioner.cc:59-115 */
int ceres_hip_op_block_jacobi_update(ceres_hip_solver* s);
/* SchurJacobiPreconditioner::UpdateImpl = SchurEliminator::Eliminate into a
 * block-diagonal lhs + Invert     I/schur_jacobi_preconditioner.cc:87-97, I/schur_eliminator_impl.h:184-311 */
int ceres_hip_op_schur_jacobi_update(ceres_hip_solver* s);
/* VisibilityBasedPreconditioner::UpdateImpl for CLUSTER_JACOBI (I/visibility_based_preconditioner.cc:322-380): SchurEliminator::Eliminate
 * into the block pairs (i <= j) of F blocks that share a chunk (or an E-free row) AND a cluster, D_f^2 on the diagonal, then one dense
 * Cholesky factorisation per cluster.  ceres_hip_op_precond_apply then applies y += M^-1 x by two triangular solves per cluster.
 * CERES_HIP_E_INVALID on a handle that was not created with CERES_HIP_CLUSTER_JACOBI; a pivot that is not positive is reported as
 * CERES_HIP_E_INVALID "Preconditioner update failed." (inside a solve: termination FAILURE with that message). */
int ceres_hip_op_cluster_jacobi_update(ceres_hip_solver* s);
/* What set_structure derived for CLUSTER_JACOBI: the number of clusters, the largest cluster's scalar dimension, the bytes of the dense
 * factors, and the seconds the host analysis took (clustering + pair lists).  Any pointer may be NULL.  CERES_HIP_E_INVALID on a NULL
 * handle, before set_structure, or on a handle without CLUSTER_JACOBI. */
int ceres_hip_cluster_jacobi_stats(const ceres_hip_solver* s, int32_t* num_clusters, int32_t* largest_cluster_dimension,
                                   int64_t* factor_bytes, double* setup_seconds);
/* The preconditioner's inverted diagonal blocks, dense row-major, block order.
 * If not_inverted != 0 the blocks as they were BEFORE Invert() are returned
 * (i.e. the diagonal blocks of J^T J + D^2, or of S).                        */
int ceres_hip_get_preconditioner_blocks(ceres_hip_solver* s, int32_t not_inverted,
                                        double* blocks, int64_t capacity);
/* y += M^-1 x   BlockRandomAccessDiagonalMatrix::RightMultiplyAndAccumulate
 *                                                                I/block_random_access_diagonal_matrix.cc:102-116 */
int ceres_hip_op_precond_apply(ceres_hip_solver* s, const double* x, double* y);

/* SchurEliminator::Eliminate with a DENSE lhs (all S(i,j) cells present) and
 * rhs; lhs is num_cols_f x num_cols_f row-major, upper block triangle filled
 * like the reference (I/schur_eliminator_impl.h:184-311,548-565).  Generic
 * kernels; meant for the small/explicit-S callers.         */
int ceres_hip_op_schur_eliminate_dense(ceres_hip_solver* s, double* lhs, double* rhs);
/* The explicit Schur complement of a solver created with use_explicit_schur_complement = 1 (one rank): the lhs
 * SparseSchurComplementSolver::InitStorage allocates (I/schur_complement_solver.cc:224-290) in the storage of
 * BlockRandomAccessSparseMatrix (I/block_random_access_sparse_matrix.cc:51-110) — block pairs (i <= j, F-relative ids,
 * sorted; every (i, i) present), each a row-major n_i x n_j cell at pair_offset.
 *   _storage_info            counts
 *   _op_schur_eliminate_sparse  SchurEliminator::Eliminate into that lhs (incl. D_f^2); returns pairs, offsets, values
 *   _op_schur_symmetric_multiply  y += S x from the stored upper block triangle
 *                            BlockRandomAccessSparseMatrix::SymmetricRightMultiplyAndAccumulate  :125-163            */
int ceres_hip_schur_storage_info(const ceres_hip_solver* s, int64_t* num_block_pairs, int64_t* num_values);
int ceres_hip_op_schur_eliminate_sparse(ceres_hip_solver* s, int32_t* pair_i, int32_t* pair_j, int64_t* pair_offset,
                                        double* values, int64_t pair_capacity, int64_t value_capacity);
int ceres_hip_op_schur_symmetric_multiply(ceres_hip_solver* s, const double* x, double* y);
/* SchurEliminator::BackSubstitute                                I/schur_eliminator_impl.h:314-380 */
int ceres_hip_op_eliminator_back_substitute(ceres_hip_solver* s, const double* z, double* x);

/* BLAS-1 used by CG: Dot / Norm / Axpby   I/eigen_vector_ops.h:47-101.  n <= num_cols. */
int ceres_hip_op_dot(ceres_hip_solver* s, const double* x, const double* y, int64_t n,
                     double* result);
int ceres_hip_op_axpby(ceres_hip_solver* s, double a, const double* x, double b, const double* y,
                       int64_t n, double* z);

/* ---- the neighbours of Solve inside one trust-region step, on the device ----
 * LevenbergMarquardtStrategy::ComputeStep (I/levenberg_marquardt_strategy.cc:69-157):
 *   diag = clamp(SquaredColumnNorm(J), min, max) unless reuse_diagonal; D = sqrt(diag / radius);
 *   Solve(J, residuals, {D, eta, -1}, step); finite check; step = -step
 * and the model-cost bookkeeping of TrustRegionMinimizer::ComputeTrustRegionStep
 * (I/trust_region_minimizer.cc:420-438): model_cost_change = -(J step)'(f + J step / 2).
 * J is read in place; nothing but the step and a few scalars returns to the host.            */
typedef struct ceres_hip_lm_options {
  double radius;          /* trust-region radius                                   */
  double min_diagonal;    /* Solver::Options::min_lm_diagonal (1e-6; >= 0, I/solver.cc:414) */
  double max_diagonal;    /* Solver::Options::max_lm_diagonal (1e32)               */
  double eta;             /* q_tolerance of the linear solve                       */
  int32_t reuse_diagonal; /* 1 after a rejected step: keep the previous diag(J'J)  */
  /* 1: `values` and `residuals` are what the PREVIOUS ceres_hip_lm_compute_step* / ceres_hip_load* on this handle received — the
   * Jacobian is re-evaluated only in HandleSuccessfulStep (I/trust_region_minimizer.cc:832-837), so the ComputeStep that follows a
   * rejected or invalid step (I/levenberg_marquardt_strategy.cc:134,164,170: the calls that also set reuse_diagonal_) solves on the
   * SAME matrix with a smaller radius.  The solver then keeps what it holds: no host-to-device copy (the host pointers may be NULL),
   * no re-layout into tiles; the step's first pass reads the resident tiles.  A caller that re-evaluated says 0 (separate from
   * reuse_diagonal: the two are independent statements).  Device entry point: the same device pointers, contents untouched.        */
  int32_t values_unchanged;
} ceres_hip_lm_options;
typedef struct ceres_hip_lm_result {
  ceres_hip_summary linear_solver; /* FAILURE also when the step is not finite      */
  double model_cost_change;
  int32_t step_is_finite;
  int32_t reserved;
} ceres_hip_lm_result;
int ceres_hip_lm_compute_step(ceres_hip_solver* s, const double* host_values, const double* host_residuals,
                              const ceres_hip_lm_options* options, double* host_step, ceres_hip_lm_result* result);
int ceres_hip_lm_compute_step_device(ceres_hip_solver* s, const double* dev_values, const double* dev_residuals,
                                     const ceres_hip_lm_options* options, double* dev_step,
                                     ceres_hip_lm_result* result);
/* ---- the upload hidden behind the evaluator ---------------------------------------------------------------
 * Through ceres_hip_lm_compute_step a step on a Venice-sized problem costs 21 ms, 18.4 of them the host-to-device copy of the
 * Jacobian the CPU Evaluator has just written (1.04 GB at 56 GB/s).  The evaluator writes it row block by row block, over hundreds of
 * milliseconds and from several threads (ProgramEvaluator::Evaluate's parallel loop, I/program_evaluator.h:168-300, into the pinned
 * values_ of BlockSparseMatrix(use_page_locked_memory), I/block_jacobian_writer.cc:261-262): finished rows can go up while later
 * rows are still being evaluated.
 *   _begin(values, residuals)      before the evaluator starts: the host arrays it will fill (pinned for the copies to be asynchronous;
 *                                  they must stay valid and — once announced — unwritten until _end returns)
 *   _ready(first_row_block, n)     THREAD-SAFE; row blocks [first, first + n) are complete in both arrays: their value ranges and
 *                                  residuals are enqueued on a copy stream.  Every row block at most once; any order; any granularity.
 *                                  (Layouts whose rows are not one or two monotone value streams — Ceres' own are: all E cells then
 *                                  all F cells in row order, or row-sequential — are remembered and sent by _end.)
 *   _end(column_scale)             rows nobody announced go up now; the solver's stream waits for the copies; column_scale != NULL:
 *                                  BlockSparseMatrix::ScaleColumns on the copy in HBM (I/block_sparse_matrix.cc:403-450) — the evaluator
 *                                  hands over the UNSCALED Jacobian, Jacobi scaling (I/trust_region_minimizer.cc:263-279) happens here.
 *                                  The HOST waits for the copies before _end returns: from then on the caller may write, scale or free
 *                                  both arrays.
 * ORDER: _end comes BEFORE the caller's own jacobian->ScaleColumns().  _end sends the rows nobody announced (every row, where the layout
 * has no value streams) from the host array and then scales the copy in HBM: rows that were already scaled on the host would be scaled
 * twice.  The caller scales its host copy after _end has returned.
 * Between _begin and _end the device copy is half written: every entry point that reads or replaces the loaded values (ceres_hip_load*,
 * ceres_hip_solve*, ceres_hip_lm_compute_step*, ceres_hip_op_*, a second _begin) returns CERES_HIP_E_INVALID and leaves the session open.
 * The values then count as loaded by ceres_hip_load: ceres_hip_lm_compute_step(s, NULL, NULL, {.., values_unchanged = 1}, ..) computes the
 * step without another copy (the first pass re-lays the tiles out as after any load).                                              */
int ceres_hip_values_begin(ceres_hip_solver* s, const double* host_values, const double* host_residuals);
int ceres_hip_values_ready(ceres_hip_solver* s, int32_t first_row_block, int32_t num_row_blocks);
int ceres_hip_values_end(ceres_hip_solver* s, const double* host_column_scale);
/* bytes that went up before / inside _end of the last streamed upload; value streams of the layout (0: not streamable, 1, 2) */
int ceres_hip_get_stream_stats(const ceres_hip_solver* s, int64_t* bytes_early, int64_t* bytes_late, int32_t* value_streams);

/* The D the last ceres_hip_lm_compute_step* used (num_cols doubles). */
int ceres_hip_get_lm_diagonal(ceres_hip_solver* s, double* host_D);
/* values[.., col] *= scale[col] on the loaded (device) copy; returns the scaled values if
 * host_values_out != NULL.  BlockSparseMatrix::ScaleColumns       I/block_sparse_matrix.cc:403-450 */
int ceres_hip_op_scale_columns(ceres_hip_solver* s, const double* host_scale, double* host_values_out);

/* ---- the Evaluator side of the boundary for bundle adjustment in BAL form ----
 * For the one cost function of bundle_adjuster (examples/snavely_reprojection_error.h:53-105,
 * camera = angle-axis(3) translation(3) focal k1 k2, 2 residuals per observation) this replaces
 * ceres::internal::Evaluator (I/evaluator.h:98-158: Evaluate(state, cost, residuals, gradient,
 * jacobian), Plus) — ProgramEvaluator + autodiff Jets + BlockJacobianWriter in the reference —
 * and TrustRegionMinimizer::Minimize with the Levenberg-Marquardt strategy
 * (I/trust_region_minimizer.cc:68-845, I/levenberg_marquardt_strategy.cc:69-157) around the
 * linear solvers above, with the Jacobian, the residuals and every vector of the loop resident
 * in HBM: per iteration only a few scalars cross PCIe.
 *
 * The reduced program is Schur-ordered (I/reorder_program.cc:278-360): state = [3 doubles per
 * point, points 0..n_p-1 | 9 doubles per camera], residual rows grouped by point, stable in
 * observation order; the Jacobian has the BlockSparseMatrix layout BlockJacobianWriter produces
 * for it (all E cells, 6 doubles per row, then all F cells, 18 per row), which
 * is fully determined by ceres_hip_bal_get_row_order.                                                   */
typedef struct ceres_hip_bal ceres_hip_bal;
/* `options` configures the linear solver (solver_type CGNR or ITERATIVE_SCHUR, preconditioner,
 * iteration limits); num_eliminate_blocks is set to num_points.  BAL reader: examples/bal_problem.cc:75-135. */
ceres_hip_bal* ceres_hip_bal_create(const ceres_hip_options* options, int32_t num_cameras, int32_t num_points,
                                    int64_t num_observations, const int32_t* camera_index,
                                    const int32_t* point_index, const double* observations);
/* Camera models (bundle_adjuster --use_quaternions, --use_manifolds: examples/bundle_adjuster.cc:111-113, 323-347).  The quaternion
 * cameras are [q_w q_x q_y q_z | t(3) | f k1 k2] (Ceres' quaternion order; SnavelyReprojectionErrorWithQuaternions, rotation by
 * QuaternionRotatePoint: q need not have unit norm).                                 state / Jacobian columns per camera */
#define CERES_HIP_CAMERA_ANGLE_AXIS 0           /* [angle-axis(3) t(3) f k1 k2] (ceres_hip_bal_create)        9 / 9  */
#define CERES_HIP_CAMERA_QUATERNION 1           /* Euclidean Plus on all ten (--use_quaternions)              10 / 10 */
#define CERES_HIP_CAMERA_QUATERNION_MANIFOLD 2  /* ProductManifold<QuaternionManifold, EuclideanManifold<6>>
                                                   (--use_quaternions --use_manifolds)                         10 / 9  */
/* ceres_hip_bal_create with a camera model (ceres_hip_bal_create is camera_model CERES_HIP_CAMERA_ANGLE_AXIS).  The state stays
 * [3 per point | cameras] and is AMBIENT (Evaluator::NumParameters, ceres_hip_bal_sizes); the Jacobian, the gradient and
 * minimize's step and scaling are in the TANGENT space (Evaluator::NumEffectiveParameters, ceres_hip_bal_num_effective_parameters):
 * the local Jacobian ambient J x PlusJacobian, then the Corrector, as ResidualBlock::Evaluate forms it.  F cells are 2 x 10 or 2 x 9
 * (E cells at 6 r, F cells at 6 n_rows + 2 width r).  NULL (message in ceres_hip_bal_last_error(NULL)) for an unknown camera_model —
 * checked before any device call — and for what ceres_hip_bal_create refuses.  With a quaternion camera: inner iterations
 * (ceres_hip_bal_set_inner_iterations with anything but CERES_HIP_INNER_NONE, ceres_hip_bal_inner_iterate) and the tile timing probe
 * return CERES_HIP_E_UNSUPPORTED, so does ceres_hip_bal_minimize on a sharded handle; the loop evaluates in the caller layout (the
 * tile-order evaluator is angle-axis only). */
ceres_hip_bal* ceres_hip_bal_create_with_camera(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                const int32_t* point_index, const double* observations);
/* ceres_hip_bal_create_with_camera for a Problem in which SetParameterBlockConstant was called on some cameras and points: the handle
 * is the REDUCED program Program::RemoveFixedBlocks leaves (I/program.cc:309-410), Schur-ordered.
 * camera_is_constant[num_cameras], point_is_constant[num_points]: non-zero = constant; either may be NULL (none constant).  The masks
 * are creation-time: one handle sees one sparsity (I/linear_solver.h:137-142), and the block structure depends on them.
 *   - The caller's STATE keeps its full layout and length [3 per point | cs per camera] (ceres_hip_bal_sizes' first value).  Constant
 *     blocks are read, never written: after ceres_hip_bal_minimize / ceres_hip_bal_inner_iterate their doubles are bit-identical.
 *   - The TANGENT side is the reduced program's: ceres_hip_bal_num_effective_parameters = 3 free points + cw free cameras; gradient,
 *     step, Jacobi scale and the Jacobian's columns are [free points in ascending index | free cameras in ascending index];
 *     num_eliminate_blocks = free points.
 *   - ROWS: an observation whose camera and point are both constant is removed (its cost is the fixed cost).  The others are grouped
 *     by point, stable in observation order, the rows of constant points (no E cell) AFTER all rows that have one, stable in
 *     observation order (the last bucket of LexicographicallyOrderResidualBlocks, I/reorder_program.cc:278-340).
 *     ceres_hip_bal_get_row_order writes num_rows entries; ceres_hip_bal_sizes reports 2 num_rows residuals and the reduced number of
 *     Jacobian values.
 *   - JACOBIAN VALUES as BlockJacobianWriter lays out the reduced program: all E cells first (6 per row with a free point, in row
 *     order), then the F cells (2 cw per row with a free camera, in row order).  A row has one cell or two.
 *   - COST: ceres_hip_bal_evaluate is the Evaluator of the reduced program (kept rows only).  ceres_hip_bal_minimize reports what
 *     TrustRegionMinimizer reports: initial_cost, final_cost and every iterations[i].cost INCLUDE the fixed cost
 *     (I/trust_region_minimizer.cc:127, 228, 261, 490); the function-tolerance test and the relative decrease use the reduced
 *     program's cost alone.  The fixed cost is evaluated once per minimize call, on the device, with the loss in force.
 *   - Inner iterations: constant blocks are in no group (block_iterations = -1: a block outside the ordering); a free block's own loop
 *     still sees ALL its observations, the ones against constant blocks included.
 *   - With both masks NULL or all zero the handle is the one ceres_hip_bal_create_with_camera builds.
 * NULL (message in ceres_hip_bal_last_error(NULL)), before any device call: no free camera or no free point (Ceres switches the linear
 * solver there — LinearSolverForZeroEBlocks, I/linear_solver.cc:51, I/trust_region_preprocessor.cc:89 — which this front end does not), and what
 * ceres_hip_bal_create_with_camera refuses.  ceres_hip_bal_minimize on a sharded handle with constant blocks: CERES_HIP_E_UNSUPPORTED.
 * Constant cameras alone keep the tile-order evaluator of the fused path; constant points leave rows without an E cell (the remainder
 * kernels) and the loop evaluates in the caller layout. */
ceres_hip_bal* ceres_hip_bal_create_with_constant_blocks(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                         int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                         const int32_t* point_index, const double* observations,
                                                         const uint8_t* camera_is_constant, const uint8_t* point_is_constant);
/* Fixed camera intrinsics: SubsetManifold(9, constant coordinates) on EVERY camera block (include/ceres/manifold.h;
 * I/residual_block.cc:161-195), together with constant blocks.  camera_coordinate_is_constant: cs entries (9), one mask for all
 * cameras of the handle; NULL or all zero: exactly the handle ceres_hip_bal_create_with_constant_blocks builds.  Angle-axis cameras
 * [angle-axis(3) t(3) f k1 k2] only, and only coordinates 6, 7, 8 (f, k1, k2) may be marked, any non-empty subset of them.
 *   - STATE: ambient and unchanged, 9 doubles per camera (ceres_hip_bal_sizes' first value, 3 n_p + 9 n_c).  A marked coordinate is
 *     read and never written: after ceres_hip_bal_minimize its doubles are bit-identical to the caller's.
 *   - TANGENT: cw = 9 - (number marked) = 6, 7 or 8 entries per free camera, its free coordinates in ascending index;
 *     ceres_hip_bal_num_effective_parameters = 3 free points + cw free cameras.  Plus adds the tangent step to the free coordinates.
 *   - JACOBIAN: the ambient one with the marked columns removed (PlusJacobian is a selection) — after the Corrector, before the Jacobi
 *     scale.  F cells are 2 x cw; the values are [E cells, 6 per row | F cells, 2 cw per row], 6 + 2 cw per kept row with both cells.
 *   - The gradient's max norm is |g_i|_inf over the tangent, the step norm the tangent |delta|; |x| of the parameter-tolerance test
 *     runs over the ambient doubles of the free blocks, marked coordinates included (the block stays in the program with all nine).
 *   - camera_is_constant / point_is_constant as above: a constant camera is removed, the coordinate mask applies to the free ones.
 *   - With an iterative solver, no force_generic_path and no constant point the handle runs the fused <2,3,cw> path.
 * NULL (message in ceres_hip_bal_last_error(NULL)), before any device call: a quaternion camera model with an entry set, an entry set
 * outside 6 .. 8, all nine set ("use constant cameras"), and what ceres_hip_bal_create_with_constant_blocks refuses.
 * On a handle with fixed intrinsics ceres_hip_bal_evaluate, ceres_hip_bal_minimize (LEVENBERG_MARQUARDT and both DOGLEG types, every
 * linear solver the front end accepts), ceres_hip_bal_set_loss, ceres_hip_bal_fixed_cost, ceres_hip_bal_reduced_sizes and
 * ceres_hip_bal_get_row_order work as usual.  CERES_HIP_E_UNSUPPORTED, with a message that says so: ceres_hip_bal_set_inner_iterations
 * with anything but NONE, ceres_hip_bal_inner_iterate, ceres_hip_bal_evaluate_gradient, ceres_hip_bal_minimize_line_search,
 * ceres_hip_bal_covariance, ceres_hip_debug_bal_evaluate_tiles_timing, and ceres_hip_bal_minimize on a sharded handle.  The loop
 * evaluates in the caller layout (the tile-order evaluator writes <2,3,9> tiles). */
ceres_hip_bal* ceres_hip_bal_create_with_fixed_intrinsics(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                          int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                          const int32_t* point_index, const double* observations,
                                                          const uint8_t* camera_is_constant, const uint8_t* point_is_constant,
                                                          const uint8_t* camera_coordinate_is_constant /* cs entries */);
/* Shared camera intrinsics: one 3-wide parameter block [f k1 k2] per GROUP of cameras beside a 6-wide pose block [angle-axis(3) t(3)]
 * per camera (examples/libmv_bundle_adjuster.cc:697-728: every residual block of a camera's images on the camera's intrinsics block).
 * camera_group: num_cameras entries in [0, num_groups); NULL: exactly the handle ceres_hip_bal_create_with_constant_blocks builds
 * (num_groups is not read).  Angle-axis cameras only; every camera belongs to exactly one group, every id in [0, num_groups) is used.
 *   - STATE: ambient and unchanged, 3 n_p + 9 n_c doubles.  The intrinsics of a group are the doubles 6 .. 8 of its cameras and must
 *     be BIT-IDENTICAL within a group: ceres_hip_bal_evaluate, ceres_hip_bal_minimize and ceres_hip_bal_fixed_cost check it on the
 *     host before any device call (CERES_HIP_E_INVALID; the message names the first offending camera and coordinate).  After
 *     ceres_hip_bal_minimize every camera of a group holds the same bits again.
 *   - TANGENT: [points | poses of the free cameras | groups], 3 n_p + 6 (free cameras) + 3 num_groups entries
 *     (ceres_hip_bal_num_effective_parameters).
 *   - COLUMN BLOCKS of the program: points (3), the free cameras' poses (6), groups (3), in that order.  A row has an E cell, a pose
 *     cell (2 x 6) unless its camera is constant, and a group cell (2 x 3).
 *   - VALUES: [E cells, 6 per row | per row, back to back in column order: pose cell 12, group cell 6] — 24 per row of a free camera.
 *   - JACOBIAN: the ambient 2 x 9 one after the Corrector; columns 0 .. 5 go to the pose cell, columns 6 .. 8 to the group cell, then
 *     the Jacobi scale.  A group's columns of J hold the rows of all its cameras; J^T r, column norms and the LM diagonal are the
 *     linear solver's operators over this structure.
 *   - PLUS: pose += step; every camera of group g gets x[6 .. 8] + delta_g — the same arithmetic on the same bits for every member.
 *   - The gradient's max norm is |g_i|_inf over the tangent, the step norm the tangent |delta|; |x| of the parameter-tolerance test
 *     counts each group's three doubles ONCE and a constant camera's pose not at all (the program's parameter blocks).
 *   - camera_is_constant (NULL-able) holds a camera's POSE constant; its rows keep the E and the group cell, its group stays free.
 *     No row is removed, the fixed cost is 0.  Constant points are not offered by this creator.
 *   - Which kernels run is ceres_hip_set_structure's decision (ceres_hip_get_info), made from the structure alone: one or two groups
 *     take the fused <2,3,6> path with the 4- or 8-scalar shared strip, constant cameras being its rows without a camera cell — with
 *     CGNR too, since this front end hands over the elimination order; three or more groups exceed the strip and run the generic
 *     kernels, and so does a grouping in which a group has a single camera.  The loop evaluates in the caller layout.
 * NULL (message in ceres_hip_bal_last_error(NULL)), before any device call: a quaternion camera model, num_groups <= 0 or
 * > num_cameras, a group id out of range, an unused group id, and what ceres_hip_bal_create_with_constant_blocks refuses.
 * On such a handle ceres_hip_bal_evaluate, ceres_hip_bal_minimize (LEVENBERG_MARQUARDT on ITERATIVE_SCHUR, CGNR and DENSE_SCHUR, both
 * DOGLEG types on DENSE_SCHUR), ceres_hip_bal_set_loss, ceres_hip_bal_sizes, ceres_hip_bal_reduced_sizes,
 * ceres_hip_bal_get_row_order and ceres_hip_bal_fixed_cost work as usual, and so does ceres_hip_bal_covariance on a DENSE_SCHUR
 * handle (poses, points and groups: see there).  CERES_HIP_E_UNSUPPORTED, with a message that says "shared intrinsics":
 * ceres_hip_bal_set_inner_iterations with anything but NONE, ceres_hip_bal_inner_iterate, ceres_hip_bal_evaluate_gradient,
 * ceres_hip_bal_minimize_line_search, ceres_hip_bal_set_bounds with a finite bound, ceres_hip_debug_bal_evaluate_tiles_timing, and
 * ceres_hip_bal_minimize on a sharded handle. */
ceres_hip_bal* ceres_hip_bal_create_with_shared_intrinsics(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                           int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                           const int32_t* point_index, const double* observations,
                                                           const uint8_t* camera_is_constant /* NULL-able */,
                                                           const int32_t* camera_group /* num_cameras entries in [0, num_groups) */,
                                                           int32_t num_groups);
/* What the reduction made of the problem (all NULL-able): rows kept, rows with an E cell (they come first), rows dropped because both
 * blocks are constant, free cameras, free points. */
int ceres_hip_bal_reduced_sizes(const ceres_hip_bal* p, int64_t* num_rows, int64_t* num_rows_e, int64_t* num_rows_removed,
                                int32_t* num_free_cameras, int32_t* num_free_points);
/* Solver::Summary::fixed_cost: 1/2 sum rho(|r|^2) over the removed rows at `state` (full layout), with the handle's current loss
 * (0 when no row was removed). */
int ceres_hip_bal_fixed_cost(ceres_hip_bal* p, const double* state, double* fixed_cost);
void ceres_hip_bal_destroy(ceres_hip_bal* p);
const char* ceres_hip_bal_last_error(const ceres_hip_bal* p);
/* The linear solver this problem drives (borrowed; operators, timing, info). */
ceres_hip_solver* ceres_hip_bal_linear_solver(ceres_hip_bal* p);
/* Evaluator::NumParameters (the ambient state) / NumResiduals, and the number of Jacobian values (6 + 2 x camera Jacobian columns per
 * observation: 24, or 26 for CERES_HIP_CAMERA_QUATERNION; 18, 20 or 22 with fixed intrinsics). */
int ceres_hip_bal_sizes(const ceres_hip_bal* p, int64_t* num_parameters, int64_t* num_residuals, int64_t* num_jacobian_values);
/* Evaluator::NumEffectiveParameters: the tangent length — of the gradient, and the Jacobian's columns (= num_parameters for the
 * angle-axis and the Euclidean quaternion camera). */
int ceres_hip_bal_num_effective_parameters(const ceres_hip_bal* p, int64_t* num_effective_parameters);
/* row_observation[r] = index of the observation residual row block r belongs to. */
int ceres_hip_bal_get_row_order(const ceres_hip_bal* p, int32_t* row_observation);
/* Robust losses (include/ceres/loss_function.h:131-330, internal/ceres/loss_function.cc:46-175).  Ceres has no enumeration of
 * them: these numbers are this ABI's own.  a, b: the loss's constructor arguments (Tolerant takes both, the others a only). */
#define CERES_HIP_LOSS_TRIVIAL 0   /* TrivialLoss: rho(s) = s                                  */
#define CERES_HIP_LOSS_HUBER 1     /* HuberLoss(a)                                             */
#define CERES_HIP_LOSS_SOFTLONE 2  /* SoftLOneLoss(a)                                          */
#define CERES_HIP_LOSS_CAUCHY 3    /* CauchyLoss(a)                                            */
#define CERES_HIP_LOSS_ARCTAN 4    /* ArctanLoss(a)                                            */
#define CERES_HIP_LOSS_TOLERANT 5  /* TolerantLoss(a, b)                                       */
#define CERES_HIP_LOSS_TUKEY 6     /* TukeyLoss(a)                                             */
/* The loss of every observation of the problem — Problem::AddResidualBlock(cost, loss, camera, point) with one loss for all, as
 * bundle_adjuster --robustify does (HuberLoss(1.0): examples/bundle_adjuster.cc:114,331) — wrapped in ScaledLoss(loss, scale).
 * It stays in force for the later ceres_hip_bal_evaluate / ceres_hip_bal_minimize calls until set again; a problem that never sets
 * one has the plain squared loss (as has CERES_HIP_LOSS_TRIVIAL with scale 1).  It is applied where Ceres applies it, in the
 * Evaluator (internal/ceres/residual_block.cc:161-195, the Corrector of internal/ceres/corrector.cc:41-135), before the linear
 * solver sees the Jacobian.  CERES_HIP_E_INVALID (message in ceres_hip_bal_last_error; of ceres_hip_bal_last_error(NULL) for a NULL
 * handle) for an unknown loss_type or a non-finite or out-of-range parameter: a <= 0 for the one-parameter losses, a < 0 or b <= 0
 * for TOLERANT, scale <= 0.  b is ignored by the other losses, a by TRIVIAL. */
int ceres_hip_bal_set_loss(ceres_hip_bal* p, int32_t loss_type, double a, double b, double scale);
/* Inner iterations (Solver::Options::use_inner_iterations, inner_iteration_ordering, inner_iteration_tolerance: include/ceres/solver.h:686-715;
 * bundle_adjuster --inner_iterations --blocks_for_inner_iterations: examples/bundle_adjuster.cc:83-88, 190-243).  After every valid
 * trust-region step ceres_hip_bal_minimize runs one coordinate-descent pass from the candidate (TrustRegionMinimizer::
 * DoInnerIterationsIfNeeded, internal/ceres/trust_region_minimizer.cc:509-587): group by group, every block of a group is refined by its
 * own small Levenberg-Marquardt solve with Ceres' DEFAULT minimizer options and every other block fixed
 * (CoordinateDescentMinimizer, internal/ceres/coordinate_descent_minimizer.cc:130-240), the loss included.  `blocks` picks the
 * ordering: */
#define CERES_HIP_INNER_NONE 0            /* no inner iterations (the default)                                       */
#define CERES_HIP_INNER_AUTOMATIC 1       /* CoordinateDescentMinimizer::CreateOrdering: recursive independent sets,
                                             reversed; degree ties broken by state position (points, then cameras)   */
#define CERES_HIP_INNER_CAMERAS 2         /* every camera in group 0 (points are not refined)                        */
#define CERES_HIP_INNER_POINTS 3          /* every point in group 0 (cameras are not refined)                         */
#define CERES_HIP_INNER_CAMERAS_POINTS 4  /* cameras in group 0, points in group 1                                    */
#define CERES_HIP_INNER_POINTS_CAMERAS 5  /* points in group 0, cameras in group 1                                    */
/* In force for the later ceres_hip_bal_minimize / ceres_hip_bal_inner_iterate calls until set again.  tolerance =
 * inner_iteration_tolerance (Ceres' default 1e-3): once a pass improves the candidate's cost by a relative amount <= tolerance, the
 * rest of that minimize call runs without them.  CERES_HIP_E_INVALID (message as for ceres_hip_bal_set_loss) for a NULL handle, an
 * unknown `blocks`, or a negative or non-finite tolerance. */
int ceres_hip_bal_set_inner_iterations(ceres_hip_bal* p, int32_t blocks, double tolerance);
/* One pass (CoordinateDescentMinimizer::Minimize) at `state` (host, in / out) with the handle's ordering and loss; cost_before /
 * cost_after: the cost at the state given and returned.  block_iterations (may be NULL): per block in state order (points, then cameras)
 * the iterations its Levenberg-Marquardt loop took, -1 for a block outside the ordering.  Bit-for-bit reproducible.
 * CERES_HIP_E_INVALID with CERES_HIP_INNER_NONE set; CERES_HIP_E_UNSUPPORTED on a sharded handle. */
int ceres_hip_bal_inner_iterate(ceres_hip_bal* p, double* state, double* cost_before, double* cost_after, int32_t* block_iterations);
/* Of the last ceres_hip_bal_minimize: Solver::Summary::num_inner_iteration_steps and inner_iteration_time_in_seconds
 * (include/ceres/solver.h:864, 914), and the number of groups of the ordering it ran (0 without inner iterations). */
int ceres_hip_bal_inner_iteration_stats(const ceres_hip_bal* p, int32_t* num_inner_iteration_steps, double* inner_iteration_seconds,
                                        int32_t* num_groups);
/* Trust-region strategy of ceres_hip_bal_minimize (Solver::Options::trust_region_strategy_type, dogleg_type: include/ceres/solver.h;
 * bundle_adjuster --trust_region_strategy --dogleg).  In force for the later ceres_hip_bal_minimize calls until set again; a handle that
 * never set it runs LEVENBERG_MARQUARDT.  DOGLEG follows DoglegStrategy (I/dogleg_strategy.cc): the Gauss-Newton step of
 * (J^T J + mu diag(J^T J)) with mu from 1e-8, the Cauchy point, and their traditional interpolation or the minimum of the model on the
 * 2-D subspace they span; a rejected step reuses both (no linear solve), an invalid one multiplies mu by 10 and keeps the radius.
 * dogleg_type is read only with CERES_HIP_DOGLEG.  CERES_HIP_E_INVALID for a NULL handle, an unknown value, or DOGLEG on an
 * ITERATIVE_SCHUR or CGNR handle (Ceres' own message, I/solver.cc:431-438); CERES_HIP_E_UNSUPPORTED for DOGLEG on a sharded handle. */
#define CERES_HIP_LEVENBERG_MARQUARDT 0
#define CERES_HIP_DOGLEG 1
#define CERES_HIP_TRADITIONAL_DOGLEG 0
#define CERES_HIP_SUBSPACE_DOGLEG 1
int ceres_hip_bal_set_trust_region_strategy(ceres_hip_bal* p, int32_t strategy, int32_t dogleg_type);
/* Evaluator::Evaluate.  Host pointers; cost is required, the others may be NULL.  jacobian_values
 * is UNSCALED; gradient = J^T residuals.  Leaves the evaluated point loaded in the linear solver
 * (as ceres_hip_load_device would), so the ceres_hip_op_* entry points can be applied to it.
 * With a loss set (ceres_hip_bal_set_loss): cost = 1/2 sum rho(|r|^2), and residuals, jacobian_values (still unscaled) and
 * gradient are the Corrector's: r~, J~ and J~^T r~ (= sum rho' J^T r). */
int ceres_hip_bal_evaluate(ceres_hip_bal* p, const double* state, double* cost, double* residuals, double* gradient,
                           double* jacobian_values);
/* Solver::Options of the trust-region loop (include/ceres/solver.h defaults in comments). */
typedef struct ceres_hip_minimizer_options {
  int32_t max_num_iterations;            /* 50 */
  int32_t jacobi_scaling;                /* 1 */
  int32_t max_consecutive_invalid_steps; /* max_num_consecutive_invalid_steps, 5 */
  int32_t reserved;
  double initial_trust_region_radius;    /* 1e4 */
  double max_trust_region_radius;        /* 1e16 */
  double min_trust_region_radius;        /* 1e-32 */
  double min_lm_diagonal;                /* 1e-6 */
  double max_lm_diagonal;                /* 1e32 */
  double min_relative_decrease;          /* 1e-3 */
  double eta;                            /* 1e-1 */
  double function_tolerance;             /* 1e-6 */
  double gradient_tolerance;             /* 1e-10 */
  double parameter_tolerance;            /* 1e-8 */
} ceres_hip_minimizer_options;
void ceres_hip_minimizer_default_options(ceres_hip_minimizer_options* o);
/* IterationSummary (include/ceres/iteration_callback.h), the fields the loop itself produces. */
typedef struct ceres_hip_iteration_summary {
  double cost, cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius;
  int32_t step_is_successful, step_is_valid, linear_solver_iterations, linear_solver_termination;
} ceres_hip_iteration_summary;
#define CERES_HIP_MAX_LOGGED_ITERATIONS 256
#define CERES_HIP_CONVERGENCE 0    /* TerminationType CONVERGENCE    */
#define CERES_HIP_NO_CONVERGENCE_T 1 /* NO_CONVERGENCE */
#define CERES_HIP_MINIMIZER_FAILURE 2 /* FAILURE */
typedef struct ceres_hip_minimizer_summary {
  double initial_cost, final_cost;
  int32_t num_successful_steps, num_unsuccessful_steps, num_linear_solves, termination_type;
  double linear_solver_seconds, evaluation_seconds, total_seconds;
  int32_t num_iterations_logged, reserved;
  ceres_hip_iteration_summary iterations[CERES_HIP_MAX_LOGGED_ITERATIONS];
  char message[256];
} ceres_hip_minimizer_summary;
/* TrustRegionMinimizer::Minimize with LEVENBERG_MARQUARDT, or DOGLEG as ceres_hip_bal_set_trust_region_strategy chose; monotonic
 * steps.  state: host, in/out. */
int ceres_hip_bal_minimize(ceres_hip_bal* p, const ceres_hip_minimizer_options* options, double* state,
                           ceres_hip_minimizer_summary* summary);
/* ---- the line search minimizer (Solver::Options::minimizer_type = LINE_SEARCH; bundle_adjuster --line_search) ----
 * LineSearchMinimizer (internal/ceres/line_search_minimizer.cc) with its search directions (line_search_direction.cc,
 * low_rank_inverse_hessian.cc) and line searches (line_search.cc, polynomial.cc), on the handle's problem: camera model, loss and
 * constant blocks as ceres_hip_bal_minimize honours them.  No Jacobian is ever formed: cost and gradient come from a gradient-only
 * evaluator, the L-BFGS history and recursion stay on the device.  The enum values are the reference's (include/ceres/types.h). */
#define CERES_HIP_STEEPEST_DESCENT 0
#define CERES_HIP_NONLINEAR_CONJUGATE_GRADIENT 1
#define CERES_HIP_LBFGS 2
#define CERES_HIP_BFGS 3 /* a dense n x n matrix: refused with CERES_HIP_E_UNSUPPORTED (use CERES_HIP_LBFGS) */
#define CERES_HIP_FLETCHER_REEVES 0
#define CERES_HIP_POLAK_RIBIERE 1
#define CERES_HIP_HESTENES_STIEFEL 2
#define CERES_HIP_ARMIJO 0
#define CERES_HIP_WOLFE 1
#define CERES_HIP_BISECTION 0
#define CERES_HIP_QUADRATIC 1
#define CERES_HIP_CUBIC 2
/* Solver::Options of the line search minimizer (include/ceres/solver.h defaults in comments). */
typedef struct ceres_hip_line_search_options {
  int32_t max_num_iterations;                       /* 50 */
  int32_t line_search_direction_type;               /* CERES_HIP_LBFGS */
  int32_t nonlinear_conjugate_gradient_type;        /* CERES_HIP_FLETCHER_REEVES */
  int32_t max_lbfgs_rank;                           /* 20 */
  int32_t use_approximate_eigenvalue_bfgs_scaling;  /* 0 */
  int32_t line_search_type;                         /* CERES_HIP_WOLFE */
  int32_t line_search_interpolation_type;           /* CERES_HIP_CUBIC */
  int32_t max_num_line_search_step_size_iterations; /* 20 */
  int32_t max_num_line_search_direction_restarts;   /* 5 */
  int32_t reserved;
  double min_line_search_step_size;                 /* 1e-9 */
  double line_search_sufficient_function_decrease;  /* 1e-4 */
  double max_line_search_step_contraction;          /* 1e-3 */
  double min_line_search_step_contraction;          /* 0.6 */
  double line_search_sufficient_curvature_decrease; /* 0.9 */
  double max_line_search_step_expansion;            /* 10 */
  double function_tolerance;                        /* 1e-6 */
  double gradient_tolerance;                        /* 1e-10 */
  double parameter_tolerance;                       /* 1e-8 */
} ceres_hip_line_search_options;
void ceres_hip_line_search_default_options(ceres_hip_line_search_options* o);
typedef struct ceres_hip_line_search_iteration {
  double cost, cost_change, gradient_max_norm, gradient_norm, step_norm, step_size;
  int32_t line_search_function_evaluations, line_search_gradient_evaluations, line_search_iterations, reserved;
} ceres_hip_line_search_iteration;
typedef struct ceres_hip_line_search_summary {
  double initial_cost, final_cost;
  int32_t num_iterations;       /* every iteration, logged or not (iteration 0 — the initial evaluation — not counted) */
  int32_t num_successful_steps;
  int32_t num_line_search_steps;
  int32_t num_line_search_direction_restarts;
  int32_t num_function_evaluations, num_gradient_evaluations;   /* the initial evaluation included */
  int32_t termination_type;     /* CERES_HIP_CONVERGENCE / CERES_HIP_NO_CONVERGENCE_T / CERES_HIP_MINIMIZER_FAILURE */
  int32_t num_iterations_logged;
  double evaluation_seconds, direction_seconds, total_seconds;
  int64_t lbfgs_history_bytes;  /* the history the handle holds: 2 rank n_t doubles, rank the largest asked for so far (0: none) */
  ceres_hip_line_search_iteration iterations[CERES_HIP_MAX_LOGGED_ITERATIONS];   /* [0]: the initial evaluation */
  char message[256];
} ceres_hip_line_search_summary;
/* Evaluator::Evaluate(state, cost, nullptr, gradient, nullptr): cost = 1/2 sum rho with the handle's loss; gradient (may be NULL: the
 * cost alone) in the tangent space — ceres_hip_bal_num_effective_parameters doubles, free points then free cameras, unscaled; per
 * observation rho' J^T r.  No Jacobian value and no per-observation contribution is written to memory; no floating-point atomics: two
 * calls at one state give the same bits.  Works on every handle (any linear solver, any camera model, constant blocks) EXCEPT one with
 * fixed intrinsics (ceres_hip_bal_create_with_fixed_intrinsics): CERES_HIP_E_UNSUPPORTED there and on a sharded handle.  The solver's
 * loaded values are not touched. */
int ceres_hip_bal_evaluate_gradient(ceres_hip_bal* p, const double* state, double* cost, double* gradient);
/* LineSearchMinimizer::Minimize.  state: host, in / out (constant blocks come back bit-identical; the reported costs include the fixed
 * cost).  No Jacobi scaling (the reference applies none here); the handle's inner-iteration and trust-region settings are ignored.
 * The options are validated first (LineSearchOptionsAreValid, internal/ceres/solver.cc, Ceres' wording): CERES_HIP_E_INVALID — also
 * for BISECTION with max_line_search_step_contraction > 0.5 or min_line_search_step_contraction < 0.5, which the reference only warns
 * about; CERES_HIP_E_UNSUPPORTED for CERES_HIP_BFGS, on a sharded handle and on a handle with fixed intrinsics.  The message is in ceres_hip_bal_last_error(p) — (NULL)
 * for a NULL handle. */
int ceres_hip_bal_minimize_line_search(ceres_hip_bal* p, const ceres_hip_line_search_options* options, double* state,
                                       ceres_hip_line_search_summary* summary);
/* ---- bound constraints (Problem::SetParameterLowerBound / SetParameterUpperBound; design/23_bounds.md) ----
 * internal/ceres/parameter_block.h:227-255 (Plus clamps every coordinate of x_plus_delta to [lower, upper]), program.cc:215-289
 * (IsBoundsConstrained, IsFeasible), trust_region_minimizer.cc:103-108, 210-220, 281-302, 596-641, 726-748 (the projected line search,
 * the initial projection, the projected gradient norm, DoLineSearch, the ambient step norm), line_search.cc:103-145, 281-366
 * (LineSearchFunction, ArmijoLineSearch), line_search_preprocessor.cc:47-51 (the line search minimizer refuses bounds).
 * Bounds are per coordinate of the AMBIENT state, in the state's layout [3 per point | cs per camera].  A value <= -DBL_MAX (or -inf)
 * is no lower bound, a value >= DBL_MAX (or +inf) no upper bound.  A handle is CONSTRAINED when some coordinate of a FREE block has a
 * finite bound; bounds on constant blocks are kept but never applied.  A handle that is not constrained behaves in every call exactly
 * as if bounds had never been set, bit for bit.  On a constrained handle ceres_hip_bal_minimize
 *   - projects the state onto the box before the first evaluation (Plus(x, 0));
 *   - reports gradient_max_norm = max |x - clamp(x - g)| over the free blocks;
 *   - after every valid step runs a projected ARMIJO search on phi(a) = cost(clamp(x + a delta)), first sample a = 1, phi'(0) =
 *     g . delta (unprojected, as Ceres passes it), direction max norm |delta|_inf; CUBIC interpolation evaluates the gradient at every
 *     sample (phi'(a) = g(x_a) . delta), QUADRATIC and BISECTION the cost alone; success: delta *= a, failure (the iteration limit, or a
 *     step below min_line_search_step_size): delta unchanged; model_cost_change stays the full step's;
 *   - takes candidate = clamp(x + delta), its cost from the loop's own cost-only evaluation, and step_norm = |x - candidate| in the
 *     ambient space (not the tangent |delta| of the unbounded loop).  The rest of the iteration is unchanged (it stays monotonic).
 * Of the line-search options only line_search_interpolation_type, min_line_search_step_size, line_search_sufficient_function_decrease,
 * max_line_search_step_contraction, min_line_search_step_contraction and max_num_line_search_step_size_iterations are read, and only
 * they are validated (LineSearchOptionsAreValid's rules and wording); NULL: the defaults.
 * ceres_hip_bal_evaluate, ceres_hip_bal_evaluate_gradient and ceres_hip_bal_covariance ignore bounds (the Evaluator and Covariance do).
 * On a constrained handle ceres_hip_bal_minimize with inner iterations set and ceres_hip_bal_inner_iterate return
 * CERES_HIP_E_UNSUPPORTED; ceres_hip_bal_minimize_line_search returns CERES_HIP_E_INVALID, "LINE_SEARCH Minimizer does not support
 * bounds."; ceres_hip_bal_minimize returns CERES_HIP_E_INVALID before any device call when a constant block's value lies outside its
 * bounds (Program::IsFeasible; the message names the block, the index and the three numbers; the state is untouched). */
/* Problem::SetParameterLowerBound / SetParameterUpperBound for every coordinate at once. lower / upper: n_a doubles each
 * (ceres_hip_bal_sizes' first value), copied; either NULL: no bound on that side; both NULL: clears. In force until set again.
 * CERES_HIP_E_INVALID: a NULL handle, a NaN bound, lower >= upper on a coordinate of a free block (Ceres' "infeasible bound": the
 * message gives the block, the index and both values), a line-search field out of range.  CERES_HIP_E_UNSUPPORTED with a non-NULL
 * array: a CERES_HIP_CAMERA_QUATERNION_MANIFOLD handle, a handle with fixed intrinsics, a sharded handle.  A refused call changes
 * nothing.  The device buffers of the feature are allocated by the first call that constrains the handle and freed with the handle. */
int ceres_hip_bal_set_bounds(ceres_hip_bal* p, const double* lower, const double* upper,
                             const ceres_hip_line_search_options* line_search_options);
/* Program::Plus(state, 0): state (host, in/out) clamped on the free blocks; *num_moved = coordinates changed. Not constrained: untouched, 0. */
int ceres_hip_bal_project(ceres_hip_bal* p, double* state, int64_t* num_moved);
/* Of the last ceres_hip_bal_minimize: Summary::is_constrained, num_line_search_steps (sum of the searches' iterations), the searches'
 * function / gradient evaluations and seconds, the coordinates the initial projection moved; and per LOGGED iteration i (index of
 * summary.iterations[i]; arrays of CERES_HIP_MAX_LOGGED_ITERATIONS, NULL-able): the search's iterations (-1: none ran — iteration 0,
 * an invalid step, an unconstrained handle), whether it succeeded, and the step size applied (1 where it failed or did not run). */
int ceres_hip_bal_bounds_stats(const ceres_hip_bal* p, int32_t* is_constrained, int32_t* num_line_search_steps,
                               int32_t* num_function_evaluations, int32_t* num_gradient_evaluations, double* line_search_seconds,
                               int64_t* num_projected, int32_t* line_search_iterations, int32_t* line_search_success, double* step_size);
/* Debug: the bounded loop's vector kernels at a host state, as the loop launches them. v: n_t (tangent).
 * trial_out (n_a) = clamp(Plus(state, t v)) on the free blocks, the rest copied; *x_norm = |state| and *step_norm = |trial_out - state|
 * over the free blocks; *projected_max_norm = max |state - clamp(Plus(state, -v))|.  CERES_HIP_E_INVALID on a handle that is not
 * constrained (the kernels need the bounds on the device). */
int ceres_hip_debug_bal_bounded_step(ceres_hip_bal* p, const double* state, const double* v, double t, double* trial_out,
                                     double* x_norm, double* step_norm, double* projected_max_norm);
/* ---- covariance (ceres::Covariance: include/ceres/covariance.h, internal/ceres/covariance_impl.cc; design/17_covariance.md) ----
 * Cov = (J^T J)^-1 with J the Evaluator's Jacobian of the reduced program at `state`: unscaled, no LM diagonal, loss-corrected when
 * apply_loss_function is set (CovarianceImpl evaluates it so, covariance_impl.cc:71); columns [free points | free cameras].  Computed in
 * the Schur form — C_p = E_p^T E_p, Y_p = C_p^-1 E_p^T F, S = F^T F - sum_p (E_p^T F)^T C_p^-1 (E_p^T F):
 *     camera - camera: the block of S^-1;   point p - camera c: -Y_p S^-1[:, c];   point p - point q: delta_pq C_p^-1 + Y_p S^-1 Y_q^T
 * with S dense, factored by the blocked Cholesky of DENSE_SCHUR and inverted from the factor on the matrix pipe.
 * Blocks are in the TANGENT space (3 for a point, 9 for an angle-axis or quaternion-manifold camera, 10 for a Euclidean quaternion
 * camera); a pair that involves a constant block is all zeros (covariance_impl.cc:143-165).  Not offered: lifting to the ambient space of
 * a manifold camera, null_space_rank and the pseudo-inverse, sharded handles, handles whose linear solver is not CERES_HIP_DENSE_SCHUR,
 * handles with fixed intrinsics (ceres_hip_bal_create_with_fixed_intrinsics: CERES_HIP_E_UNSUPPORTED).
 * SHARED INTRINSICS (ceres_hip_bal_create_with_shared_intrinsics, DENSE_SCHUR; design/28_shared_covariance.md).  The same matrix of the
 * handle's own Jacobian: unscaled, no LM diagonal, loss-corrected unless apply_loss_function = 0, columns [points | poses of the free
 * cameras | groups].  The camera side of the Schur form then has two cells per row: with a_k the pose columns of observation k (none
 * when the pose is constant) and g_k its group's, Y_k = C_p^-1 E_k^T [F_k^pose | F_k^grp] and cols_k = {a_k .. a_k + 5, g_k .. g_k + 2},
 *     pose / group - pose / group: the sub-block of S^-1;   point p - pose / group t: -sum_k Y_k S^-1[cols_k, t];
 *     point p - point q: delta_pq C_p^-1 + sum_{k,l} Y_k S^-1[cols_k, cols_l] Y_l^T.
 * Blocks: point q is q (3), the POSE of camera c is num_points + c (6), group g is num_points + num_cameras + g (3).  A pair with a
 * constant pose is zeros; a group is never constant, even when all its cameras' poses are.  The state's groups must be bit-identical
 * (CERES_HIP_E_INVALID before any device call, as ceres_hip_bal_evaluate answers).  Everything below holds unchanged.
 * RANK.  An unpivoted Cholesky does not notice a lost gauge, so S and every C_p are factored with a unit diagonal (S~ = Lambda S Lambda,
 * Lambda = diag(S)^-1/2; S^-1 = Lambda S~^-1 Lambda) and the call FAILS when a pivot is not above min_scaled_pivot, or when a diagonal
 * entry is not positive (a point all of whose rows a loss switched off).  This guard is a property of the inputs — on bundle-adjustment
 * problems a free gauge leaves pivots below 1e-10 and a fixed one pivots above 1e-3 (design/17_covariance.md) — NOT a rank-revealing
 * factorization.  Ceres' SPARSE_QR path fails on the same problems, with "Jacobian matrix is rank deficient". */
typedef struct ceres_hip_covariance_options {
  int32_t apply_loss_function;   /* 1 (Covariance::Options::apply_loss_function); 0: the uncorrected Jacobian even when a loss is set */
  int32_t reserved;
  double  min_scaled_pivot;      /* 1e-8, see RANK above */
} ceres_hip_covariance_options;
void ceres_hip_covariance_default_options(ceres_hip_covariance_options* o);
typedef struct ceres_hip_covariance_summary {
  int32_t termination_type;      /* CERES_HIP_SUCCESS / CERES_HIP_FAILURE */
  int32_t reserved;
  double  min_point_pivot, min_schur_pivot;   /* smallest pivot of the unit-diagonal-scaled factorizations (0: not positive; the Schur
                                                 one is -1 when the point stage already failed) */
  double  evaluate_seconds, eliminate_seconds, factor_seconds, inverse_seconds, blocks_seconds;
  int64_t device_bytes;          /* what this feature holds on the handle (the second n x n buffer, the point blocks, the lists) */
  char    message[256];
} ceres_hip_covariance_summary;
/* Blocks are numbered in state order: point q is q, camera c is num_points + c (on a handle with shared intrinsics group g is
 * num_points + num_cameras + g; on every other handle such an index is out of range).  blocks_out: the concatenation, in pair order, of
 * dim(a) x dim(b) row-major blocks; the pair (b, a) gives the exact transpose of (a, b); a pair may repeat.  options NULL: the defaults.
 * The handle's loss, camera model and constant masks are honoured as ceres_hip_bal_evaluate honours them; the solver's loaded values are
 * overwritten as by that call; the loss, the inner-iteration and strategy settings and a later ceres_hip_bal_minimize are not affected.
 * The second n x n buffer (n = tangent scalars of the free cameras) is allocated on the first call and released with the handle.
 * Returns CERES_HIP_E_INVALID (message in ceres_hip_bal_last_error; of (NULL) for a NULL handle, which answers before any device call)
 * for a NULL handle, state, summary or pair array, num_pairs < 0, a block index out of range, a non-finite or negative
 * min_scaled_pivot; CERES_HIP_E_UNSUPPORTED for a handle whose linear solver is not CERES_HIP_DENSE_SCHUR, for a sharded handle and
 * for a handle with fixed intrinsics.
 * A rank-deficient problem returns 0 with termination_type = CERES_HIP_FAILURE, the message naming the factorization that failed and
 * the pivot; blocks_out is then not written.  No floating-point atomics: two calls at one state give the same bits. */
int ceres_hip_bal_covariance(ceres_hip_bal* p, const ceres_hip_covariance_options* options, const double* state,
                             int64_t num_pairs, const int32_t* block_a, const int32_t* block_b,
                             double* blocks_out, ceres_hip_covariance_summary* summary);
/* Debug, host only: one LineSearch::Search (ARMIJO or WOLFE as the options say) on a caller's univariate function.  fn(x, want_gradient,
 * value, gradient, user): a non-zero return or a non-finite value is an invalid sample.  direction_max_norm is taken as 1. */
typedef int (*ceres_hip_univariate_fn)(double x, int want_gradient, double* value, double* gradient, void* user);
typedef struct ceres_hip_line_search_result {
  int32_t success, num_function_evaluations, num_gradient_evaluations, num_iterations;
  double optimal_step_size, optimal_value;
  char error[512];
} ceres_hip_line_search_result;
int ceres_hip_debug_line_search(const ceres_hip_line_search_options* options, ceres_hip_univariate_fn fn, void* user, double step_size_estimate,
                                double initial_cost, double initial_gradient, ceres_hip_line_search_result* out);
/* Debug, host only: MinimizeInterpolatingPolynomial (internal/ceres/polynomial.cc) on n samples with 1 to 6 valid values and gradients in all; coefficients_out (may be NULL):
 * the interpolating polynomial, highest power first, one coefficient per valid value or gradient (at most 6). */
int ceres_hip_debug_minimize_interpolating_polynomial(int32_t n, const double* x, const double* value, const int32_t* value_valid,
                                                      const double* gradient, const int32_t* gradient_valid, double x_min, double x_max,
                                                      double* optimal_x, double* optimal_value, double* coefficients_out);
/* Debug, device 0: the L-BFGS operator the minimizer runs.  The num_updates pairs (row-major [num_updates][n]) go through the secant test
 * and the circular buffer in order — accepted_out[k] = 1 / 0 — then direction_out = -H gradient by the two-loop recursion. */
int ceres_hip_debug_lbfgs_direction(int64_t n, int32_t rank, int32_t use_scaling, int32_t num_updates, const double* delta_x,
                                    const double* delta_gradient, const double* gradient, double* direction_out, int32_t* accepted_out);
/* Timing probe of the evaluator that writes the solver's tiles (what ceres_hip_bal_minimize runs per Jacobian evaluation on the
 * fused <2,3,9> path): average microseconds of `iters` back-to-back launches at `state`; flags != 0 switch groups of its stores
 * off (experiments; the handle's Jacobian is unusable afterwards until the next evaluation).                                  */
int ceres_hip_debug_bal_evaluate_tiles_timing(ceres_hip_bal* p, const double* state, int32_t flags, int32_t iters, double* avg_us);

/* ---- timing for the roofline numbers --------------------------------------
 * Runs `iters` back-to-back launches of one operator on the solver's stream
 * with device-resident operands and brackets them with HIP events recorded on
 * that same stream; returns the average milliseconds per application.        */
#define CERES_HIP_TIMED_JTJX 1
#define CERES_HIP_TIMED_SX 2
#define CERES_HIP_TIMED_SCHUR_INIT 3 /* incl. the fused re-layout, as a solve runs it */
#define CERES_HIP_TIMED_SCHUR_JACOBI 4
#define CERES_HIP_TIMED_BACK_SUBSTITUTE 5
#define CERES_HIP_TIMED_PACK 6
#define CERES_HIP_TIMED_BLOCK_JACOBI 7
#define CERES_HIP_TIMED_COPY 8 /* plain device copy of the values array: HBM ceiling probe */
#define CERES_HIP_TIMED_CGNR_SETUP 10 /* CGNR per-step set-up on the <2,3,9> path (re-layout + J^T b + JACOBI blocks) */
#define CERES_HIP_TIMED_READ_STREAM 9 /* read-only pass over the packed tiles, same loads as the fused kernels */
#define CERES_HIP_TIMED_MODEL_COST 11 /* -(J x)'(f + J x / 2) as the LM step forms it where nothing else does (fused path: the kJx pass) */
#define CERES_HIP_TIMED_JACOBIAN_GRAM 12 /* the dogleg strategy's pass over J: what ceres_hip_op_jacobian_gram launches, on device vectors */
/* CLUSTER_JACOBI handles: the gather elimination into the cluster pairs / scatter into the dense cluster matrices + their Cholesky
 * factorisations (re-assembled every time) / one application z = M^-1 r */
#define CERES_HIP_TIMED_CLUSTER_ELIMINATE 13
#define CERES_HIP_TIMED_CLUSTER_FACTOR 14
#define CERES_HIP_TIMED_CLUSTER_APPLY 15
int ceres_hip_time_op(ceres_hip_solver* s, int32_t op, int32_t iters, double* avg_ms);
/* Per-phase event timings (ms) of the most recent ceres_hip_solve* / ceres_hip_lm_compute_step*.  The phases are bracketed by HIP events
 * on the solver's stream, and an event record between two kernels idles the device for about 6 us (a barrier packet with a completion
 * signal; seven of them in a step): they are recorded only after ceres_hip_set_phase_timing(s, 1) (or with CERES_HIP_TIMING=1 in the
 * environment).  Without it only total_ms is filled, from the host's clock around the call, and operator_applications.               */
int ceres_hip_set_phase_timing(ceres_hip_solver* s, int32_t enable);
typedef struct ceres_hip_solve_timing {
  double upload_ms, pack_ms, setup_ms, preconditioner_ms, cg_ms, back_substitute_ms,
      download_ms, total_ms;
  int32_t operator_applications; /* lhs applications inside CG (incl. residual resets) */
  int32_t reserved;
} ceres_hip_solve_timing;
int ceres_hip_get_last_timing(const ceres_hip_solver* s, ceres_hip_solve_timing* t);

/* ---- debug: the host-side tile packing plan of the <2,3,9> path -------------
 * Pure host code (no device needed): lets the CPU test-suite check the plan the
 * fused kernels rely on.  Arrays are sized n_tiles*64 (slots) / n_tiles; call once
 * with slot_capacity = 0 to obtain n_tiles.  slot_row = row block of the slot or -1. */
int ceres_hip_debug_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t* eligible,
                         int64_t* n_tiles, int32_t* slot_row, int32_t* slot_cam, int32_t* slot_pt,
                         uint32_t* slot_seg, int32_t* tile_kind, int32_t* tile_aux, int64_t slot_capacity,
                         char* why_not, int32_t why_capacity);

/* Debug: the plan of the streamed upload (ceres_hip_values_ready).  Pure host code.  *value_streams = 0, 1 or 2; lo / hi (each
 * 2 * num_row_blocks entries, class-major; either may be NULL): row blocks [r0, r1) own the doubles [lo[k][r0], hi[k][r1 - 1]) of the
 * value array in class k < *value_streams (1 stream: whole rows; 2: k = 0 the rows' first cells, k = 1 their other cells). */
int ceres_hip_debug_value_streams(const ceres_hip_block_structure* bs, int32_t* value_streams, int64_t* lo, int64_t* hi);
/* Debug: the handle's own device copies of the loaded values (values_extent doubles) and residuals (num_rows), after waiting for the
 * copy stream and the solver's stream.  Either pointer may be NULL. */
int ceres_hip_debug_read_loaded(ceres_hip_solver* s, double* host_values_out, double* host_residuals_out);

/* Debug: the inner-iteration ordering of a BAL structure (pure host code; what a handle with ceres_hip_bal_set_inner_iterations(p,
 * blocks, ...) runs): group_of_block[num_points + num_cameras] = the group of every block in state order (points, then cameras), -1 for a
 * block outside the ordering; *num_groups.  blocks: CERES_HIP_INNER_AUTOMATIC .. CERES_HIP_INNER_POINTS_CAMERAS. */
int ceres_hip_debug_inner_iteration_ordering(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                             const int32_t* point_index, int32_t blocks, int32_t* group_of_block, int32_t* num_groups);

/* Host-only (no device, like ceres_hip_debug_cluster_cameras): the reduction ceres_hip_bal_create_with_constant_blocks makes —
 * row_observation[*num_rows] (room for num_observations entries), camera_column[num_cameras] / point_column[num_points] = index of the
 * block among the free ones or -1.  CERES_HIP_E_INVALID (message in ceres_hip_bal_last_error(NULL)): NULL index arrays, an index out
 * of range, no free camera, no free point. */
int ceres_hip_debug_bal_reduce(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                               const int32_t* point_index, const uint8_t* camera_is_constant, const uint8_t* point_is_constant,
                               int64_t* num_rows, int64_t* num_rows_e, int32_t* row_observation, int32_t* camera_column,
                               int32_t* point_column);
/* Debug: the camera clustering of CLUSTER_JACOBI (csrc/visibility.cc; pure host code): membership[num_col_blocks - num_eliminate_blocks]
 * = the cluster of every F block, *num_clusters = their number (clusters numbered by ascending first member; the tie-break rule is
 * stated at ceres_hip_options.visibility_clustering_type).  CERES_HIP_E_INVALID for NULL pointers, a structure AnalyzeStructure
 * rejects, no F block, or an unknown clustering type. */
int ceres_hip_debug_cluster_cameras(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t visibility_clustering_type,
                                    int32_t* membership, int32_t* num_clusters);

/* Debug: the subspace dogleg's boundary minimum (DoglegStrategy::FindMinimumOnTrustRegionBoundary and the first-order check of
 * ComputeSubspaceDoglegStep, I/dogleg_strategy.cc:304-336, 473-515; pure host code).  B[4]: the 2x2 model matrix, row-major; g[2]; the
 * radius.  x[2] = the minimiser x of 1/2 x'Bx + g'x over the real parts of all four roots of the quartic, UNSCALED (what the strategy
 * keeps; x * radius / |x| lies on the boundary).  Returns 0, CERES_HIP_DOGLEG_NO_ROOT (no usable root: x = 0) or
 * CERES_HIP_DOGLEG_COSINE (cos(x, -(Bx + g)) < 0.99; x is still the minimiser) — the two cases that fall back to the traditional step;
 * CERES_HIP_E_INVALID for NULL pointers. */
#define CERES_HIP_DOGLEG_NO_ROOT 1
#define CERES_HIP_DOGLEG_COSINE 2
int ceres_hip_debug_dogleg_subspace_minimum(const double* B, const double* g, double radius, double* x);

/* DenseCholesky::FactorAndSolve on a caller-supplied matrix (I/dense_cholesky.cc: what DENSE_SCHUR runs on its reduced system,
 * I/schur_complement_solver.cc:163-222): A is n x n row-major with its UPPER triangle authoritative, x = A^-1 b.  The blocked
 * factorisation (128-wide panels, trailing update on v_mfma_f64_16x16x4_f64) runs `repeats` times from fresh copies; *factor_ms =
 * its average duration (HIP events), *failed = 1 if a pivot was not positive (x is then b).  Needs only a created handle.          */
int ceres_hip_op_dense_cholesky_solve(ceres_hip_solver* s, int32_t n, const double* A, const double* b, double* x, int32_t repeats,
                                      double* factor_ms, int32_t* failed);
/* Debug: the same factorisation with the factor returned and the memory around it watched.  A as above; b (n doubles) may be NULL.
 * The matrix and the vector sit in the middle of larger device allocations: a guard band of 2 * 128 * n doubles on either side of the
 * matrix and of 256 doubles on either side of the vector, filled with the byte 0x5A before the first run.  Each of `repeats` runs
 * starts from a fresh copy, factors on the handle's stream and, with b given and no pivot refused, solves.  factor (n * n doubles):
 * the whole array as the last run left it (L in the lower triangle; above the diagonal whatever the kernels keep there); x (n doubles,
 * required with b): the last run's solution, b itself if a pivot was refused; *failed: the last run's flag; *guard_words_changed: the
 * guard words whose bits differ from the fill after the last run; *repeatable: 1 if every run left the same bits in the lower triangle
 * (and the same flag).  The last three may be NULL.  Needs only a created handle. */
int ceres_hip_op_dense_cholesky_factor(ceres_hip_solver* s, int32_t n, const double* A, const double* b, double* factor, double* x,
                                       int32_t repeats, int32_t* failed, int64_t* guard_words_changed, int32_t* repeatable);

/* Debug: the camera-accumulation plan for more cameras than LDS rows (csrc/plan.cc; pure host code).  With groups >= 2 and
 * num_eliminate_blocks > 0 this is the HYBRID plan a Schur solver builds for `groups` workgroups of `rows` LDS accumulator rows;
 * with groups = 0 the spill-everything plan.  counts[8] = {n_tiles, hybrid (0/1), rows per workgroup, rows shared by every
 * workgroup (the popular cameras), first flush row of the ring, ring rows, entries of the second pass, units of the second pass}.
 * slot_word = camera | accumulator row << 20 (row 0xFFF: the slot is spilled), -1 = padding slot; tile_zbase = ring row of a tile's
 * first spilled slot; group g walks the tiles [grp_tile_ptr[g], grp_tile_ptr[g+1]) and flushes accumulator row r to ring row
 * counts[4] + g rows + r; unit u sums the ring rows entry_row[unit_begin[u] .. unit_end[u]) into camera unit_cam[u].  Call once with
 * capacities 0 for the counts.  Returns CERES_HIP_E_UNSUPPORTED if the structure is not <2,3,9>-shaped or its cameras fit in LDS. */
int ceres_hip_debug_hybrid_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t groups, int32_t rows,
                                int64_t counts[8], int32_t* slot_word, int32_t* slot_row, int32_t* tile_zbase, int32_t* grp_tile_ptr,
                                int32_t* entry_row, int32_t* unit_cam, int32_t* unit_begin, int32_t* unit_end,
                                int64_t slot_capacity, int64_t entry_capacity, int64_t unit_capacity);

/* Debug: where the plan (csrc/plan.cc; pure host code) puts the points of more than 64 observations, and the ROUNDS the streaming
 * kernels take them in.  renumber != 0: the plan of a Schur solver (points renumbered); groups >= 2: the hybrid plan.  The tiles of
 * range g (a hybrid group, or range 0 = everything) are [range_tile_ptr[g], range_tile_ptr[g+1]); from long_ptr[g] on they belong to
 * long points (tile_kind 3 = head of a point that is in the rounds, 1 = of one that is not, tile_aux = its number of tiles;
 * 2 = continuation).  A workgroup takes whole SEQUENCES of rounds: those of range g are [round_ptr[g], round_ptr[g+1]), sequence q is
 * the rounds [seq_ptr[q], seq_ptr[q+1]).  Round r gives wave w the tile round_word[8 r + w] & 0x3FFFFFF (0xFFFFFFFF: none); bits
 * 26..28 = first wave of the point, bits 29..31 = its number of waves - 1; round_flag[r]: 0 = a round of whole points, else 1 (sum)
 * or 2 (apply), + 4 on the last round of the phase: the rounds of ONE point of more than 8 tiles.  counts[5] = {n_tiles, ranges,
 * rounds, long points behind the others (0/1), sequences}.  seq_ptr holds sequences + 1 entries within round_capacity + 1.  Call
 * once with capacities 0 for the counts.                                                                                          */
int ceres_hip_debug_long_rounds(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t renumber, int32_t groups,
                                int32_t rows, int64_t counts[5], int32_t* tile_kind, int32_t* tile_aux, int32_t* range_tile_ptr,
                                int32_t* long_ptr, int32_t* round_ptr, int32_t* seq_ptr, int32_t* round_flag, uint32_t* round_word,
                                int64_t tile_capacity, int64_t range_capacity, int64_t round_capacity);

/* Debug: which cameras' part of x the streaming kernels keep in LDS beside the accumulators (csrc/plan.cc, BalPlan::xhot_cam; pure
 * host code; the plan of a Schur solver when num_eliminate_blocks > 0).  counts[4] = {n_tiles, cameras, staged cameras, LDS bytes the
 * accumulators take}; staged_cam[r] = the camera of LDS row r (most observed first); slot_word = camera | (row + 1) << 20 for a staged
 * camera's slot, camera alone otherwise, -1 = padding slot.  counts[2] = 0 when the accumulators do not all fit in LDS (the hybrid plan's
 * regime) or CERES_HIP_XHOT=0.  Call once with capacities 0 for the counts.  Returns CERES_HIP_E_UNSUPPORTED for structures off the fused path. */
int ceres_hip_debug_staged_x_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int64_t counts[4], int32_t* staged_cam,
                                  int32_t* slot_word, int64_t staged_capacity, int64_t slot_capacity);

/* Debug: exercise the sharded (world > 1) code paths on one GPU through a 1-rank RCCL
 * communicator; the instance must then be given the WHOLE problem.  Call before set_structure. */
int ceres_hip_debug_comm_loopback(ceres_hip_solver* s, int32_t logical_world);
/* Measurement (bench.py: extra.shard_ceiling): this instance becomes rank 0 of `logical_world` ranks whose PEERS ARE GHOSTS.  The
 * peer-to-peer all-reduce kernel does all its work — pushes into every peer's slot, sets and awaits every peer's flags, adds the
 * `world` slots in rank order — against local dummy buffers that read "arrived" with zero contributions.  Given ONE RANK'S SHARD of
 * a problem the instance runs the sharded code path alone on the device: the time a perfect interconnect would give that rank
 * (its sums are the shard's own, so its results are not the whole problem's).  Call before set_structure; max_elements as for
 * ceres_hip_comm_p2p_prepare.                                                                                                  */
int ceres_hip_debug_comm_ghost_peers(ceres_hip_solver* s, int32_t logical_world, int64_t max_elements);

#ifdef __cplusplus
}
#endif
#endif /* CERES_HIP_H_ */
