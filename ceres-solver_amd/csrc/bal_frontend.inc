// SURVEY.md §8 f4 — the Evaluator side of the boundary for BAL problems and the trust-region loop
// around the linear solvers.  Textually included at the end of solver.hip (it drives the solver
// through its internal operators: op_jtb, op_squared_column_norm, lm_step_loaded).
//
//   ceres_hip_bal_evaluate  = Evaluator::Evaluate              I/evaluator.h:116-124
//   ceres_hip_bal_minimize  = TrustRegionMinimizer::Minimize   I/trust_region_minimizer.cc:68-845
//                             with LevenbergMarquardtStrategy  I/levenberg_marquardt_strategy.cc:69-157
//                             or DoglegStrategy                I/dogleg_strategy.cc (dogleg.inc)
//   ceres_hip_bal_minimize_line_search = LineSearchMinimizer::Minimize   I/line_search_minimizer.cc (line_search.inc)
//   ceres_hip_bal_set_bounds = Problem::SetParameterLowerBound / SetParameterUpperBound: the projection inside Plus, the projected
//                             gradient norm and DoLineSearch of the loop below (bounds.inc)
// The loop below follows the reference statement by statement (the same restatement as
// oracle/bal_harness.cc, which is what the parity tests compare it with); only the places
// where vectors live differ: everything of size num_parameters / num_residuals stays in HBM.
#include "bal_layout.h"

struct ceres_hip_bal {
  ceres_hip_solver* s = nullptr;
  std::string err;
  int nc = 0, np = 0;
  int64_t no = 0;
  // CERES_HIP_CAMERA_* (ceres_hip_bal_create_with_camera): state doubles (cs) and Jacobian columns (cw) per camera; the state is ambient
  // (n_a = 3 n_p + cs n_c: d_x, d_cand, the caller's state), the step, scale, delta and gradient are tangent (n_t = 3 n_p + cw n_c)
  int32_t camera_model = CERES_HIP_CAMERA_ANGLE_AXIS;
  int cs = 9, cw = 9;
  int64_t n_a = 0, n_t = 0;
  std::vector<int32_t> row_obs;  // residual row block -> observation
  int32_t *d_row_cam = nullptr, *d_row_pt = nullptr;
  double2* d_row_obs = nullptr;
  // the same three in SLOT order (the tile-order evaluator), and its {state, scale} records
  int32_t *d_slot_cam = nullptr, *d_slot_pt = nullptr;
  double2* d_slot_obs = nullptr;
  double *d_pt_pack = nullptr, *d_cam_pack = nullptr;
  // point and pixel of every entry of the solver's camera-major list (the preconditioner pass that evaluates its F cells)
  int32_t* d_cm_pt = nullptr;
  double2* d_cm_obs = nullptr;
  double *d_x = nullptr, *d_cand = nullptr, *d_res = nullptr, *d_vals = nullptr, *d_step = nullptr, *d_delta = nullptr,
         *d_scale = nullptr, *d_grad = nullptr;
  PartialSums parts;            // every per-workgroup partial sum this file and its .inc files read back (partial_sums.h)
  LossParams loss;              // ceres_hip_bal_set_loss: applies to every observation (kLossNone: the squared loss)
  // ceres_hip_bal_set_inner_iterations (inner_iterations.inc): CERES_HIP_INNER_*, in force until set again; the lists it runs on; and
  // what the last ceres_hip_bal_minimize did with them (ceres_hip_bal_inner_iteration_stats)
  int32_t inner_blocks = 0;
  double inner_tolerance = 1e-3;
  struct BalInner* inner = nullptr;
  int32_t inner_steps = 0, inner_groups_used = 0;
  double inner_seconds = 0.0;
  // ceres_hip_bal_set_trust_region_strategy (dogleg.inc): CERES_HIP_LEVENBERG_MARQUARDT / CERES_HIP_DOGLEG, in force until set again;
  // the dogleg strategy's device vectors (a = gradient / diagonal, b = gn / diagonal), made on first use
  int32_t tr_strategy = CERES_HIP_LEVENBERG_MARQUARDT, dogleg_type = CERES_HIP_TRADITIONAL_DOGLEG;
  double *d_dl_a = nullptr, *d_dl_b = nullptr;
  // ceres_hip_bal_create_with_constant_blocks (constant_blocks.inc): nc, np and n_a stay the caller's (the state is full), `no` is the
  // number of KEPT rows, n_t the reduced tangent length.  Everything below is unset on a handle without constant blocks.
  bool has_const = false;
  int nfc = 0, nfp = 0;                        // free cameras / points (= nc, np without constants)
  int64_t n_rows_e = 0, n_rows_f = 0;          // rows with an E cell (they come first) / with an F cell
  std::vector<int32_t> cam_col, pt_col;        // block -> index among the free ones, -1: constant
  std::vector<int32_t> all_cam, all_pt;        // the caller's observations, every one (the inner iterations' lists; the removed rows)
  std::vector<double> all_obs;
  int32_t *d_row_fpos = nullptr, *d_row_scam = nullptr, *d_row_spt = nullptr;   // BalEvalArgs' per-row positions
  int64_t n_removed = 0;                       // rows removed (both blocks constant) and their camera / point / pixel: the fixed cost
  int32_t *d_rm_cam = nullptr, *d_rm_pt = nullptr;
  double2* d_rm_obs = nullptr;
  int64_t* d_free_block = nullptr;             // BalFreeBlocks::block
  int32_t *d_pack_cam = nullptr, *d_pack_scale = nullptr;   // BalEvalTilesArgs' camera records (constant cameras on the tile path)
  double2* d_scrap = nullptr;
  // ceres_hip_bal_create_with_fixed_intrinsics (SubsetManifold on every camera; kernels_subset.hip): bit k set — coordinate 6 + k of every
  // camera is constant.  cs stays 9, cw = 9 - bits; 0 on every other handle
  int intrinsics_mask = 0;
  // ceres_hip_bal_create_with_shared_intrinsics (kernels_shared.hip): the number of intrinsics groups, 0 on every other handle.  cs stays
  // 9, cw = 6 (the pose); the tangent is [points | free cameras' poses | groups], n_t = 3 np + 6 nfc + 3 n_groups; every row has an E
  // cell and a group cell, the rows of free cameras a pose cell between them.  group_of / group_first: a camera's group, a group's
  // first camera (the one the state check compares the others with, the one that adds the group's norms in Plus)
  int n_groups = 0;
  std::vector<int32_t> group_of, group_first;
  int32_t *d_row_gpos = nullptr, *d_row_sgrp = nullptr, *d_cam_pose = nullptr, *d_cam_group = nullptr, *d_cam_first = nullptr;
  // ceres_hip_bal_evaluate_gradient / ceres_hip_bal_minimize_line_search (line_search.inc): their lists and vectors, made on first use
  struct BalLineSearch* ls = nullptr;
  // ceres_hip_bal_covariance (covariance.inc): its lists and buffers, made on first use
  struct BalCovariance* cov = nullptr;
  // ceres_hip_bal_set_bounds (bounds.inc, kernels_bounds.hip): some coordinate of a free block has a finite bound — the one field
  // ceres_hip_bal_minimize tests before anything it does for bounds; the bounds on the device (ambient layout, -inf / +inf: none), made
  // by the first call that constrains the handle; the host copies, the search's options and the statistics
  bool is_constrained = false;
  double *d_lower = nullptr, *d_upper = nullptr;
  struct BalBoundsState* bounds = nullptr;
};
void bal_inner_free(ceres_hip_bal* p);
void bal_ls_free(ceres_hip_bal* p);
void bal_cov_free(ceres_hip_bal* p);
void bal_bounds_free(ceres_hip_bal* p);

namespace {

// the stage's capacity, the largest round trip: an evaluator's cost set + seven vector sets (trial point 2 | 4, norms 2 | 0, dots 3)
constexpr int kPartialSumsCapacity = kMaxEvalGrid + 7 * kMaxVecGrid;
BalBounds bal_bounds_args(const ceres_hip_bal* p);   // (bounds.inc)
double bal_bounds_step_size(const ceres_hip_bal* p);

int bal_fail(ceres_hip_bal* p, int code) {
  if (p && p->s) p->err = p->s->err;
  return code;
}
#define BAL_TRY(p, expr)                    \
  do {                                      \
    int _rc = (expr);                       \
    if (_rc != 0) return bal_fail(p, _rc);  \
  } while (0)

// The handle's stage of partial sums (partial_sums.h).  A refusal is an error of the call, which abandons its round trip.
int bal_parts_refused(ceres_hip_bal* p) { return fail(p->s, CERES_HIP_E_HIP, "%s", p->parts.refusal().c_str()); }
int bal_parts_room(ceres_hip_bal* p, int max_doubles, double** at) {
  *at = p->parts.room(max_doubles);
  return *at ? 0 : bal_parts_refused(p);
}
int bal_parts_collect(ceres_hip_bal* p) {
  if (!p->parts.error.empty()) return bal_parts_refused(p);
  HIP_TRY(p->s, p->parts.collect(p->s->stream));
  return 0;
}
// Jacobian values of the program: E cells, F cells, and with shared intrinsics a group cell per row
int64_t bal_num_values(const ceres_hip_bal* p) { return 6 * p->n_rows_e + 2 * p->cw * p->n_rows_f + (p->n_groups ? 6 * p->no : 0); }
// A block's index among the free ones, -1: constant — the identity on a handle without constant blocks (which keeps no map)
int bal_point_column(const ceres_hip_bal* p, int q) { return p->has_const ? p->pt_col[q] : q; }
int bal_camera_column(const ceres_hip_bal* p, int c) { return p->has_const ? p->cam_col[c] : c; }

// a pixel list (two doubles per entry) as the kernels take it
int dev_upload_pixels(ceres_hip_solver* s, double2** d, const std::vector<double>& pixels) {
  double* q = nullptr;
  TRY(dev_upload(s, &q, pixels));
  *d = reinterpret_cast<double2*>(q);
  return 0;
}

// The handle's rows back on the host for the lists built on first use: the arrays asked for, copied on the solver's stream, one synchronisation.
// The handle keeps no host copy — 28 bytes per row.  fpos: the value position of a row's F cell; a handle that uploaded none has one in every row.
enum : int { kRowCam = 1, kRowPt = 2, kRowPixel = 4, kRowFpos = 8 };
struct BalHostRows { std::vector<int32_t> cam, pt, fpos; std::vector<double> pixel; };
int bal_fetch_rows(ceres_hip_bal* p, int which, BalHostRows& H) {
  ceres_hip_solver* s = p->s;
  const size_t no = size_t(p->no);
  auto fetch = [&](auto& host, const void* dev, size_t n) { host.resize(n); return hipMemcpyAsync(host.data(), dev, n * sizeof(host[0]), hipMemcpyDeviceToHost, s->stream); };
  if (which & kRowCam) HIP_TRY(s, fetch(H.cam, p->d_row_cam, no));
  if (which & kRowPt) HIP_TRY(s, fetch(H.pt, p->d_row_pt, no));
  if (which & kRowPixel) HIP_TRY(s, fetch(H.pixel, p->d_row_obs, 2 * no));
  if ((which & kRowFpos) && p->d_row_fpos) HIP_TRY(s, fetch(H.fpos, p->d_row_fpos, no));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if ((which & kRowFpos) && !p->d_row_fpos) {
    H.fpos.resize(no);
    for (size_t r = 0; r < no; ++r) H.fpos[r] = int32_t(6 * p->n_rows_e + 2 * int64_t(p->cw) * int64_t(r));
  }
  return 0;
}

// Shared intrinsics: the doubles 6 .. 8 of a group's cameras are one parameter block — bit-identical, checked on the host before any
// device call of an entry point that takes a state.  0, or CERES_HIP_E_INVALID naming the first offending camera and coordinate.
int bal_shared_check(ceres_hip_bal* p, const char* fn, const double* state) {
  if (!p->n_groups) return 0;
  for (int c = 0; c < p->nc; ++c) {
    const int f = p->group_first[p->group_of[c]];
    if (f == c) continue;
    const double* a = state + 3 * int64_t(p->np) + 9 * int64_t(c) + 6;
    const double* b = state + 3 * int64_t(p->np) + 9 * int64_t(f) + 6;
    for (int j = 0; j < 3; ++j) {
      if (memcmp(a + j, b + j, sizeof(double)) == 0) continue;
      p->err = std::string(fn) + ": shared intrinsics: camera " + std::to_string(c) + " coordinate " + std::to_string(6 + j) +
               " differs from camera " + std::to_string(f) + ", the first of group " + std::to_string(p->group_of[c]) +
               " (the intrinsics of a group must be bit-identical)";
      return CERES_HIP_E_INVALID;
    }
  }
  return 0;
}

// cost (and residuals / Jacobian values in the solver's layout) at a device state vector, enqueued: *cost is the set of its partial sums
// (removed_rows: over the rows whose blocks are both constant instead — the fixed cost)
int bal_evaluate_enqueue(ceres_hip_bal* p, const double* d_state, bool jacobian, const double* d_scale, double* d_residuals, PartialSet* cost,
                         bool removed_rows = false) {
  ceres_hip_solver* s = p->s;
  BalEvalConstArgs A;
  TRY(bal_parts_room(p, kMaxEvalGrid, &A.partials));
  A.n_rows = p->no; A.row_cam = p->d_row_cam; A.row_pt = p->d_row_pt; A.row_obs = p->d_row_obs;
  if (removed_rows) { A.n_rows = p->n_removed; A.row_cam = p->d_rm_cam; A.row_pt = p->d_rm_pt; A.row_obs = p->d_rm_obs; }
  A.state = d_state; A.cam_base = 3 * int64_t(p->np); A.scale = d_scale;
  A.residuals = d_residuals; A.values = jacobian ? p->d_vals : nullptr; A.loss = p->loss;
  int nparts = 0;
  if (p->n_groups && jacobian) {   // shared intrinsics: a pose cell and a group cell per row (the cost alone has no cell to split)
    BalEvalSharedArgs H;
    static_cast<BalEvalArgs&>(H) = A;
    H.row_fpos = p->d_row_fpos; H.row_scam = p->d_row_scam; H.row_spt = p->d_row_spt; H.row_gpos = p->d_row_gpos; H.row_sgrp = p->d_row_sgrp;
    HIP_TRY(s, LaunchBalEvaluateShared(H, &nparts, s->stream));
  } else if (p->intrinsics_mask && jacobian) {   // fixed intrinsics: F cells of 2 x cw (the cost alone has no columns to remove)
    A.row_fpos = p->d_row_fpos; A.row_scam = p->d_row_scam; A.row_spt = p->d_row_spt;   // (uploaded with or without constant blocks)
    HIP_TRY(s, LaunchBalEvaluateSubset(A, p->intrinsics_mask, &nparts, s->stream));
  } else if (p->has_const && jacobian) {   // a reduced program: the cells of constant blocks are neither scaled nor stored
    A.row_fpos = p->d_row_fpos; A.row_scam = p->d_row_scam; A.row_spt = p->d_row_spt;
    HIP_TRY(s, LaunchBalEvaluateConst(A, &nparts, s->stream, p->camera_model));
  } else {
    HIP_TRY(s, LaunchBalEvaluate(A, jacobian, &nparts, s->stream, p->camera_model));
  }
  *cost = p->parts.take(nparts);
  return 0;
}
int bal_evaluate_device(ceres_hip_bal* p, const double* d_state, bool jacobian, const double* d_scale, double* d_residuals, double* cost,
                        bool removed_rows = false) {
  PartialSet c;
  TRY(bal_evaluate_enqueue(p, d_state, jacobian, d_scale, d_residuals, &c, removed_rows));
  TRY(bal_parts_collect(p));
  *cost = p->parts.sum(c);
  return 0;
}

// Can the evaluator write the solver's tiles itself?  (the fused <2,3,9> path with fp64 tiles; CERES_HIP_EVAL_TILES=0: the two-pass
// form — caller-layout values, re-laid-out by the gradient's pass — for A/B runs and as the cross-check of the tests)
bool bal_writes_tiles(const ceres_hip_bal* p) {
  const ceres_hip_solver* s = p->s;
  // (the tile evaluator computes the angle-axis Jacobian: quaternion cameras keep the two-pass form — the manifold's <2,3,9> included)
  if (p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS) return false;
  if (p->intrinsics_mask || p->n_groups) return false;   // (the tile evaluator writes <2,3,9> tiles)
  // (constant blocks: the tile evaluator's records exist for constant cameras alone — constant points leave remainder rows anyway)
  if (p->has_const && !p->d_pack_cam) return false;
  if (const char* e = getenv("CERES_HIP_EVAL_TILES")) if (atoi(e) == 0) return false;
  // (DENSE_SCHUR forms S from the caller-layout values, E cells included: it keeps the two-pass form)
  return s->path == CERES_HIP_PATH_BAL && s->ops && s->ops->ne == 3 && s->ops->nf == 9 && s->ops->ns == 0 && !s->d_Jf && s->d_J && s->world <= 1 &&
         !has_remainder(s) && !is_dense_schur(s) && !is_cluster_jacobi(s) && p->d_slot_obs &&   // (CLUSTER_JACOBI eliminates from the caller layout too)
         // (cameras' sums outside LDS AND no block preconditioner: the LM diagonal's column norms come from the generic kernel on every
         // fresh step — lm_step_loaded, StepRequest::fuse — which reads the caller layout)
         (s->lds_mode || s->opt.preconditioner_type != CERES_HIP_IDENTITY);
}

// The camera-major passes (preconditioner blocks, F^T F) evaluate their F cells from the records the tile-order evaluator leaves — no
// caller-layout copy of the Jacobian exists then — or read them from p->d_vals (CERES_HIP_EVAL_TILES=2: always; 3: never).
bool bal_camera_pass_evaluates(const ceres_hip_bal* p) {
  if (p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS) return false;   // (the evaluating pass is angle-axis)
  if (p->intrinsics_mask || p->n_groups) return false;                // (and nine columns wide)
  if (const char* e = getenv("CERES_HIP_EVAL_TILES")) {
    if (atoi(e) == 2) return false;
    if (atoi(e) == 3) return p->d_cm_obs != nullptr;   // (tests: the evaluating kernel whatever the item length)
  }
  // where the camera-major pass would take the matrix-pipe kernel (items of a few hundred observations at most: kernels_bal.inc,
  // CameraItems) it keeps it, on a caller-layout copy of the F cells: the evaluating kernel is the lane-per-observation form, whose
  // wavefront reductions dominate short items (Ladybug shape, 50 000 cameras of 60 observations: no gain from evaluating)
  const CamItems& I = p->s->cam_items;
  return p->d_cm_obs != nullptr && I.observations >= int64_t(384) * I.count;
}
void bal_set_camera_eval(ceres_hip_bal* p, bool on) {
  CamItems& I = p->s->cam_items;
  I.ev_cam_pack = on ? p->d_cam_pack : nullptr; I.ev_pt_pack = on ? p->d_pt_pack : nullptr;
  I.ev_pt = on ? p->d_cm_pt : nullptr; I.ev_obs = on ? p->d_cm_obs : nullptr;
  I.ev_loss = p->loss;
}

// The tile-order evaluator's arguments, all but the room for its partial sums; values: where the F cells' caller-layout copy goes, or nullptr
BalEvalTilesConstArgs bal_tile_args(const ceres_hip_bal* p, const double* d_state, const double* d_scale, double* values, int debug_flags) {
  const ceres_hip_solver* s = p->s;
  BalEvalTilesConstArgs T;
  T.debug_flags = debug_flags;
  T.e.n_rows = p->no; T.e.row_cam = p->d_row_cam; T.e.row_pt = p->d_row_pt; T.e.row_obs = p->d_row_obs;
  T.e.state = d_state; T.e.cam_base = 3 * int64_t(p->np); T.e.scale = d_scale;
  T.e.residuals = p->d_res; T.e.values = values; T.e.loss = p->loss;
  T.n_tiles = s->plan.n_tiles; T.slot_bpos = s->d_slot_bpos; T.slot_fpos = s->d_slot_fpos;
  T.J_out = s->d_J; T.tile_pitch = s->ops->tile_pitch; T.b_out = s->d_bt;
  T.slot_cam = p->d_slot_cam; T.slot_pt = p->d_slot_pt; T.slot_obs = p->d_slot_obs; T.pt_pack = p->d_pt_pack; T.cam_pack = p->d_cam_pack;
  T.pack_cam = p->d_pack_cam; T.pack_scale = p->d_pack_scale; T.n_pack_cams = p->nc; T.scrap = p->d_scrap;   // (constant cameras; nullptr otherwise)
  return T;
}

// Cost, residuals and the (scaled) Jacobian at a device state vector, the Jacobian written STRAIGHT INTO THE TILES (kernels_evaluator.hip):
// afterwards the solver holds loaded, packed values — its first pass over J gathers nothing.  Of the caller layout only the F cells
// exist (p->d_vals; the camera-major preconditioner pass reads them there).  Enqueued, as bal_evaluate_enqueue.
int bal_evaluate_into_tiles(ceres_hip_bal* p, const double* d_state, const double* d_scale, PartialSet* cost, int debug_flags = 0) {
  ceres_hip_solver* s = p->s;
  const bool cam_eval = debug_flags == 0 && bal_camera_pass_evaluates(p);
  BalEvalTilesConstArgs T = bal_tile_args(p, d_state, d_scale, cam_eval ? nullptr : p->d_vals, debug_flags);
  TRY(bal_parts_room(p, kMaxEvalGrid, &T.e.partials));
  TRY(load_device(s, p->d_vals, p->d_res, nullptr));   // (marks the tiles stale: they are, until the launch below is enqueued)
  bal_set_camera_eval(p, cam_eval);
  int nparts = 0;
  if (p->has_const) HIP_TRY(s, LaunchBalEvaluateTilesConst(T, p->np, &nparts, s->stream));
  else HIP_TRY(s, LaunchBalEvaluateTiles(T, p->np, p->nc, &nparts, s->stream));
  s->packed = true;
  s->tiles_only = true;   // (E cells are never written; F cells only for the camera-major pass that reads them)
  *cost = p->parts.take(nparts);
  return 0;
}

// max |g_i / scale_i| — with quaternion-manifold cameras |x - Plus(x, -g)|_inf at the state d_x — enqueued: *out is the set of maxima
int bal_gradient_max(ceres_hip_bal* p, const double* d_scale, const double* d_x, PartialSet* out) {
  ceres_hip_solver* s = p->s;
  int nparts = 0; double* parts = nullptr;
  TRY(bal_parts_room(p, kMaxVecGrid, &parts));
  if (p->is_constrained)   // |x - clamp(x - g)|_inf over the free blocks (I/trust_region_minimizer.cc:281-302)
    HIP_TRY(s, LaunchBoundsGradientMax(bal_bounds_args(p), d_x, p->d_grad, d_scale, parts, &nparts, s->stream));
  else if (p->camera_model == CERES_HIP_CAMERA_QUATERNION_MANIFOLD && p->has_const)
    HIP_TRY(s, LaunchBalGradientMaxQuatFree(BalFreeBlocks{p->d_free_block, p->nfp, p->nfc}, p->d_grad, d_scale, d_x, parts, &nparts, s->stream));
  else if (p->camera_model == CERES_HIP_CAMERA_QUATERNION_MANIFOLD)
    HIP_TRY(s, LaunchBalGradientMaxQuat(p->d_grad, d_scale, d_x, p->np, p->nc, parts, &nparts, s->stream));
  else
    HIP_TRY(s, LaunchBalGradientMax(p->d_grad, d_scale, p->n_t, parts, &nparts, s->stream));
  *out = p->parts.take(nparts);
  return 0;
}

// delta = step .* scale, cand = Plus(x, delta), enqueued; the sets of |x|^2 and |delta|^2
// (a constrained handle: delta = a (step .* scale) with the projected search's step size a, cand = clamp(x + delta), and the second
// sum is |cand - x|^2, Ceres' ambient step norm; the kernel's two further sets are taken and not read)
int bal_candidate(ceres_hip_bal* p, const double* x, const double* scale, double* cand, PartialSet* x_norm2, PartialSet* delta_norm2) {
  ceres_hip_solver* s = p->s;
  int n = 0; double* parts = nullptr;
  TRY(bal_parts_room(p, (p->is_constrained ? 4 : 2) * kMaxVecGrid, &parts));
  if (p->is_constrained)
    HIP_TRY(s, LaunchBoundsTrialPoint(bal_bounds_args(p), x, p->d_step, scale, nullptr, bal_bounds_step_size(p), true, p->d_delta, cand, parts,
                                      &n, s->stream));
  else if (p->n_groups)   // (shared intrinsics: one group step for many cameras; constant poses are copied)
    HIP_TRY(s, LaunchBalCandidateShared(BalSharedCameras{p->np, p->nc, p->d_cam_pose, p->d_cam_group, p->d_cam_first}, x, p->d_step, scale,
                                        p->d_delta, cand, parts, &n, s->stream));
  else if (p->intrinsics_mask)   // (fixed intrinsics: a narrower step scattered into the free coordinates, with or without constant blocks)
    HIP_TRY(s, LaunchBalCandidateSubset(BalFreeBlocks{p->has_const ? p->d_free_block : nullptr, p->nfp, p->nfc}, p->intrinsics_mask, p->np, x,
                                        p->d_step, scale, p->d_delta, cand, parts, &n, s->stream));
  else if (p->has_const)   // (Plus scattered into the free blocks; cand's constant blocks hold the state's values already: ceres_hip_bal_minimize)
    HIP_TRY(s, LaunchBalCandidateFree(BalFreeBlocks{p->d_free_block, p->nfp, p->nfc}, p->camera_model, x, p->d_step, scale, p->d_delta, cand, parts,
                                      &n, s->stream));
  else if (p->camera_model == CERES_HIP_CAMERA_QUATERNION_MANIFOLD)
    HIP_TRY(s, LaunchBalCandidateQuat(x, p->d_step, scale, p->d_delta, cand, p->np, p->nc, parts, &n, s->stream));
  else   // (the angle-axis and the Euclidean quaternion camera: Plus is x + delta)
    HIP_TRY(s, LaunchBalCandidate(x, p->d_step, scale, p->d_delta, cand, p->n_a, parts, &n, s->stream));
  *x_norm2 = p->parts.take(n); *delta_norm2 = p->parts.take(n);
  if (p->is_constrained) { p->parts.take(n); p->parts.take(n); }
  return 0;
}

// Solver::Summary::fixed_cost at a device state vector: the cost-only evaluator over the removed rows (both blocks constant), its
// partial sums added in their fixed order
int bal_fixed_cost_device(ceres_hip_bal* p, const double* d_state, double* cost) {
  *cost = 0.0;
  return p->n_removed == 0 ? 0 : bal_evaluate_device(p, d_state, false, nullptr, nullptr, cost, true);
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

#include "constant_blocks.inc"
#include "inner_iterations.inc"
#include "dogleg.inc"
#include "line_search.inc"
#include "bounds.inc"
#include "covariance.inc"

extern "C" {

void ceres_hip_minimizer_default_options(ceres_hip_minimizer_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;            // include/ceres/solver.h defaults
  o->jacobi_scaling = 1;
  o->max_consecutive_invalid_steps = 5;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_relative_decrease = 1e-3;
  o->eta = 1e-1;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
}

const char* ceres_hip_bal_last_error(const ceres_hip_bal* p) { return p ? p->err.c_str() : g_create_error.c_str(); }
ceres_hip_solver* ceres_hip_bal_linear_solver(ceres_hip_bal* p) { return p ? p->s : nullptr; }

void ceres_hip_bal_destroy(ceres_hip_bal* p) {
  if (!p) return;
  if (p->parts.pinned) (void)hipHostFree(p->parts.pinned);
  bal_inner_free(p);
  bal_ls_free(p);
  bal_cov_free(p);
  bal_bounds_free(p);
  if (p->s) ceres_hip_destroy(p->s);  // frees every device allocation made through dev_alloc
  delete p;
}

}  // extern "C"

namespace {

// ceres_hip_bal_create, ceres_hip_bal_create_with_camera, ceres_hip_bal_create_with_constant_blocks, ceres_hip_bal_create_with_fixed_intrinsics
// and ceres_hip_bal_create_with_shared_intrinsics (`fn` names the entry point in the messages), in three stages.  The masks may be NULL;
// with none set the reduction is the identity, the camera keeps its width and the handle is what it always was.
ceres_hip_bal* bal_create(const char* fn, const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras, int32_t num_points,
                          int64_t num_observations, const int32_t* camera_index, const int32_t* point_index,
                          const double* observations, const uint8_t* camera_is_constant = nullptr,
                          const uint8_t* point_is_constant = nullptr, const uint8_t* camera_coordinate_is_constant = nullptr,
                          const int32_t* camera_group = nullptr, int32_t num_groups = 0) try {   // (host vectors sized by the caller's counts: no C++ exception crosses the C boundary)
  const std::string name(fn);
  static_assert(kCamAngleAxis == CERES_HIP_CAMERA_ANGLE_AXIS && kCamQuaternion == CERES_HIP_CAMERA_QUATERNION &&
                kCamQuaternionManifold == CERES_HIP_CAMERA_QUATERNION_MANIFOLD, "device camera models are the ABI's");
  static_assert(kBalAngleAxis == kCamAngleAxis && kBalQuaternion == kCamQuaternion && kBalQuaternionManifold == kCamQuaternionManifold, "and the layout's");
  // ---- 1. validate and lay out (bal_layout.h); a local: the handle keeps of it what is moved or copied below
  BalLayout L;
  const std::string why = !options && bal_camera_model_known(camera_model) ? "bad arguments"
      : bal_layout(camera_model, num_cameras, num_points, num_observations, camera_index, point_index, observations, camera_is_constant,
                   point_is_constant, camera_coordinate_is_constant, camera_group, num_groups, L);
  if (!why.empty()) {
    g_create_error = name + ": " + why;
    return nullptr;
  }
  // ---- 2. the linear solver and its structure
  ceres_hip_options o = *options;
  o.num_eliminate_blocks = L.nfp();
  ceres_hip_solver* s = ceres_hip_create(&o);
  if (!s) return nullptr;
  ceres_hip_bal* p = new ceres_hip_bal;
  p->s = s;
  const int64_t no = L.n_rows;
  p->nc = num_cameras; p->np = num_points; p->no = no;
  p->nfc = L.nfc(); p->nfp = L.nfp(); const bool has_const = p->has_const = L.has_const;
  p->camera_model = camera_model; p->cs = L.cs; p->cw = L.cw; p->intrinsics_mask = L.intrinsics_mask;
  p->n_a = L.n_a; p->n_t = L.n_t; p->n_rows_e = L.n_rows_e; p->n_rows_f = L.n_rows_f; p->n_removed = int64_t(L.rm_cam.size());
  p->n_groups = L.n_groups; p->group_first = L.group_first;
  if (L.n_groups) p->group_of.assign(camera_group, camera_group + num_cameras);
  p->row_obs = std::move(L.red.row_obs);
  if (has_const) {   // the reduced program's maps, the caller's observations (the inner iterations' lists)
    p->cam_col = L.red.camera_column; p->pt_col = L.red.point_column;
    p->all_cam.assign(camera_index, camera_index + num_observations);
    p->all_pt.assign(point_index, point_index + num_observations);
    p->all_obs.assign(observations, observations + 2 * num_observations);
  }
  auto bail = [&](const char* what) -> ceres_hip_bal* {
    g_create_error = std::string(what) + ": " + s->err;
    ceres_hip_bal_destroy(p);
    return nullptr;
  };
  ceres_hip_block_structure flat{int32_t(no), int32_t(L.col_size.size()), L.row_size.data(), L.row_pos.data(), L.col_size.data(), L.col_pos.data(),
                                 L.row_ptr.data(), L.cell_col.data(), L.cell_pos.data()};
  if (ceres_hip_set_structure(s, &flat) != CERES_HIP_OK) return bail((name + ": set_structure").c_str());
  if (hipSetDevice(s->opt.device) != hipSuccess) return bail((name + ": hipSetDevice").c_str());
  // ---- 3. upload: a flat list, every line one device array of the handle
  auto U = [&](auto** d, const auto& v) { return dev_upload(s, d, v) == 0; };
  auto P = [&](double2** d, const std::vector<double>& v) { return dev_upload_pixels(s, d, v) == 0; };
  auto A = [&](auto** d, size_t n) { return dev_alloc(s, d, n) == 0; };
  bool ok = U(&p->d_row_cam, L.row_cam) && U(&p->d_row_pt, L.row_pt) && P(&p->d_row_obs, L.row_pixel) &&
            A(&p->d_x, size_t(p->n_a)) && A(&p->d_cand, size_t(p->n_a)) &&
            A(&p->d_step, size_t(p->n_t)) && A(&p->d_delta, size_t(p->n_t)) && A(&p->d_scale, size_t(p->n_t)) && A(&p->d_grad, size_t(p->n_t)) &&
            A(&p->d_res, size_t(2 * no)) && A(&p->d_vals, size_t(L.n_values)) && A(&p->parts.device, size_t(kPartialSumsCapacity));
  // the evaluators' per-row positions: constant blocks, fixed or shared intrinsics (kernels_constant.hip, kernels_subset.hip, kernels_shared.hip)
  if (has_const || L.intrinsics_mask || L.n_groups) ok = ok && U(&p->d_row_fpos, L.row_fpos) && U(&p->d_row_scam, L.row_scam) && U(&p->d_row_spt, L.row_spt);
  if (has_const) ok = ok && U(&p->d_free_block, L.free_block);
  if (has_const && p->n_removed > 0) ok = ok && U(&p->d_rm_cam, L.rm_cam) && U(&p->d_rm_pt, L.rm_pt) && P(&p->d_rm_obs, L.rm_pixel);
  if (L.n_groups)   // shared intrinsics: the group cell's positions, and Plus' per-camera records (kernels_shared.hip)
    ok = ok && U(&p->d_row_gpos, L.row_gpos) && U(&p->d_row_sgrp, L.row_sgrp) && U(&p->d_cam_pose, L.cam_pose) && U(&p->d_cam_group, L.cam_group) &&
         U(&p->d_cam_first, L.cam_first);
  // the tile evaluator's and the evaluating camera-major pass's records, where the fused path's plan and the layout have them
  const BalRecords K = s->path == CERES_HIP_PATH_BAL ? bal_records(L, s->plan.slot_bpos, s->plan.cam_ptr, s->plan.cam_fpos) : BalRecords{};
  if (K.slots)
    ok = ok && U(&p->d_slot_cam, K.slot_cam) && U(&p->d_slot_pt, K.slot_pt) && P(&p->d_slot_obs, K.slot_pixel) &&
         A(&p->d_pt_pack, size_t(6) * num_points) && A(&p->d_cam_pack, size_t(18) * num_cameras);
  if (K.slots && has_const) ok = ok && U(&p->d_pack_cam, K.pack_cam) && U(&p->d_pack_scale, K.pack_scale) && A(&p->d_scrap, K.slot_cam.size());
  if (K.camera_major) ok = ok && U(&p->d_cm_pt, K.cm_pt) && P(&p->d_cm_obs, K.cm_pixel);
  // (every upload above is a stream copy that reads a vector of L or K, gone at the return: one wait for all, on every path, as the on-demand builders wait)
  ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
  if (!ok) return bail((name + ": device allocation").c_str());
  if (hipHostMalloc(reinterpret_cast<void**>(&p->parts.pinned), sizeof(double) * kPartialSumsCapacity) != hipSuccess)
    return bail((name + ": pinned allocation").c_str());
  p->parts.capacity = kPartialSumsCapacity;
  return p;
} catch (const std::exception& ex) {
  g_create_error = std::string(fn) + ": " + ex.what();
  return nullptr;
}

}  // namespace

extern "C" {

ceres_hip_bal* ceres_hip_bal_create(const ceres_hip_options* options, int32_t num_cameras, int32_t num_points,
                                    int64_t num_observations, const int32_t* camera_index, const int32_t* point_index,
                                    const double* observations) {
  return bal_create("ceres_hip_bal_create", options, CERES_HIP_CAMERA_ANGLE_AXIS, num_cameras, num_points, num_observations, camera_index,
                    point_index, observations);
}

ceres_hip_bal* ceres_hip_bal_create_with_camera(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                const int32_t* point_index, const double* observations) {
  return bal_create("ceres_hip_bal_create_with_camera", options, camera_model, num_cameras, num_points, num_observations, camera_index,
                    point_index, observations);
}

ceres_hip_bal* ceres_hip_bal_create_with_constant_blocks(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                         int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                         const int32_t* point_index, const double* observations,
                                                         const uint8_t* camera_is_constant, const uint8_t* point_is_constant) {
  return bal_create("ceres_hip_bal_create_with_constant_blocks", options, camera_model, num_cameras, num_points, num_observations, camera_index,
                    point_index, observations, camera_is_constant, point_is_constant);
}

ceres_hip_bal* ceres_hip_bal_create_with_fixed_intrinsics(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                          int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                          const int32_t* point_index, const double* observations,
                                                          const uint8_t* camera_is_constant, const uint8_t* point_is_constant,
                                                          const uint8_t* camera_coordinate_is_constant) {
  // (nothing marked: the handle — and the messages — of ceres_hip_bal_create_with_constant_blocks; an unknown camera model: the mask's
  // length is unknown too, it is not read)
  const bool known = bal_camera_model_known(camera_model);
  bool any = false;
  for (int j = 0; known && camera_coordinate_is_constant && j < (camera_model == CERES_HIP_CAMERA_ANGLE_AXIS ? 9 : 10); ++j)
    any = any || camera_coordinate_is_constant[j] != 0;
  const bool mine = any || (!known && camera_coordinate_is_constant);
  return bal_create(mine ? "ceres_hip_bal_create_with_fixed_intrinsics" : "ceres_hip_bal_create_with_constant_blocks", options, camera_model, num_cameras,
                    num_points, num_observations, camera_index, point_index, observations, camera_is_constant, point_is_constant,
                    any ? camera_coordinate_is_constant : nullptr);
}

ceres_hip_bal* ceres_hip_bal_create_with_shared_intrinsics(const ceres_hip_options* options, int32_t camera_model, int32_t num_cameras,
                                                           int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                                           const int32_t* point_index, const double* observations,
                                                           const uint8_t* camera_is_constant, const int32_t* camera_group, int32_t num_groups) {
  // (no grouping: the handle — and the messages — of ceres_hip_bal_create_with_constant_blocks)
  if (!camera_group)
    return bal_create("ceres_hip_bal_create_with_constant_blocks", options, camera_model, num_cameras, num_points, num_observations, camera_index,
                      point_index, observations, camera_is_constant, nullptr);
  return bal_create("ceres_hip_bal_create_with_shared_intrinsics", options, camera_model, num_cameras, num_points, num_observations, camera_index,
                    point_index, observations, camera_is_constant, nullptr, nullptr, camera_group, num_groups);
}

int ceres_hip_bal_reduced_sizes(const ceres_hip_bal* p, int64_t* num_rows, int64_t* num_rows_e, int64_t* num_rows_removed,
                                int32_t* num_free_cameras, int32_t* num_free_points) {
  if (!p) return CERES_HIP_E_INVALID;
  if (num_rows) *num_rows = p->no;
  if (num_rows_e) *num_rows_e = p->n_rows_e;
  if (num_rows_removed) *num_rows_removed = p->n_removed;
  if (num_free_cameras) *num_free_cameras = p->nfc;
  if (num_free_points) *num_free_points = p->nfp;
  return 0;
}

int ceres_hip_bal_fixed_cost(ceres_hip_bal* p, const double* state, double* fixed_cost) {
  if (!p || !state || !fixed_cost) return CERES_HIP_E_INVALID;
  if (int rc = bal_shared_check(p, "ceres_hip_bal_fixed_cost", state)) return rc;
  ceres_hip_solver* s = p->s;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, up(s, p->d_cand, state, size_t(p->n_a)));
  BAL_TRY(p, bal_fixed_cost_device(p, p->d_cand, fixed_cost));
  return 0;
}

int ceres_hip_bal_sizes(const ceres_hip_bal* p, int64_t* num_parameters, int64_t* num_residuals, int64_t* num_jacobian_values) {
  if (!p) return CERES_HIP_E_INVALID;
  if (num_parameters) *num_parameters = p->n_a;
  if (num_residuals) *num_residuals = 2 * p->no;
  if (num_jacobian_values) *num_jacobian_values = bal_num_values(p);
  return 0;
}

int ceres_hip_bal_num_effective_parameters(const ceres_hip_bal* p, int64_t* num_effective_parameters) {
  if (!p || !num_effective_parameters) return CERES_HIP_E_INVALID;
  *num_effective_parameters = p->n_t;
  return 0;
}

int ceres_hip_bal_get_row_order(const ceres_hip_bal* p, int32_t* row_observation) {
  if (!p || !row_observation) return CERES_HIP_E_INVALID;
  memcpy(row_observation, p->row_obs.data(), sizeof(int32_t) * p->row_obs.size());
  return 0;
}

int ceres_hip_bal_set_loss(ceres_hip_bal* p, int32_t loss_type, double a, double b, double scale) {
  auto invalid = [&](const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_set_loss: " + why;
    return CERES_HIP_E_INVALID;
  };
  if (!p) return invalid("NULL problem handle");
  static_assert(kLossTrivial == CERES_HIP_LOSS_TRIVIAL && kLossHuber == CERES_HIP_LOSS_HUBER && kLossSoftLOne == CERES_HIP_LOSS_SOFTLONE &&
                kLossCauchy == CERES_HIP_LOSS_CAUCHY && kLossArctan == CERES_HIP_LOSS_ARCTAN && kLossTolerant == CERES_HIP_LOSS_TOLERANT &&
                kLossTukey == CERES_HIP_LOSS_TUKEY, "device loss numbers are the ABI's");
  if (loss_type < CERES_HIP_LOSS_TRIVIAL || loss_type > CERES_HIP_LOSS_TUKEY) return invalid("unknown loss_type " + std::to_string(loss_type));
  if (!std::isfinite(scale) || scale <= 0.0) return invalid("scale must be finite and > 0");
  const bool one_param = loss_type != CERES_HIP_LOSS_TRIVIAL && loss_type != CERES_HIP_LOSS_TOLERANT;
  if (one_param && (!std::isfinite(a) || a <= 0.0)) return invalid("a must be finite and > 0");
  if (loss_type == CERES_HIP_LOSS_TOLERANT) {
    if (!std::isfinite(a) || a < 0.0) return invalid("a must be finite and >= 0 for the tolerant loss");
    if (!std::isfinite(b) || b <= 0.0) return invalid("b must be finite and > 0 for the tolerant loss");
  }
  // the constants each loss's constructor derives (include/ceres/loss_function.h:131-330, I/loss_function.cc:134-137)
  LossParams L;
  L.type = loss_type; L.k = scale;
  switch (loss_type) {
    case CERES_HIP_LOSS_HUBER: L.a = a; L.b = a * a; break;
    case CERES_HIP_LOSS_SOFTLONE:
    case CERES_HIP_LOSS_CAUCHY: L.b = a * a; L.c = 1.0 / L.b; break;
    case CERES_HIP_LOSS_ARCTAN: L.a = a; L.b = 1.0 / (a * a); break;
    case CERES_HIP_LOSS_TOLERANT: L.a = a; L.b = b; L.c = b * std::log(1.0 + std::exp(-a / b)); break;
    case CERES_HIP_LOSS_TUKEY: L.b = a * a; break;
    default: break;
  }
  // the trivial loss unscaled IS the squared loss: the kernels' squared-loss instantiations run (a problem that never set a loss)
  if (loss_type == CERES_HIP_LOSS_TRIVIAL && scale == 1.0) L = LossParams{};
  p->loss = L;
  return 0;
}

int ceres_hip_bal_evaluate(ceres_hip_bal* p, const double* state, double* cost, double* residuals, double* gradient,
                           double* jacobian_values) {
  if (!p || !state || !cost) return CERES_HIP_E_INVALID;
  if (int rc = bal_shared_check(p, "ceres_hip_bal_evaluate", state)) return rc;
  ceres_hip_solver* s = p->s;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, up(s, p->d_x, state, size_t(p->n_a)));
  const bool jac = gradient != nullptr || jacobian_values != nullptr;
  BAL_TRY(p, bal_evaluate_device(p, p->d_x, jac, nullptr, p->d_res, cost));
  if (residuals) BAL_TRY(p, down(s, residuals, p->d_res, size_t(2 * p->no)));
  if (jac) {
    bal_set_camera_eval(p, false);
    BAL_TRY(p, load_device(s, p->d_vals, p->d_res, nullptr));
    if (jacobian_values) BAL_TRY(p, down(s, jacobian_values, p->d_vals, size_t(bal_num_values(p))));
    if (gradient) {
      BAL_TRY(p, op_jtb(s, p->d_grad));
      BAL_TRY(p, down(s, gradient, p->d_grad, size_t(p->n_t)));
    }
  }
  return 0;
}

// Timing probe (tools/eval_tiles_probe.py): `iters` back-to-back tile-order evaluations at `state` with some of the kernel's stores
// switched off (BalEvalTilesArgs::debug_flags — the results are then incomplete: nothing else may use this handle afterwards).
int ceres_hip_debug_bal_evaluate_tiles_timing(ceres_hip_bal* p, const double* state, int32_t flags, int32_t iters, double* avg_us) {
  if (!p || !state || !avg_us || iters <= 0) return CERES_HIP_E_INVALID;
  ceres_hip_solver* s = p->s;
  if (p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS) {
    p->err = "ceres_hip_debug_bal_evaluate_tiles_timing: the tile evaluator is angle-axis only";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->intrinsics_mask) {
    p->err = "ceres_hip_debug_bal_evaluate_tiles_timing: the tile evaluator is not supported on handles with fixed intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->n_groups) {
    p->err = "ceres_hip_debug_bal_evaluate_tiles_timing: the tile evaluator is not supported on handles with shared intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!bal_writes_tiles(p)) return fail(s, CERES_HIP_E_UNSUPPORTED, "the evaluator does not write this structure's tiles");
  if (p->has_const && flags != 0) return fail(s, CERES_HIP_E_UNSUPPORTED, "the store experiments are not built for handles with constant cameras");
  BAL_TRY(p, up(s, p->d_x, state, size_t(p->n_a)));
  PartialSet cost;
  hipEvent_t e0, e1;
  HIP_TRY(s, hipEventCreate(&e0));
  HIP_TRY(s, hipEventCreate(&e1));
  int rc = 0;
  for (int w = 0; w < 2 && !rc; ++w)
    if ((rc = bal_evaluate_into_tiles(p, p->d_x, nullptr, &cost, flags)) == 0) rc = bal_parts_collect(p);
  float ms = 0;
  // (the launches alone: every one writes the same partial sums, which nobody takes; no synchronisation in between; the loss ceres_hip_bal_minimize runs)
  BalEvalTilesConstArgs T = bal_tile_args(p, p->d_x, nullptr, p->d_vals, flags);
  if (!rc) rc = bal_parts_room(p, kMaxEvalGrid, &T.e.partials);
  if (!rc) {
    int nparts = 0;
    (void)hipEventRecord(e0, s->stream);
    for (int i = 0; i < iters; ++i) {
      if (p->has_const) (void)LaunchBalEvaluateTilesConst(T, p->np, &nparts, s->stream);
      else (void)LaunchBalEvaluateTiles(T, p->np, p->nc, &nparts, s->stream);
    }
    (void)hipEventRecord(e1, s->stream);
    if (hipStreamSynchronize(s->stream) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = fail(s, CERES_HIP_E_HIP, "timing probe");
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  s->packed = false;
  s->loaded = false;   // (nothing usable is loaded: operators answer "no values loaded" until the next evaluation)
  *avg_us = 1e3 * double(ms) / iters;
  return rc ? bal_fail(p, rc) : 0;
}

int ceres_hip_bal_minimize(ceres_hip_bal* p, const ceres_hip_minimizer_options* o, double* state,
                           ceres_hip_minimizer_summary* S) {
  if (!p || !o || !state || !S) return CERES_HIP_E_INVALID;
  ceres_hip_solver* s = p->s;
  hipStream_t st = s->stream;
  if (int rc = bal_shared_check(p, "ceres_hip_bal_minimize", state)) return rc;
  if (p->n_groups && s->world > 1) {
    p->err = "ceres_hip_bal_minimize: shared intrinsics are not supported on sharded handles";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->n_groups && p->inner_blocks != CERES_HIP_INNER_NONE) {   // (unreachable through ceres_hip_bal_set_inner_iterations)
    p->err = "ceres_hip_bal_minimize: inner iterations are not supported on handles with shared intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->is_constrained) {   // Program::IsFeasible for the constant blocks (I/program.cc:240-289), before any device call
    const std::string why = bal_bounds_constant_infeasible(p, state);
    if (!why.empty()) {
      p->err = "ceres_hip_bal_minimize: " + why;
      return CERES_HIP_E_INVALID;
    }
    if (p->inner_blocks != CERES_HIP_INNER_NONE) {
      p->err = "ceres_hip_bal_minimize: inner iterations are not supported on handles with bounds";
      return CERES_HIP_E_UNSUPPORTED;
    }
  }
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const auto t_start = std::chrono::steady_clock::now();
  memset(S, 0, sizeof(*S));
  if (p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS && s->world > 1) {
    p->err = "ceres_hip_bal_minimize: quaternion cameras are not supported on sharded handles";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->has_const && s->world > 1) {
    p->err = "ceres_hip_bal_minimize: constant parameter blocks are not supported on sharded handles";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->intrinsics_mask && s->world > 1) {
    p->err = "ceres_hip_bal_minimize: fixed intrinsics are not supported on sharded handles";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->intrinsics_mask && p->inner_blocks != CERES_HIP_INNER_NONE) {   // (unreachable through ceres_hip_bal_set_inner_iterations)
    p->err = "ceres_hip_bal_minimize: inner iterations are not supported on handles with fixed intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  const int64_t n = p->n_a;
  BAL_TRY(p, up(s, p->d_x, state, size_t(n)));
  double* x = p->d_x;
  double* cand = p->d_cand;
  if (p->is_constrained) {   // iteration zero: x = Plus(x, 0), the projection onto the box (I/trust_region_minimizer.cc:210-220)
    p->bounds->reset_stats();
    p->bounds->ran_constrained = 1;
    BAL_TRY(p, bal_bounds_project_device(p, x, &p->bounds->num_projected));
  }
  // Constant blocks: the candidate buffer starts as a copy of the state — Plus and the inner passes write free blocks only, so the
  // constant blocks of both buffers stay the caller's doubles through every swap — and the removed rows' cost is taken once, here
  // (TrustRegionMinimizer adds solver_summary_->fixed_cost to every cost it reports: I/trust_region_minimizer.cc:127, 228, 261, 490)
  double fixed_cost = 0.0;
  if (p->has_const) {
    HIP_TRY(s, hipMemcpyAsync(cand, x, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    BAL_TRY(p, bal_fixed_cost_device(p, x, &fixed_cost));
  }
  const double* scale = o->jacobi_scaling ? p->d_scale : nullptr;
  double radius = o->initial_trust_region_radius, decrease_factor = 2.0;
  bool reuse_diagonal = false, one_success = false;
  int invalid_run = 0, iteration = 0;
  double x_cost = 0, grad_max = 0;
  s->have_lm_diag = false;
  // inner iterations (inner_iterations.inc): set or not, this call's statistics start from zero
  const bool inner_set = p->inner_blocks != CERES_HIP_INNER_NONE;
  bool inner_enabled = inner_set;   // (TrustRegionMinimizer::inner_iterations_are_enabled_: the tolerance may switch it off)
  p->inner_steps = 0; p->inner_seconds = 0.0; p->inner_groups_used = 0;
  // the dogleg strategy (dogleg.inc): its radius is `radius`, its other state lives here
  const bool dogleg = p->tr_strategy == CERES_HIP_DOGLEG;
  DoglegState dl;
  if (dogleg) {
    dl.type = p->dogleg_type;
    BAL_TRY(p, dogleg_alloc(p));
  }
  if (inner_set) {
    if (s->world > 1) {
      p->err = "ceres_hip_bal_minimize: inner iterations are not supported on sharded handles";
      return CERES_HIP_E_UNSUPPORTED;
    }
    BAL_TRY(p, bal_inner_plan(p));
    p->inner_groups_used = p->inner->num_groups;
  }

  auto log_iter = [&](const ceres_hip_iteration_summary& it) {
    if (p->is_constrained) bal_bounds_log(p, S->num_iterations_logged);   // (the projected search of the iteration being logged)
    if (S->num_iterations_logged < CERES_HIP_MAX_LOGGED_ITERATIONS) {
      S->iterations[S->num_iterations_logged] = it;
      S->iterations[S->num_iterations_logged++].cost += fixed_cost;   // (0.0 without constant blocks)
    }
  };
  // EvaluateGradientAndJacobian, I/trust_region_minimizer.cc:246-314.  The Jacobian is written
  // already scaled; the gradient of the unscaled problem is recovered from (J S)^T f = S J^T f.
  const bool into_tiles = bal_writes_tiles(p);
  PartialSet x_cost_parts;
  auto eval_values = [&](const double* sc, bool for_column_norms = false) -> int {   // J (scaled by sc) and f at x, loaded into the solver
    // (with the cameras' sums outside LDS the column norms come from the generic kernel, which reads the caller layout: that one
    // evaluation — the first of a run — keeps the two-pass form)
    // (enqueued only: the cost is collected with the gradient's maximum, one host round trip for both)
    if (into_tiles && !(for_column_norms && !s->lds_mode)) return bal_evaluate_into_tiles(p, x, sc, &x_cost_parts);
    TRY(bal_evaluate_enqueue(p, x, true, sc, p->d_res, &x_cost_parts));
    bal_set_camera_eval(p, false);
    return load_device(s, p->d_vals, p->d_res, nullptr);
  };
  auto eval_jacobian = [&]() -> int {
    const auto t0 = std::chrono::steady_clock::now();
    if (o->jacobi_scaling && iteration == 0) {  // scale = 1 / (1 + sqrt(SquaredColumnNorm(J))) of the first Jacobian
      TRY(eval_values(nullptr, true));
      p->parts.drop();   // (the cost of the unscaled evaluation that only feeds the column norms is never read)
      TRY(op_squared_column_norm(s, p->d_grad));
      HIP_TRY(s, LaunchBalJacobiScale(p->d_grad, p->d_scale, p->n_t, st));
    }
    TRY(eval_values(scale));
    TRY(op_jtb(s, p->d_grad));
    PartialSet grad_max_parts;
    TRY(bal_gradient_max(p, scale, x, &grad_max_parts));
    TRY(bal_parts_collect(p));
    grad_max = p->parts.max(grad_max_parts); x_cost = p->parts.sum(x_cost_parts);
    S->evaluation_seconds += seconds_since(t0);
    return 0;
  };
  auto finish = [&](int term, const char* msg) {
    S->termination_type = term;
    snprintf(S->message, sizeof(S->message), "%s", msg);
  };
  BAL_TRY(p, eval_jacobian());
  S->initial_cost = x_cost + fixed_cost;
  S->termination_type = CERES_HIP_NO_CONVERGENCE_T;
  {
    ceres_hip_iteration_summary it0{};
    it0.cost = x_cost; it0.gradient_max_norm = grad_max; it0.trust_region_radius = radius;
    it0.step_is_valid = 1; it0.step_is_successful = 1;
    log_iter(it0);
  }
  while (true) {
    // FinalizeIterationAndCheckIfMinimizerCanContinue, :320-362
    if (iteration >= o->max_num_iterations) { finish(CERES_HIP_NO_CONVERGENCE_T, "Maximum number of iterations reached."); break; }
    if (grad_max <= o->gradient_tolerance) { finish(CERES_HIP_CONVERGENCE, "Gradient tolerance reached."); break; }
    if (radius <= o->min_trust_region_radius) { finish(CERES_HIP_CONVERGENCE, "Minimum trust region radius reached."); break; }
    ++iteration;
    ceres_hip_iteration_summary it{};
    ceres_hip_lm_result lr{};
    const auto t0 = std::chrono::steady_clock::now();
    if (dogleg) {   // DoglegStrategy::ComputeStep + the model cost change (dogleg.inc)
      int solves = 0;
      dl.radius = radius;
      BAL_TRY(p, dogleg_step(p, dl, o, reuse_diagonal, p->d_step, &lr, &solves));
      S->linear_solver_seconds += seconds_since(t0);
      S->num_linear_solves += solves;
    } else {   // LevenbergMarquardtStrategy::ComputeStep + the model cost change, on the device (f1)
      ceres_hip_lm_options lo{};
      lo.radius = radius; lo.min_diagonal = o->min_lm_diagonal; lo.max_diagonal = o->max_lm_diagonal; lo.eta = o->eta;
      lo.reuse_diagonal = reuse_diagonal ? 1 : 0;
      BAL_TRY(p, lm_step_loaded(s, &lo, p->d_step, &lr));
      HIP_TRY(s, hipStreamSynchronize(st));
      S->linear_solver_seconds += seconds_since(t0);
      ++S->num_linear_solves;
      reuse_diagonal = true;
    }
    it.linear_solver_iterations = lr.linear_solver.num_iterations;
    it.linear_solver_termination = lr.linear_solver.termination_type;
    if (lr.linear_solver.termination_type == CERES_HIP_FATAL_ERROR) {
      finish(CERES_HIP_MINIMIZER_FAILURE, "Linear solver failed due to unrecoverable non-numeric causes.");
      break;
    }
    // ComputeTrustRegionStep, :381-461
    const bool valid = lr.linear_solver.termination_type != CERES_HIP_FAILURE && lr.step_is_finite &&
                       lr.model_cost_change > 0.0;
    it.step_is_valid = valid;
    if (!valid) {  // HandleInvalidStep :466-497
      if (++invalid_run >= o->max_consecutive_invalid_steps) {
        finish(CERES_HIP_MINIMIZER_FAILURE, "Too many consecutive invalid steps.");
        break;
      }
      if (dogleg) { dl.mu *= kDoglegMuIncrease; dl.reuse = false; }   // StepIsInvalid: the radius stays
      else { radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true; }
      it.cost = x_cost; it.gradient_max_norm = grad_max; it.trust_region_radius = radius;
      ++S->num_unsuccessful_steps;
      log_iter(it);
      continue;
    }
    invalid_run = 0;
    // delta = step .* scale; candidate = Plus(x, delta); |x|, |delta|; the candidate's cost — two kernels, ONE host round trip
    // (inner iterations set: |x - candidate| too, a third kernel in the same round trip — Ceres' step norm, whether or not an inner
    // pass follows: ParameterToleranceReached, I/trust_region_minimizer.cc:726-748)
    double xn = 0, dn = 0, cand_cost = 0;
    PartialSet xn_parts, dn_parts, diff_parts, cost_parts;
    auto diff_norm = [&](PartialSet* out) -> int {   // |x - candidate|^2, enqueued
      int nd = 0; double* parts = nullptr;
      TRY(bal_parts_room(p, kMaxVecGrid, &parts));
      HIP_TRY(s, LaunchBalDiffNorm(x, cand, n, parts, &nd, st));
      *out = p->parts.take(nd);
      return 0;
    };
    {
      // DoLineSearch (I/trust_region_minimizer.cc:103-108): the projected Armijo search scales delta; the candidate below is
      // clamp(x + a delta), its cost the loop's own evaluator's
      if (p->is_constrained) BAL_TRY(p, bal_bounds_line_search(p, x, scale, cand, x_cost));
      const auto te = std::chrono::steady_clock::now();
      BAL_TRY(p, bal_candidate(p, x, scale, cand, &xn_parts, &dn_parts));
      if (inner_set) BAL_TRY(p, diff_norm(&diff_parts));
      BAL_TRY(p, bal_evaluate_enqueue(p, cand, false, nullptr, nullptr, &cost_parts));
      BAL_TRY(p, bal_parts_collect(p));
      xn = p->parts.sum(xn_parts); dn = p->parts.sum(inner_set ? diff_parts : dn_parts);
      cand_cost = p->parts.sum(cost_parts);
      S->evaluation_seconds += seconds_since(te);
    }
    // DoInnerIterationsIfNeeded, I/trust_region_minimizer.cc:509-587: one coordinate-descent pass from the candidate, which always
    // replaces it; its cost change boosts the model cost change
    double model_cost_change = lr.model_cost_change;
    bool inner_useful = false;
    if (inner_enabled && std::isfinite(cand_cost)) {
      const auto ti = std::chrono::steady_clock::now();
      ++p->inner_steps;
      double inner_cost = 0;
      BAL_TRY(p, bal_inner_pass(p, cand));
      BAL_TRY(p, diff_norm(&diff_parts));
      BAL_TRY(p, bal_evaluate_enqueue(p, cand, false, nullptr, nullptr, &cost_parts));
      BAL_TRY(p, bal_parts_collect(p));
      inner_cost = p->parts.sum(cost_parts);
      if (std::isfinite(inner_cost)) {
        dn = p->parts.sum(diff_parts);
        model_cost_change += cand_cost - inner_cost;
        inner_useful = inner_cost < std::min(x_cost, cand_cost);
        inner_enabled = 1.0 - inner_cost / cand_cost > p->inner_tolerance;
        cand_cost = inner_cost;
      } else {   // (the evaluation failed: Ceres keeps the candidate as it was — rebuilt here from x and the step)
        BAL_TRY(p, bal_candidate(p, x, scale, cand, &xn_parts, &dn_parts));
        p->parts.drop();   // (its sums were read above)
      }
      p->inner_seconds += seconds_since(ti);
    }
    it.step_norm = std::sqrt(dn);
    if (one_success && it.step_norm <= o->parameter_tolerance * (std::sqrt(xn) + o->parameter_tolerance)) {
      finish(CERES_HIP_CONVERGENCE, "Parameter tolerance reached.");
      it.cost = x_cost; it.trust_region_radius = radius;
      log_iter(it);
      break;
    }
    it.cost_change = x_cost - cand_cost;
    if (std::fabs(it.cost_change) <= o->function_tolerance * x_cost) {
      finish(CERES_HIP_CONVERGENCE, "Function tolerance reached.");
      it.cost = x_cost; it.trust_region_radius = radius;
      log_iter(it);
      break;
    }
    it.relative_decrease = (x_cost - cand_cost) / model_cost_change;  // TrustRegionStepEvaluator, monotonic
    if (inner_useful || it.relative_decrease > o->min_relative_decrease) {  // IsStepSuccessful :801-825; HandleSuccessfulStep :829-845
      std::swap(x, cand);
      one_success = true;
      BAL_TRY(p, eval_jacobian());
      if (dogleg) {   // StepAccepted(relative_decrease): no clamp to max_trust_region_radius
        if (it.relative_decrease < 0.25) radius *= 0.5;
        if (it.relative_decrease > 0.75) radius = std::max(radius, 3.0 * dl.step_norm);
        dl.mu = std::max(kDoglegMinMu, 2.0 * dl.mu / kDoglegMuIncrease);
        dl.reuse = false;
      } else {
        radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * it.relative_decrease - 1.0, 3));
        radius = std::min(o->max_trust_region_radius, radius);
      }
      decrease_factor = 2.0;
      reuse_diagonal = false;
      it.step_is_successful = 1;
      ++S->num_successful_steps;
    } else {
      if (dogleg) { radius *= 0.5; dl.reuse = true; }   // StepRejected
      else { radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true; }
      ++S->num_unsuccessful_steps;
    }
    it.cost = it.step_is_successful ? x_cost : cand_cost;
    it.gradient_max_norm = grad_max;
    it.trust_region_radius = radius;
    log_iter(it);
  }
  S->final_cost = x_cost + fixed_cost;
  BAL_TRY(p, down(s, state, x, size_t(n)));
  S->total_seconds = seconds_since(t_start);
  return 0;
}

}  // extern "C"
