// covariance.inc — ceres_hip_bal_covariance (ceres::Covariance for bundle adjustment in the Schur form: design/17_covariance.md,
// kernels_covariance.hip).  Textually included by bal_frontend.inc.  The stages, each timed by the host's clock around a stream
// synchronisation:
//   evaluate    the caller-layout Jacobian at `state` (bal_evaluate_device, the loss switched off for the call if asked)
//   eliminate   C_p by the generic block-diagonal kernel, its scaled factorisation and inverse (the point stage can fail here), the
//               block-sparse S by the DENSE_SCHUR eliminator with NO diagonal, expanded into the solver's dense n x n buffer
//   factor      S~ = Lambda S Lambda, LaunchDenseCholesky, the smallest squared diagonal entry of L (the Schur stage can fail here)
//   inverse     Lambda (L L^T)^-1 Lambda into the second n x n buffer
//   blocks      one wavefront per requested pair, then one copy to the host
// A handle with shared intrinsics (n_groups != 0; design/28_shared_covariance.md) runs the same stages over its own structure — the
// eliminator forms S over poses and groups — with lists, pair codes and a blocks pass of its own (kernels_covariance_shared.hip); every
// branch for it tests n_groups first.
// Nothing of the solver's own state is used but its structure, its stream, the dense buffer and the eliminator's scratch, all of
// which every DENSE_SCHUR solve rebuilds; the factorisation flag is this feature's own.

struct BalCovariance {
  double *d_cinv = nullptr, *d_ppiv = nullptr, *d_lam = nullptr, *d_W = nullptr, *d_min = nullptr;
  int* d_flag = nullptr;
  int32_t *d_pt_ptr = nullptr, *d_ent_epos = nullptr, *d_ent_fpos = nullptr, *d_ent_ccol = nullptr;
  int32_t *d_ent_gpos = nullptr, *d_ent_gcol = nullptr;   // shared intrinsics: the group cell of every entry (fpos / ccol: its pose cell, -1: none)
  // per call, grown on demand: the pairs' codes and offsets, the output
  int32_t *d_code_a = nullptr, *d_code_b = nullptr;
  int64_t* d_off = nullptr;
  double* d_out = nullptr;
  int64_t pair_capacity = 0, out_capacity = 0;
  int64_t fixed_bytes = 0;   // everything but the per-call buffers
};

namespace {

int64_t cov_device_bytes(const BalCovariance* c) {
  return c->fixed_bytes + c->pair_capacity * int64_t(2 * sizeof(int32_t) + sizeof(int64_t)) + c->out_capacity * int64_t(sizeof(double));
}

// The lists of the blocks pass and the buffers every call uses: built on the first call.
int bal_cov_prepare(ceres_hip_bal* p) {
  if (p->cov) return 0;
  ceres_hip_solver* s = p->s;
  const int64_t no = p->no;
  BalHostRows H;
  TRY(bal_fetch_rows(p, kRowCam | kRowPt | kRowFpos, H));
  // per free point its rows with a free camera, in row order (the rows of a point are consecutive and carry their E cell at 6 r).
  // Shared intrinsics: EVERY row of a point (a row of a constant pose still carries its group cell); per entry the E cell, the pose cell
  // and its first column in S^-1 (-1, -1: the pose is constant), the group cell — behind the pose cell — and its first column
  const bool shared = p->n_groups != 0;
  std::vector<int32_t> gpos, gcol;
  const BalGrouping by_pt = bal_group_by(no, p->nfp, [&](int64_t r) { return shared || bal_camera_column(p, H.cam[r]) >= 0 ? bal_point_column(p, H.pt[r]) : -1; });
  std::vector<int32_t> epos, fpos = bal_gather(by_pt.perm, H.fpos.data()), ccol;
  epos.reserve(fpos.size()); ccol.reserve(fpos.size());
  for (int32_t r : by_pt.perm) {
    if (r >= p->n_rows_e) return fail(s, CERES_HIP_E_INVALID, "covariance: a row with a free point behind the rows with an E cell");
    epos.push_back(int32_t(6 * int64_t(r)));
    if (!p->n_groups) { ccol.push_back(bal_camera_column(p, H.cam[r])); continue; }
    const int cc = bal_camera_column(p, H.cam[r]);
    ccol.push_back(cc >= 0 ? 6 * cc : -1);
    gcol.push_back(6 * p->nfc + 3 * p->group_of[H.cam[r]]);
  }
  if (p->n_groups) {   // (bal_layout: a row's pose cell and group cell back to back behind the E cells, in row order)
    std::vector<int32_t> row_gpos(size_t(no), 0);
    int64_t next = 6 * p->n_rows_e;
    for (int64_t r = 0; r < no; ++r) {
      if (H.fpos[r] >= 0) {
        if (H.fpos[r] != next) return fail(s, CERES_HIP_E_INVALID, "covariance: a pose cell is not where the layout of shared intrinsics puts it");
        next += 12;
      }
      row_gpos[r] = int32_t(next); next += 6;
    }
    if (next != bal_num_values(p)) return fail(s, CERES_HIP_E_INVALID, "covariance: the cells of the rows do not add up to the handle's values");
    gpos = bal_gather(by_pt.perm, row_gpos.data());
  }
  std::unique_ptr<BalCovariance> c(new BalCovariance);
  const int64_t before = s->device_bytes;
  const size_t n = size_t(s->hs.num_cols_f);
  TRY(dev_upload(s, &c->d_pt_ptr, by_pt.ptr)); TRY(dev_upload(s, &c->d_ent_epos, epos)); TRY(dev_upload(s, &c->d_ent_fpos, fpos)); TRY(dev_upload(s, &c->d_ent_ccol, ccol));
  if (p->n_groups) { TRY(dev_upload(s, &c->d_ent_gpos, gpos)); TRY(dev_upload(s, &c->d_ent_gcol, gcol)); }
  TRY(dev_alloc(s, &c->d_cinv, size_t(9) * p->nfp)); TRY(dev_alloc(s, &c->d_ppiv, size_t(p->nfp)));
  TRY(dev_alloc(s, &c->d_lam, n)); TRY(dev_alloc(s, &c->d_min, 4)); TRY(dev_alloc(s, &c->d_flag, 1));
  TRY(dev_alloc(s, &c->d_W, n * n));
  HIP_TRY(s, hipStreamSynchronize(s->stream));   // (the uploads read host vectors that go out of scope here)
  c->fixed_bytes = s->device_bytes - before;
  p->cov = c.release();
  return 0;
}

int bal_cov_reserve(ceres_hip_bal* p, int64_t pairs, int64_t out) {
  ceres_hip_solver* s = p->s;
  BalCovariance* c = p->cov;
  if (pairs > c->pair_capacity) {
    dev_release(s, c->d_code_a, c->pair_capacity * int64_t(sizeof(int32_t))); dev_release(s, c->d_code_b, c->pair_capacity * int64_t(sizeof(int32_t)));
    dev_release(s, c->d_off, c->pair_capacity * int64_t(sizeof(int64_t)));
    c->d_code_a = c->d_code_b = nullptr; c->d_off = nullptr; c->pair_capacity = 0;
    TRY(dev_alloc(s, &c->d_code_a, size_t(pairs))); TRY(dev_alloc(s, &c->d_code_b, size_t(pairs))); TRY(dev_alloc(s, &c->d_off, size_t(pairs)));
    c->pair_capacity = pairs;
  }
  if (out > c->out_capacity) {
    dev_release(s, c->d_out, c->out_capacity * int64_t(sizeof(double)));
    c->d_out = nullptr; c->out_capacity = 0;
    TRY(dev_alloc(s, &c->d_out, size_t(out)));
    c->out_capacity = out;
  }
  return 0;
}

// min over a device vector (LaunchCovMin) and where: one small copy, one synchronisation
int cov_min(ceres_hip_bal* p, const double* v, int64_t count, int64_t stride, int square, double* value, int64_t* at) {
  ceres_hip_solver* s = p->s;
  double h[2] = {0.0, -1.0};
  HIP_TRY(s, LaunchCovMin(v, count, stride, square, p->cov->d_min, s->stream));
  HIP_TRY(s, hipMemcpyAsync(h, p->cov->d_min, sizeof(h), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  *value = h[0]; *at = int64_t(h[1]);
  return 0;
}

int bal_covariance_impl(ceres_hip_bal* p, const ceres_hip_covariance_options& o, const double* state, int64_t num_pairs, const int32_t* block_a,
                        const int32_t* block_b, double* blocks_out, ceres_hip_covariance_summary* S) {
  ceres_hip_solver* s = p->s;
  hipStream_t st = s->stream;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  TRY(bal_cov_prepare(p));
  BalCovariance* c = p->cov;
  const int n = int(s->hs.num_cols_f);
  // the pairs: codes and offsets (host), the output's length
  const size_t npairs = size_t(num_pairs);
  std::vector<int32_t> code_a(npairs), code_b(npairs);
  std::vector<int64_t> off(npairs);
  int64_t total = 0;
  auto code = [&](int32_t blk, int* dim) {
    if (p->n_groups) {   // shared intrinsics: point | pose (6, constant: zeros) | group (3, never constant); the index is the first column in S^-1
      *dim = blk >= p->np && blk < p->np + p->nc ? 6 : 3;
      if (blk < p->np) return 4 * blk + int(kCovSharedPoint);
      if (blk >= p->np + p->nc) return 4 * (6 * p->nfc + 3 * (blk - p->np - p->nc)) + int(kCovSharedGroup);
      const int q = bal_camera_column(p, blk - p->np);
      return q >= 0 ? 4 * (6 * q) + int(kCovSharedPose) : int(kCovSharedConstPose);
    }
    if (blk < p->np) {
      const int q = bal_point_column(p, blk);
      *dim = 3;
      return q >= 0 ? 4 * q + int(kCovPoint) : int(kCovConstPoint);
    }
    const int q = bal_camera_column(p, blk - p->np);
    *dim = p->cw;
    return q >= 0 ? 4 * q + int(kCovCamera) : int(kCovConstCamera);
  };
  for (int64_t i = 0; i < num_pairs; ++i) {
    int da = 0, db = 0;
    code_a[i] = code(block_a[i], &da); code_b[i] = code(block_b[i], &db);
    off[i] = total;
    total += int64_t(da) * db;
  }
  TRY(bal_cov_reserve(p, std::max<int64_t>(num_pairs, 1), std::max<int64_t>(total, 1)));
  S->device_bytes = cov_device_bytes(c);
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](double* seconds) -> int {
    HIP_TRY(s, hipStreamSynchronize(st));
    *seconds = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    return 0;
  };
  // ---- evaluate
  TRY(up(s, p->d_x, state, size_t(p->n_a)));
  {
    const LossParams kept = p->loss;
    if (!o.apply_loss_function) p->loss = LossParams{};
    double cost = 0.0;
    const int rc = bal_evaluate_device(p, p->d_x, true, nullptr, p->d_res, &cost);
    p->loss = kept;
    TRY(rc);
  }
  bal_set_camera_eval(p, false);
  TRY(load_device(s, p->d_vals, p->d_res, nullptr));   // (no LM diagonal: D == nullptr)
  TRY(lap(&S->evaluate_seconds));
  // ---- eliminate
  HIP_TRY(s, LaunchGenBlockDiagonal(s->G, s->values, kE, nullptr, c->d_cinv, s->hs.diag_off_e.back(), st));
  HIP_TRY(s, LaunchCovPointFactor(p->nfp, c->d_cinv, c->d_ppiv, st));
  int64_t at = -1;
  TRY(cov_min(p, c->d_ppiv, p->nfp, 1, 0, &S->min_point_pivot, &at));
  S->min_schur_pivot = -1.0;
  if (!(S->min_point_pivot > o.min_scaled_pivot)) {
    TRY(lap(&S->eliminate_seconds));
    S->termination_type = CERES_HIP_FAILURE;
    snprintf(S->message, sizeof(S->message),
             "The point factorization failed: free point %lld has the scaled pivot %.3e (0: a diagonal entry or a pivot of E^T E is not positive), not above "
             "min_scaled_pivot = %.3e. The Jacobian is rank deficient.", (long long)at, S->min_point_pivot, o.min_scaled_pivot);
    return 0;
  }
  HIP_TRY(s, LaunchSchurSparseEliminate(s->G, s->schur_pairs, s->values, c->d_cinv, nullptr, s->d_Sblk, st));
  HIP_TRY(s, hipMemsetAsync(s->d_S, 0, sizeof(double) * size_t(n) * size_t(n), st));
  HIP_TRY(s, LaunchSchurBlocksToDense(s->G, s->schur_pairs, s->d_Sblk, s->schur_storage.num_values(), s->d_S, st));
  TRY(lap(&S->eliminate_seconds));
  // ---- scale, factor
  int flags[1] = {0};
  HIP_TRY(s, hipMemsetAsync(c->d_flag, 0, sizeof(int), st));
  HIP_TRY(s, LaunchCovScale(s->d_S, n, c->d_lam, c->d_flag, st));
  HIP_TRY(s, hipMemcpyAsync(flags, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  if (flags[0]) {
    TRY(lap(&S->factor_seconds));
    S->termination_type = CERES_HIP_FAILURE;
    S->min_schur_pivot = 0.0;
    snprintf(S->message, sizeof(S->message),
             "The Schur complement factorization failed: a diagonal entry of S is not positive. The Jacobian is rank deficient.");
    return 0;
  }
  HIP_TRY(s, LaunchDenseCholesky(s->d_S, n, c->d_flag, st));
  HIP_TRY(s, hipMemcpyAsync(flags, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  TRY(cov_min(p, s->d_S, n, int64_t(n) + 1, 1, &S->min_schur_pivot, &at));
  if (flags[0]) S->min_schur_pivot = 0.0;   // (the factorisation went on with a 1 in the pivot's place: 0 stands for "not positive")
  TRY(lap(&S->factor_seconds));
  if (!(S->min_schur_pivot > o.min_scaled_pivot)) {
    S->termination_type = CERES_HIP_FAILURE;
    if (flags[0])
      snprintf(S->message, sizeof(S->message),
               "The Schur complement factorization failed: a pivot of the unit-diagonal-scaled S is not positive (reported as 0), not above "
               "min_scaled_pivot = %.3e. The Jacobian is rank deficient.", o.min_scaled_pivot);
    else
      snprintf(S->message, sizeof(S->message),
               "The Schur complement factorization failed: column %lld of the unit-diagonal-scaled S has the pivot %.3e, not above min_scaled_pivot = %.3e. "
               "The Jacobian is rank deficient.", (long long)at, S->min_schur_pivot, o.min_scaled_pivot);
    return 0;
  }
  // ---- inverse from the factor
  HIP_TRY(s, LaunchCovInverseFromFactor(s->d_S, n, c->d_lam, c->d_W, st));
  TRY(lap(&S->inverse_seconds));
  // ---- blocks
  if (num_pairs > 0) {
    HIP_TRY(s, hipMemcpyAsync(c->d_code_a, code_a.data(), sizeof(int32_t) * size_t(num_pairs), hipMemcpyHostToDevice, st));
    HIP_TRY(s, hipMemcpyAsync(c->d_code_b, code_b.data(), sizeof(int32_t) * size_t(num_pairs), hipMemcpyHostToDevice, st));
    HIP_TRY(s, hipMemcpyAsync(c->d_off, off.data(), sizeof(int64_t) * size_t(num_pairs), hipMemcpyHostToDevice, st));
    if (p->n_groups) {
      CovSharedBlocksArgs A;
      A.n_pairs = int(num_pairs); A.n = n;
      A.code_a = c->d_code_a; A.code_b = c->d_code_b; A.out_off = c->d_off; A.out = c->d_out;
      A.values = p->d_vals; A.cinv = c->d_cinv; A.sinv = c->d_W;
      A.pt_ptr = c->d_pt_ptr; A.ent_epos = c->d_ent_epos; A.ent_ppos = c->d_ent_fpos; A.ent_pcol = c->d_ent_ccol;
      A.ent_gpos = c->d_ent_gpos; A.ent_gcol = c->d_ent_gcol;
      HIP_TRY(s, LaunchCovSharedBlocks(A, st));
    } else {
      CovBlocksArgs A;
      A.n_pairs = int(num_pairs); A.n = n;
      A.code_a = c->d_code_a; A.code_b = c->d_code_b; A.out_off = c->d_off; A.out = c->d_out;
      A.values = p->d_vals; A.cinv = c->d_cinv; A.sinv = c->d_W;
      A.pt_ptr = c->d_pt_ptr; A.ent_epos = c->d_ent_epos; A.ent_fpos = c->d_ent_fpos; A.ent_ccol = c->d_ent_ccol;
      HIP_TRY(s, LaunchCovBlocks(A, p->cw, st));
    }
    HIP_TRY(s, hipStreamSynchronize(st));   // (a failure of the pass must not leave half a result with the caller)
    TRY(down(s, blocks_out, c->d_out, size_t(total)));
  }
  TRY(lap(&S->blocks_seconds));
  S->termination_type = CERES_HIP_SUCCESS;
  snprintf(S->message, sizeof(S->message), "Success.");
  return 0;
}

}  // namespace

void bal_cov_free(ceres_hip_bal* p) {
  delete p->cov;   // (the device buffers go with the solver's other allocations)
  p->cov = nullptr;
}

extern "C" {

void ceres_hip_covariance_default_options(ceres_hip_covariance_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->apply_loss_function = 1;   // Covariance::Options, include/ceres/covariance.h
  o->min_scaled_pivot = 1e-8;   // design/17_covariance.md: the logarithmic middle between a free gauge's pivots and a fixed one's
}

int ceres_hip_bal_covariance(ceres_hip_bal* p, const ceres_hip_covariance_options* options, const double* state, int64_t num_pairs,
                             const int32_t* block_a, const int32_t* block_b, double* blocks_out, ceres_hip_covariance_summary* summary) try {
  auto refuse = [&](int code, const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_covariance: " + why;
    return code;
  };
  if (!p) return refuse(CERES_HIP_E_INVALID, "NULL problem handle");
  if (!state) return refuse(CERES_HIP_E_INVALID, "NULL state");
  if (!summary) return refuse(CERES_HIP_E_INVALID, "NULL summary");
  if (num_pairs < 0) return refuse(CERES_HIP_E_INVALID, "num_pairs < 0");
  if (num_pairs > 0 && (!block_a || !block_b || !blocks_out)) return refuse(CERES_HIP_E_INVALID, "NULL pair array or output");
  if (num_pairs > int64_t(INT32_MAX) - 4) return refuse(CERES_HIP_E_INVALID, "more than 2^31 pairs");
  ceres_hip_covariance_options o;
  ceres_hip_covariance_default_options(&o);
  if (options) o = *options;
  if (!std::isfinite(o.min_scaled_pivot) || o.min_scaled_pivot < 0.0) return refuse(CERES_HIP_E_INVALID, "min_scaled_pivot must be finite and >= 0");
  ceres_hip_solver* s = p->s;
  if (p->intrinsics_mask) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with fixed intrinsics");
  if (!is_dense_schur(s)) return refuse(CERES_HIP_E_UNSUPPORTED, "the handle's linear solver is not CERES_HIP_DENSE_SCHUR");
  if (s->world > 1) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on sharded handles");
  const int64_t num_blocks = int64_t(p->np) + p->nc + p->n_groups;   // (shared intrinsics: the groups behind the cameras' poses)
  for (int64_t i = 0; i < num_pairs; ++i) {
    if (block_a[i] < 0 || block_a[i] >= num_blocks || block_b[i] < 0 || block_b[i] >= num_blocks)
      return refuse(CERES_HIP_E_INVALID, "pair " + std::to_string(i) + ": block index out of range [0, " + std::to_string(num_blocks) + ")");
  }
  if (int rc = bal_shared_check(p, "ceres_hip_bal_covariance", state)) return rc;
  memset(summary, 0, sizeof(*summary));
  summary->termination_type = CERES_HIP_FAILURE;
  BAL_TRY(p, bal_covariance_impl(p, o, state, num_pairs, block_a, block_b, blocks_out, summary));
  return 0;
} catch (const std::exception& ex) {
  (p ? p->err : g_create_error) = std::string("ceres_hip_bal_covariance: ") + ex.what();
  return CERES_HIP_E_INVALID;
}

}  // extern "C"
