// solver_ops.inc — part of solver.hip (included there, after the solver struct and the operators): the operator-level entry points of the C ABI (ceres_hip_op_*, ceres_hip_get_*): host vectors in, host vectors out, for parity tests

// ---- operator-level entry points: host vectors in, host vectors out ----------
namespace {
int up(ceres_hip_solver* s, double* dev, const double* host, size_t n) {
  if (n) HIP_TRY(s, hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return 0;
}
int down(ceres_hip_solver* s, double* host, const double* dev, size_t n) {
  if (n) HIP_TRY(s, hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return 0;
}
}  // namespace

int ceres_hip_op_right_multiply(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  TRY(require_caller_values(s, "ceres_hip_op_right_multiply"));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const HostStructure& h = s->hs;
  double *dx = s->scratch_vec, *dy = s->scratch_vec + h.num_cols;
  TRY(up(s, dx, x, h.num_cols));
  TRY(up(s, dy, y, h.num_rows));
  HIP_TRY(s, LaunchGenRightMultiply(s->G, s->values, kAll, dx, dy, nullptr, s->stream));
  return down(s, y, dy, h.num_rows);
}

int ceres_hip_op_left_multiply(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  TRY(require_caller_values(s, "ceres_hip_op_left_multiply"));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const HostStructure& h = s->hs;
  double *dy = s->scratch_vec, *dx = s->scratch_vec + h.num_cols;
  TRY(up(s, dx, x, h.num_rows));
  TRY(up(s, dy, y, h.num_cols));
  HIP_TRY(s, LaunchGenLeftMultiply(s->G, s->values, kAll, dx, dy, nullptr, s->stream));
  return down(s, y, dy, h.num_cols);
}

// ---- PartitionedMatrixView products (I/partitioned_matrix_view_impl.h:112-375) -----------------
// E = the first cell of each of the first num_row_blocks_e rows, F = everything else; vectors are
// indexed in the part's own column space (F: col_block_pos - num_cols_e), rows in the full row space.
namespace {
int pmv_product(ceres_hip_solver* s, int part, bool left, const double* x, double* y) {
  TRY(require_loaded(s));
  TRY(require_caller_values(s, "a PartitionedMatrixView product"));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const HostStructure& h = s->hs;
  const size_t ncols = size_t(part == kE ? h.num_cols_e : h.num_cols_f);
  const size_t nin = left ? size_t(h.num_rows) : ncols, nout = left ? ncols : size_t(h.num_rows);
  // scratch_vec holds num_cols + num_rows doubles: column-space vector first, row-space vector behind it
  double* dcol = s->scratch_vec;
  double* drow = s->scratch_vec + h.num_cols;
  double* dx = left ? drow : dcol;
  double* dy = left ? dcol : drow;
  TRY(up(s, dx, x, nin));
  TRY(up(s, dy, y, nout));
  if (left) HIP_TRY(s, LaunchGenLeftMultiply(s->G, s->values, part, dx, dy, nullptr, s->stream));
  else HIP_TRY(s, LaunchGenRightMultiply(s->G, s->values, part, dx, dy, nullptr, s->stream));
  return down(s, y, dy, nout);
}
int pmv_block_diagonal(ceres_hip_solver* s, int part, double* blocks, int64_t capacity) {
  TRY(require_loaded(s));
  TRY(require_caller_values(s, "a PartitionedMatrixView product"));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const HostStructure& h = s->hs;
  const int64_t len = part == kE ? h.diag_off_e.back() : h.diag_off_f.back();
  if (capacity < len) return fail(s, CERES_HIP_E_INVALID, "capacity %lld < %lld", (long long)capacity, (long long)len);
  double* tmp = nullptr;
  HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(double) * std::max<int64_t>(1, len)));
  hipError_t e = debug_poison(s, tmp, size_t(len));
  if (e == hipSuccess) e = LaunchGenBlockDiagonal(s->G, s->values, part, nullptr, tmp, len, s->stream);
  int rc = e == hipSuccess ? down(s, blocks, tmp, size_t(len)) : fail(s, CERES_HIP_E_HIP, "block diagonal kernel failed");
  (void)hipFree(tmp);
  return rc;
}
}  // namespace

int ceres_hip_op_right_multiply_e(ceres_hip_solver* s, const double* x, double* y) { return pmv_product(s, kE, false, x, y); }
int ceres_hip_op_right_multiply_f(ceres_hip_solver* s, const double* x, double* y) { return pmv_product(s, kF, false, x, y); }
int ceres_hip_op_left_multiply_e(ceres_hip_solver* s, const double* x, double* y) { return pmv_product(s, kE, true, x, y); }
int ceres_hip_op_left_multiply_f(ceres_hip_solver* s, const double* x, double* y) { return pmv_product(s, kF, true, x, y); }
int ceres_hip_op_block_diagonal_ete(ceres_hip_solver* s, double* blocks, int64_t capacity) { return pmv_block_diagonal(s, kE, blocks, capacity); }
int ceres_hip_op_block_diagonal_ftf(ceres_hip_solver* s, double* blocks, int64_t capacity) { return pmv_block_diagonal(s, kF, blocks, capacity); }

int ceres_hip_op_squared_column_norm(ceres_hip_solver* s, double* x) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  TRY(op_squared_column_norm(s, s->scratch_vec));
  return down(s, x, s->scratch_vec, s->hs.num_cols);
}

int ceres_hip_op_jtjx(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "jtjx is the CGNR operator; this instance is ITERATIVE_SCHUR");
  TRY(up(s, s->cg.p, x, s->hs.num_cols));
  TRY(op_jtjx(s, s->cg.p, s->cg.z, nullptr));
  return down(s, y, s->cg.z, s->hs.num_cols);
}

int ceres_hip_op_jtb(ceres_hip_solver* s, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  TRY(op_jtb(s, s->scratch_vec));
  return down(s, y, s->scratch_vec, s->hs.num_cols);
}

// the dogleg strategy's one pass over J (kernels_dogleg.hip), on host vectors
int ceres_hip_op_jacobian_gram(ceres_hip_solver* s, const double* a, const double* b, double* out) {
  if (!s) return CERES_HIP_E_INVALID;
  if (!a || !b || !out) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_op_jacobian_gram: NULL argument");
  TRY(require_loaded(s));
  TRY(require_caller_values(s, "ceres_hip_op_jacobian_gram"));
  if (s->world > 1) return fail(s, CERES_HIP_E_UNSUPPORTED, "ceres_hip_op_jacobian_gram: sharded instances hold a share of the rows");
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const size_t nc = size_t(s->hs.num_cols);
  double* tmp = nullptr;
  HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(double) * (2 * nc + 5 * kDoglegGrid)));
  int np = 0;
  hipError_t e = debug_poison(s, tmp, 2 * nc + 5 * kDoglegGrid);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp, a, sizeof(double) * nc, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(tmp + nc, b, sizeof(double) * nc, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = LaunchJacobianGram(s->G, s->values, tmp, tmp + nc, s->have_b ? s->b : nullptr, tmp + 2 * nc, &np, s->stream);
  std::vector<double> h(size_t(5) * kDoglegGrid);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), tmp + 2 * nc, sizeof(double) * 5 * np, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(s, CERES_HIP_E_HIP, "ceres_hip_op_jacobian_gram: %s", hipGetErrorString(e));
  for (int k = 0; k < 5; ++k) {
    double t = 0;
    for (int q = 0; q < np; ++q) t += h[size_t(5) * q + k];   // fixed order: deterministic
    out[k] = t;
  }
  return 0;
}

int ceres_hip_op_schur_init(ceres_hip_solver* s) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, true));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return 0;
}

int ceres_hip_get_schur_rhs(ceres_hip_solver* s, double* rhs) {
  TRY(require_loaded(s));
  return down(s, rhs, s->rhs_f, s->hs.num_cols_f);
}

int ceres_hip_get_ete_inverse(ceres_hip_solver* s, double* blocks, int64_t capacity) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const HostStructure& h = s->hs;
  const int64_t len = h.diag_off_e.back();
  if (capacity < len) return fail(s, CERES_HIP_E_INVALID, "capacity %lld < %lld", (long long)capacity, (long long)len);
  if (s->path == CERES_HIP_PATH_BAL) {
    double* tmp = nullptr;
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(double) * len));
    hipError_t e = debug_poison(s, tmp, size_t(len));
    if (e == hipSuccess) e = LaunchExpandSym(s->etei, s->ops->ne, s->ops->etei_pitch, tmp, s->d_pt_eoff, s->plan.n_points, s->stream);  // internal point order -> the caller's E blocks
    int rc = e == hipSuccess ? down(s, blocks, tmp, size_t(len)) : fail(s, CERES_HIP_E_HIP, "expand failed");
    (void)hipFree(tmp);
    return rc;
  }
  return down(s, blocks, s->etei, size_t(len));
}

int ceres_hip_op_schur_sx(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  TRY(up(s, s->cg.p, x, s->hs.num_cols_f));
  TRY(op_sx(s, s->cg.p, s->cg.z, nullptr));
  return down(s, y, s->cg.z, s->hs.num_cols_f);
}

int ceres_hip_op_back_substitute(ceres_hip_solver* s, const double* z, double* x) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  if (s->hs.num_cols_f > 0) TRY(up(s, s->cg.p, z, s->hs.num_cols_f));
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_back_substitute(s, op, s->hs.num_cols_f > 0 ? s->cg.p : nullptr, s->own_x));
  return down(s, x, s->own_x, s->hs.num_cols);
}

int ceres_hip_op_power_series_operator(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  const int n = s->hs.num_cols_f;
  TRY(up(s, s->cg.p, x, n));
  TRY(up(s, s->cg.z, y, n));
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_power_series(s, op, s->cg.p, s->cg.z, nullptr));
  return down(s, y, s->cg.z, n);
}

int ceres_hip_op_spse_apply(ceres_hip_solver* s, const double* x, double* y, int32_t max_iters, double tolerance) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  if (max_iters < 1) return fail(s, CERES_HIP_E_INVALID, "max_num_spse_iterations < 1");
  const int n = s->hs.num_cols_f;
  TRY(up(s, s->cg.p, x, n));
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_spse_apply(s, op, s->cg.p, s->cg.z, max_iters, tolerance, nullptr));
  return down(s, y, s->cg.z, n);
}

int ceres_hip_op_block_jacobi_update(ceres_hip_solver* s) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  if (is_schur(s)) TRY(op_schur_init(s, op, false));
  TRY(op_preconditioner(s, op, CERES_HIP_JACOBI, s->precond, true));
  s->precond_valid = true;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return 0;
}

int ceres_hip_op_schur_jacobi_update(ceres_hip_solver* s) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, true));
  TRY(op_preconditioner(s, op, CERES_HIP_SCHUR_JACOBI, s->precond, true));
  s->precond_valid = true;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return 0;
}

int ceres_hip_op_cluster_jacobi_update(ceres_hip_solver* s) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_cluster_jacobi(s)) return fail(s, CERES_HIP_E_INVALID, "the handle was not created with the CLUSTER_JACOBI preconditioner");
  if (s->hs.ncb - s->hs.nelim <= 0) return fail(s, CERES_HIP_E_INVALID, "the structure has no F block");
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, false));
  bool failed = false;
  TRY(op_cluster_jacobi_update(s, op, &failed));
  if (failed) return fail(s, CERES_HIP_E_INVALID, "Preconditioner update failed.");
  return 0;
}

int ceres_hip_cluster_jacobi_stats(const ceres_hip_solver* s, int32_t* num_clusters, int32_t* largest_cluster_dimension, int64_t* factor_bytes,
                                   double* setup_seconds) {
  if (!s) return CERES_HIP_E_INVALID;
  if (!s->have_structure || !is_cluster_jacobi(s)) return CERES_HIP_E_INVALID;
  const ClusterLayoutHost& L = s->cluster_host;
  if (num_clusters) *num_clusters = L.num_clusters;
  if (largest_cluster_dimension) *largest_cluster_dimension = L.largest;
  if (factor_bytes) *factor_bytes = L.mat_off.empty() ? 0 : int64_t(sizeof(double)) * L.mat_off.back();
  if (setup_seconds) *setup_seconds = s->cluster_setup_seconds;
  return 0;
}

int ceres_hip_get_preconditioner_blocks(ceres_hip_solver* s, int32_t not_inverted, double* blocks, int64_t capacity) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (is_cluster_jacobi(s)) return fail(s, CERES_HIP_E_INVALID, "CLUSTER_JACOBI keeps one dense factor per cluster, not blocks per F block");
  const HostStructure& h = s->hs;
  const int64_t len = is_schur(s) ? h.diag_off_f.back() : h.diag_off_all.back();
  if (capacity < len) return fail(s, CERES_HIP_E_INVALID, "capacity %lld < %lld", (long long)capacity, (long long)len);
  if (!not_inverted) {
    if (!s->precond_valid) return fail(s, CERES_HIP_E_INVALID, "no preconditioner has been computed");
    TRY(precond_to_caller_order(s));  // a CGNR solve left its point blocks in CG's order
    return down(s, blocks, s->precond, size_t(len));
  }
  // re-assemble without inverting, into a temporary
  double* tmp = nullptr;
  HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&tmp), sizeof(double) * std::max<int64_t>(1, len)));
  int rc = debug_poison(s, tmp, size_t(len)) == hipSuccess ? 0 : fail(s, CERES_HIP_E_HIP, "CERES_HIP_DEBUG_POISON: filling a new buffer failed");
  int type = s->opt.preconditioner_type == CERES_HIP_IDENTITY ? CERES_HIP_JACOBI : s->opt.preconditioner_type;
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  if (!rc && is_schur(s)) rc = op_schur_init(s, op, true);
  if (!rc) rc = op_preconditioner(s, op, type, tmp, false);
  if (!rc) rc = down(s, blocks, tmp, size_t(len));
  (void)hipFree(tmp);
  return rc;
}

int ceres_hip_op_precond_apply(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (is_cluster_jacobi(s)) {   // y += M^-1 x, M^-1 x by two triangular solves per cluster
    if (!x || !y) return fail(s, CERES_HIP_E_INVALID, "x or y == NULL");
    if (!s->cluster_valid) return fail(s, CERES_HIP_E_INVALID, "no preconditioner has been computed");
    const int nf = s->hs.num_cols_f;
    TRY(up(s, s->cg.p, x, nf));
    TRY(up(s, s->cg.r, y, nf));
    TRY(op_cluster_jacobi_apply(s, s->cg.p, s->cg.z, nullptr));
    HIP_TRY(s, LaunchAxpby(1.0, s->cg.r, 1.0, s->cg.z, s->cg.z, nf, s->stream));
    return down(s, y, s->cg.z, nf);
  }
  if (!s->precond_valid) return fail(s, CERES_HIP_E_INVALID, "no preconditioner has been computed");
  TRY(precond_to_caller_order(s));  // a CGNR solve left its point blocks in CG's order
  const HostStructure& h = s->hs;
  const int n = is_schur(s) ? h.num_cols_f : h.num_cols;
  TRY(up(s, s->cg.p, x, n));
  TRY(up(s, s->cg.z, y, n));
  if (is_schur(s))
    HIP_TRY(s, LaunchGenBlockDiagonalApply(s->G, h.nelim, h.ncb - h.nelim, s->G.diag_off_f, s->precond, s->cg.p, s->cg.z, nullptr, s->stream));
  else
    HIP_TRY(s, LaunchGenBlockDiagonalApply(s->G, 0, h.ncb, s->G.diag_off_all, s->precond, s->cg.p, s->cg.z, nullptr, s->stream));
  return down(s, y, s->cg.z, n);
}

int ceres_hip_op_schur_eliminate_dense(ceres_hip_solver* s, double* lhs, double* rhs) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  if (s->path != CERES_HIP_PATH_GENERIC) return fail(s, CERES_HIP_E_UNSUPPORTED, "dense elimination runs on the generic path: create the solver with force_generic_path = 1");
  const HostStructure& h = s->hs;
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, false));
  const int64_t n = h.num_cols_f;
  double* d_lhs = nullptr;
  HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&d_lhs), sizeof(double) * std::max<int64_t>(1, n * n)));
  hipError_t e = debug_poison(s, d_lhs, size_t(n * n));
  if (e == hipSuccess) e = LaunchGenSchurDense(s->G, s->values, s->etei, s->D, d_lhs, s->stream);
  int rc = e == hipSuccess ? down(s, lhs, d_lhs, size_t(n * n)) : fail(s, CERES_HIP_E_HIP, "dense Schur kernel failed");
  (void)hipFree(d_lhs);
  if (rc) return rc;
  if (rhs && s->have_b) return down(s, rhs, s->rhs_f, size_t(n));
  return 0;
}

// ---- explicit Schur complement in BlockRandomAccessSparseMatrix storage (use_explicit_schur_complement, one rank) ----
int ceres_hip_schur_storage_info(const ceres_hip_solver* s, int64_t* num_block_pairs, int64_t* num_values) {
  if (!s || !s->have_structure || !s->sparse_S) return CERES_HIP_E_INVALID;
  if (num_block_pairs) *num_block_pairs = int64_t(s->schur_storage.pair_i.size());
  if (num_values) *num_values = s->schur_storage.num_values();
  return 0;
}

int ceres_hip_op_schur_eliminate_sparse(ceres_hip_solver* s, int32_t* pair_i, int32_t* pair_j, int64_t* pair_offset, double* values,
                                        int64_t pair_capacity, int64_t value_capacity) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!s->sparse_S) return fail(s, CERES_HIP_E_INVALID, "create the solver with use_explicit_schur_complement = 1 (one rank)");
  const SchurStorage& Q = s->schur_storage;
  const int64_t np = int64_t(Q.pair_i.size());
  if (pair_capacity < np || value_capacity < Q.num_values()) return fail(s, CERES_HIP_E_INVALID, "capacity too small");
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, false));
  HIP_TRY(s, LaunchSchurSparseEliminate(s->G, s->schur_pairs, s->values, s->etei, s->D, s->d_S, s->stream));
  for (int64_t p = 0; p < np; ++p) { pair_i[p] = Q.pair_i[p]; pair_j[p] = Q.pair_j[p]; pair_offset[p] = Q.pair_off[p]; }
  return down(s, values, s->d_S, size_t(Q.num_values()));
}

int ceres_hip_op_schur_symmetric_multiply(ceres_hip_solver* s, const double* x, double* y) {
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!s->sparse_S) return fail(s, CERES_HIP_E_INVALID, "create the solver with use_explicit_schur_complement = 1 (one rank)");
  const int n = s->hs.num_cols_f;
  TRY(up(s, s->cg.p, x, n));
  TRY(up(s, s->cg.z, y, n));
  HIP_TRY(s, LaunchSchurSparseSymv(s->G, s->schur_pairs, s->d_S, s->cg.p, s->cg.z, nullptr, 1, s->stream));
  return down(s, y, s->cg.z, n);
}

int ceres_hip_op_eliminator_back_substitute(ceres_hip_solver* s, const double* z, double* x) {
  // SchurEliminator::BackSubstitute recomputes (E^T E + D^2)^-1 per chunk and applies it to
  // E^T (b - F z): the same result as ImplicitSchurComplement::BackSubstitute after Init.
  TRY(require_loaded(s));
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (!is_schur(s)) return fail(s, CERES_HIP_E_INVALID, "not an ITERATIVE_SCHUR instance");
  SolveCtx op;   // operator-level call: a plain request, nothing promised
  TRY(op_schur_init(s, op, false));
  return ceres_hip_op_back_substitute(s, z, x);
}

int ceres_hip_op_dot(ceres_hip_solver* s, const double* x, const double* y, int64_t n, double* result) {
  if (!s || !s->have_structure) return CERES_HIP_E_INVALID;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (n > s->hs.num_cols) return fail(s, CERES_HIP_E_INVALID, "n exceeds num_cols");
  double *dx = s->scratch_vec, *dy = s->own_x;
  TRY(up(s, dx, x, size_t(n)));
  TRY(up(s, dy, y, size_t(n)));
  HIP_TRY(s, LaunchDot(dx, dy, n, s->cg.partials, s->cg.comm, s->stream));
  return down(s, result, s->cg.comm, 1);
}

int ceres_hip_op_axpby(ceres_hip_solver* s, double a, const double* x, double b, const double* y, int64_t n, double* z) {
  if (!s || !s->have_structure) return CERES_HIP_E_INVALID;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (n > s->hs.num_cols) return fail(s, CERES_HIP_E_INVALID, "n exceeds num_cols");
  double *dx = s->scratch_vec, *dy = s->own_x;
  TRY(up(s, dx, x, size_t(n)));
  TRY(up(s, dy, y, size_t(n)));
  HIP_TRY(s, LaunchAxpby(a, dx, b, dy, dy, n, s->stream));  // z may alias y (CG does both, I/conjugate_gradients_solver.h:190,220-226)
  return down(s, z, dy, size_t(n));
}

