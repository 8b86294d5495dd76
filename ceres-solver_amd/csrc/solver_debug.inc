// solver_debug.inc — part of solver.hip (included there, after the solver struct and the operators): debug exports of the host-side plans (testable without a GPU) and DenseCholesky on a caller-supplied matrix

// which way the last ITERATIVE_SCHUR solve of the handle got its point part (design/20_point_tail.md): 0 = the back-substitution pass over
// J, 1 = the point tail; < 0: no handle
int ceres_hip_debug_last_backsub_route(const ceres_hip_solver* s) { return s ? s->last_backsub_route : CERES_HIP_E_INVALID; }

// ---- debug exports: the host-side packing plan, testable without a GPU -------
int ceres_hip_debug_staged_x_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int64_t counts[4], int32_t* staged_cam,
                                  int32_t* slot_word, int64_t staged_capacity, int64_t slot_capacity) {
  try {
  if (!bs || !counts) return CERES_HIP_E_INVALID;
  HostStructure h;
  if (!AnalyzeStructure(*bs, num_eliminate_blocks, &h).empty()) return CERES_HIP_E_INVALID;
  BalPlan P;
  // the plan set_structure builds for a Schur solver (num_eliminate_blocks > 0: points always renumbered) / for CGNR (renumbered where its
  // CG vectors allow), with the hybrid request of a 256-CU device: the slot words exported here are the ones the device is given
  HybridRequest hyb;
  hyb.groups = 256;
  hyb.rows = 0;
  hyb.lds_bytes = int64_t(kMaxLdsBytes) - 512;
  BuildBalPlan(h, num_eliminate_blocks > 0 ? kReorderAlways : kReorderIfContiguous, hyb, &P);
  if (!P.eligible) return CERES_HIP_E_UNSUPPORTED;
  counts[0] = P.n_tiles; counts[1] = P.n_cameras; counts[2] = int64_t(P.xhot_cam.size());
  counts[3] = int64_t((size_t(P.nf) * P.n_cameras + size_t(P.ns)) * sizeof(double));
  if (staged_capacity >= int64_t(P.xhot_cam.size()) && staged_cam)
    for (size_t r = 0; r < P.xhot_cam.size(); ++r) staged_cam[r] = P.xhot_cam[r];
  const int64_t n_slots = P.n_tiles * kTile;
  if (slot_capacity >= n_slots && slot_word)
    for (int64_t i = 0; i < n_slots; ++i) slot_word[i] = P.slot_cam[i] < 0 ? -1 : P.slot_word[i];
  return 0;
  } catch (...) { return CERES_HIP_E_INVALID; }   // (host allocations sized by the caller's structure: no C++ exception crosses the C boundary)
}

// the clustering set_structure computes for CLUSTER_JACOBI (visibility.cc)
int ceres_hip_debug_cluster_cameras(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t visibility_clustering_type,
                                    int32_t* membership, int32_t* num_clusters) {
  try {
  if (!bs || !membership || !num_clusters) return CERES_HIP_E_INVALID;
  HostStructure h;
  if (!AnalyzeStructure(*bs, num_eliminate_blocks, &h).empty()) return CERES_HIP_E_INVALID;
  if (num_eliminate_blocks <= 0 || !h.chunks_contiguous) return CERES_HIP_E_INVALID;
  std::vector<int32_t> m;
  int n = 0;
  if (!ClusterCameras(h, visibility_clustering_type, &m, &n).empty()) return CERES_HIP_E_INVALID;
  for (size_t f = 0; f < m.size(); ++f) membership[f] = m[f];
  *num_clusters = n;
  return 0;
  } catch (...) { return CERES_HIP_E_INVALID; }
}

int ceres_hip_debug_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t* eligible,
                         int64_t* n_tiles, int32_t* slot_row_out, int32_t* slot_cam_out, int32_t* slot_pt_out,
                         uint32_t* slot_seg_out, int32_t* tile_kind_out, int32_t* tile_aux_out, int64_t slot_capacity,
                         char* why_not, int32_t why_capacity) {
  try {
  if (!bs || !eligible || !n_tiles) return CERES_HIP_E_INVALID;
  HostStructure h;
  std::string e = AnalyzeStructure(*bs, num_eliminate_blocks, &h);
  if (!e.empty()) { if (why_not) snprintf(why_not, why_capacity, "%s", e.c_str()); *eligible = 0; return CERES_HIP_E_INVALID; }
  BalPlan P;
  // CERES_HIP_DEBUG_PLAN_REORDER=1: the plan a Schur solver builds (points renumbered so that the tiles fill up)
  { const char* e = getenv("CERES_HIP_DEBUG_PLAN_REORDER"); BuildBalPlan(h, (e && atoi(e) != 0 && num_eliminate_blocks > 0) ? kReorderAlways : kReorderNever, HybridRequest(), &P); }
  *eligible = P.eligible ? 1 : 0;
  if (why_not) snprintf(why_not, why_capacity, "%s", P.why_not.c_str());
  *n_tiles = P.n_tiles;
  if (!P.eligible) return 0;
  const int64_t n_slots = P.n_tiles * kTile;
  if (slot_capacity < n_slots) return 0;  // caller only wanted the counts
  for (int64_t i = 0; i < n_slots; ++i) {
    slot_row_out[i] = P.slot_row[i];
    slot_cam_out[i] = P.slot_cam[i];
    slot_pt_out[i] = P.slot_pt[i];
    slot_seg_out[i] = P.slot_seg[i];
  }
  for (int64_t t = 0; t < P.n_tiles; ++t) { tile_kind_out[t] = P.tile_kind[t]; tile_aux_out[t] = P.tile_aux[t]; }
  return 0;
  } catch (...) { return CERES_HIP_E_INVALID; }   // (host allocations sized by the caller's structure: no C++ exception crosses the C boundary)
}

// the plan of the streamed upload (plan.cc, PlanValueStreams): host only, no device
int ceres_hip_debug_value_streams(const ceres_hip_block_structure* bs, int32_t* value_streams, int64_t* lo, int64_t* hi) {
  try {
  if (!bs || !value_streams) return CERES_HIP_E_INVALID;
  HostStructure h;
  if (!AnalyzeStructure(*bs, 0, &h).empty()) return CERES_HIP_E_INVALID;   // (the plan does not depend on the elimination order)
  ValueStreamPlan P;
  PlanValueStreams(h, &P);
  *value_streams = P.streams;
  for (int k = 0; k < 2; ++k) {
    if (lo) std::copy(P.lo[k].begin(), P.lo[k].end(), lo + size_t(k) * size_t(h.nrb));
    if (hi) std::copy(P.hi[k].begin(), P.hi[k].end(), hi + size_t(k) * size_t(h.nrb));
  }
  return 0;
  } catch (...) { return CERES_HIP_E_INVALID; }   // (host allocations sized by the caller's structure: no C++ exception crosses the C boundary)
}

// what the device holds as the loaded values and residuals of the handle's own copies (ceres_hip_load, ceres_hip_lm_compute_step,
// ceres_hip_values_end): tests compare the bytes that arrived, not a step computed from them.  Waits for the copy stream and the solver's.
int ceres_hip_debug_read_loaded(ceres_hip_solver* s, double* host_values_out, double* host_b_out) {
  if (!s) return CERES_HIP_E_INVALID;
  if (!s->have_structure) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_set_structure has not been called");
  HIP_TRY(s, hipSetDevice(s->opt.device));
  if (s->copy_stream) HIP_TRY(s, hipStreamSynchronize(s->copy_stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (host_values_out) HIP_TRY(s, hipMemcpy(host_values_out, s->own_values, sizeof(double) * size_t(s->hs.values_extent), hipMemcpyDeviceToHost));
  if (host_b_out) HIP_TRY(s, hipMemcpy(host_b_out, s->own_b, sizeof(double) * size_t(s->hs.num_rows), hipMemcpyDeviceToHost));
  return 0;
}

int ceres_hip_op_dense_cholesky_solve(ceres_hip_solver* s, int32_t n, const double* A, const double* b, double* x, int32_t repeats,
                                      double* factor_ms, int32_t* failed) {
  if (!s || !A || !b || !x || n < 1 || repeats < 1) return CERES_HIP_E_INVALID;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  hipStream_t st = s->stream;
  const size_t nn = size_t(n) * size_t(n);
  double *dA0 = nullptr, *dA = nullptr, *dx = nullptr;
  int* dflag = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto cleanup = [&] {
    if (dA0) (void)hipFree(dA0); if (dA) (void)hipFree(dA); if (dx) (void)hipFree(dx); if (dflag) (void)hipFree(dflag);
    if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1);
  };
  auto run = [&]() -> int {
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dA0), nn * sizeof(double)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dA), nn * sizeof(double)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dx), size_t(n) * sizeof(double)));
    HIP_TRY(s, debug_poison(s, dA0, nn));
    HIP_TRY(s, debug_poison(s, dA, nn));
    HIP_TRY(s, debug_poison(s, dx, size_t(n)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dflag), sizeof(int)));
    HIP_TRY(s, hipEventCreate(&e0)); HIP_TRY(s, hipEventCreate(&e1));
    HIP_TRY(s, hipMemcpyAsync(dA0, A, nn * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(s, hipMemcpyAsync(dx, b, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(s, hipMemsetAsync(dflag, 0, sizeof(int), st));
    double total = 0.0;
    for (int r = 0; r < repeats; ++r) {   // the factorisation is in place: every repeat starts from a fresh copy, only the factorisation is timed
      HIP_TRY(s, hipMemcpyAsync(dA, dA0, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
      HIP_TRY(s, hipEventRecord(e0, st));
      HIP_TRY(s, LaunchDenseCholesky(dA, n, dflag, st));
      HIP_TRY(s, hipEventRecord(e1, st));
      HIP_TRY(s, hipEventSynchronize(e1));
      float ms = 0;
      HIP_TRY(s, hipEventElapsedTime(&ms, e0, e1));
      total += ms;
    }
    if (factor_ms) *factor_ms = total / repeats;
    int flag = 0;
    HIP_TRY(s, hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(s, hipStreamSynchronize(st));
    if (failed) *failed = flag;
    if (!flag) HIP_TRY(s, LaunchDenseCholeskySolve(dA, n, dx, st));
    HIP_TRY(s, hipMemcpyAsync(x, dx, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(s, hipStreamSynchronize(st));
    return 0;
  };
  const int rc = run();
  cleanup();
  return rc;
}

// The same factorisation with the factor itself returned and the memory around the matrix and the vector watched: both sit in the middle
// of larger allocations whose guard bands (2 * 128 rows of n doubles on either side of the matrix, 256 doubles on either side of the
// vector) are filled with the byte 0x5A (a finite double) before the first run and compared word by word after the last.
int ceres_hip_op_dense_cholesky_factor(ceres_hip_solver* s, int32_t n, const double* A, const double* b, double* factor, double* x,
                                       int32_t repeats, int32_t* failed, int64_t* guard_words_changed, int32_t* repeatable) {
  if (!s || !A || !factor || (b && !x) || n < 1 || repeats < 1) return CERES_HIP_E_INVALID;
  try {
  HIP_TRY(s, hipSetDevice(s->opt.device));
  hipStream_t st = s->stream;
  const size_t nn = size_t(n) * size_t(n);
  const size_t mat_guard = size_t(2) * 128 * size_t(n), vec_guard = 256;
  const size_t mat_words = nn + 2 * mat_guard, vec_words = size_t(n) + 2 * vec_guard;
  constexpr int kGuardByte = 0x5A;
  double *dA0 = nullptr, *dbuf = nullptr, *dvec = nullptr;
  int* dflag = nullptr;
  auto cleanup = [&] {
    if (dA0) (void)hipFree(dA0); if (dbuf) (void)hipFree(dbuf); if (dvec) (void)hipFree(dvec); if (dflag) (void)hipFree(dflag);
  };
  std::vector<double> previous;
  if (repeats > 1) previous.resize(nn);
  std::vector<uint64_t> guard(std::max(mat_guard, vec_guard));
  int64_t changed = 0;
  int same = 1, flag = 0;
  auto run = [&]() -> int {
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dA0), nn * sizeof(double)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dbuf), mat_words * sizeof(double)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dvec), vec_words * sizeof(double)));
    HIP_TRY(s, hipMalloc(reinterpret_cast<void**>(&dflag), sizeof(int)));
    double* dA = dbuf + mat_guard;
    double* dx = dvec + vec_guard;
    HIP_TRY(s, hipMemsetAsync(dbuf, kGuardByte, mat_words * sizeof(double), st));
    HIP_TRY(s, hipMemsetAsync(dvec, kGuardByte, vec_words * sizeof(double), st));
    HIP_TRY(s, hipMemcpyAsync(dA0, A, nn * sizeof(double), hipMemcpyHostToDevice, st));
    for (int r = 0; r < repeats; ++r) {   // in place: every repeat starts from a fresh copy of the matrix and of b
      HIP_TRY(s, hipMemcpyAsync(dA, dA0, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (b) HIP_TRY(s, hipMemcpyAsync(dx, b, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(s, hipMemsetAsync(dflag, 0, sizeof(int), st));
      HIP_TRY(s, LaunchDenseCholesky(dA, n, dflag, st));
      int this_flag = 0;
      HIP_TRY(s, hipMemcpyAsync(&this_flag, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(s, hipStreamSynchronize(st));
      if (b && !this_flag) HIP_TRY(s, LaunchDenseCholeskySolve(dA, n, dx, st));
      if (r > 0) std::memcpy(previous.data(), factor, nn * sizeof(double));
      HIP_TRY(s, hipMemcpyAsync(factor, dA, nn * sizeof(double), hipMemcpyDeviceToHost, st));
      if (b) HIP_TRY(s, hipMemcpyAsync(x, dx, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(s, hipStreamSynchronize(st));
      if (r > 0) {
        if (this_flag != flag) same = 0;
        for (size_t i = 0; i < size_t(n) && same; ++i)
          if (std::memcmp(previous.data() + i * size_t(n), factor + i * size_t(n), (i + 1) * sizeof(double)) != 0) same = 0;
      }
      flag = this_flag;
    }
    uint64_t pattern;
    std::memset(&pattern, kGuardByte, sizeof(pattern));
    const double* bands[4] = {dbuf, dbuf + mat_guard + nn, dvec, dvec + vec_guard + size_t(n)};
    const size_t words[4] = {mat_guard, mat_guard, vec_guard, vec_guard};
    for (int k = 0; k < 4; ++k) {
      HIP_TRY(s, hipMemcpyAsync(guard.data(), bands[k], words[k] * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(s, hipStreamSynchronize(st));
      for (size_t i = 0; i < words[k]; ++i) changed += guard[i] != pattern;
    }
    return 0;
  };
  const int rc = run();
  cleanup();
  if (rc != 0) return rc;
  if (failed) *failed = flag;
  if (guard_words_changed) *guard_words_changed = changed;
  if (repeatable) *repeatable = same;
  return 0;
  } catch (...) { return CERES_HIP_E_INVALID; }   // (host buffers sized by the caller's n: no C++ exception crosses the C boundary)
}

int ceres_hip_debug_hybrid_plan(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t groups, int32_t rows,
                                int64_t counts[8], int32_t* slot_word, int32_t* slot_row, int32_t* tile_zbase, int32_t* grp_tile_ptr,
                                int32_t* entry_row, int32_t* unit_cam, int32_t* unit_begin, int32_t* unit_end,
                                int64_t slot_capacity, int64_t entry_capacity, int64_t unit_capacity) {
  if (!bs || !counts) return CERES_HIP_E_INVALID;
  if (!bs || !counts) return CERES_HIP_E_INVALID;
  HostStructure h;
  if (!AnalyzeStructure(*bs, num_eliminate_blocks, &h).empty()) return CERES_HIP_E_INVALID;
  BalPlan P;
  HybridRequest hyb;
  hyb.groups = groups; hyb.rows = rows;
  BuildBalPlan(h, num_eliminate_blocks > 0 ? kReorderAlways : kReorderNever, hyb, &P);
  if (!P.eligible || P.cameras_in_lds) return CERES_HIP_E_UNSUPPORTED;
  const int64_t n_slots = P.n_tiles * kTile, n_entries = int64_t(P.zc_slot.size()), n_units = int64_t(P.zu_cam.size());
  counts[0] = P.n_tiles; counts[1] = P.hybrid ? 1 : 0; counts[2] = P.hyb_rows; counts[3] = P.hyb_hot;
  counts[4] = P.z_flush_row0; counts[5] = P.z_ring_rows; counts[6] = n_entries; counts[7] = n_units;
  if (slot_capacity < n_slots || entry_capacity < n_entries || unit_capacity < n_units) return 0;  // the caller only wanted the counts
  for (int64_t i = 0; i < n_slots; ++i) {
    slot_word[i] = P.slot_cam[i] < 0 ? -1 : P.slot_word[i];
    slot_row[i] = P.slot_row[i];
  }
  std::copy(P.tile_zbase.begin(), P.tile_zbase.end(), tile_zbase);
  if (P.hybrid) std::copy(P.grp_tile_ptr.begin(), P.grp_tile_ptr.end(), grp_tile_ptr);
  std::copy(P.zc_slot.begin(), P.zc_slot.end(), entry_row);
  std::copy(P.zu_cam.begin(), P.zu_cam.end(), unit_cam);
  std::copy(P.zu_begin.begin(), P.zu_begin.end(), unit_begin);
  std::copy(P.zu_end.begin(), P.zu_end.end(), unit_end);
  return 0;
}

int ceres_hip_debug_long_rounds(const ceres_hip_block_structure* bs, int32_t num_eliminate_blocks, int32_t renumber, int32_t groups,
                                int32_t rows, int64_t counts[5], int32_t* tile_kind, int32_t* tile_aux, int32_t* range_tile_ptr,
                                int32_t* long_ptr, int32_t* round_ptr, int32_t* seq_ptr, int32_t* round_flag, uint32_t* round_word,
                                int64_t tile_capacity, int64_t range_capacity, int64_t round_capacity) {
  if (!bs || !counts) return CERES_HIP_E_INVALID;
  if (!bs || !counts) return CERES_HIP_E_INVALID;
  HostStructure h;
  if (!AnalyzeStructure(*bs, num_eliminate_blocks, &h).empty()) return CERES_HIP_E_INVALID;
  BalPlan P;
  HybridRequest hyb;
  hyb.groups = groups; hyb.rows = rows;
  BuildBalPlan(h, renumber ? kReorderAlways : kReorderNever, hyb, &P);
  if (!P.eligible) return CERES_HIP_E_UNSUPPORTED;
  const int64_t n_ranges = int64_t(P.long_ptr.size()), n_rounds = int64_t(P.round_word.size()) / kRoundWaves;
  counts[0] = P.n_tiles; counts[1] = n_ranges; counts[2] = n_rounds; counts[3] = P.long_behind ? 1 : 0; counts[4] = int64_t(P.seq_ptr.size()) - 1;
  if (tile_capacity < P.n_tiles || range_capacity < n_ranges || round_capacity < n_rounds) return 0;  // the caller only wanted the counts
  std::copy(P.tile_kind.begin(), P.tile_kind.end(), tile_kind);
  std::copy(P.tile_aux.begin(), P.tile_aux.end(), tile_aux);
  if (P.grp_tile_ptr.empty()) { range_tile_ptr[0] = 0; range_tile_ptr[1] = int32_t(P.n_tiles); }
  else std::copy(P.grp_tile_ptr.begin(), P.grp_tile_ptr.end(), range_tile_ptr);
  std::copy(P.long_ptr.begin(), P.long_ptr.end(), long_ptr);
  std::copy(P.round_ptr.begin(), P.round_ptr.end(), round_ptr);
  std::copy(P.round_word.begin(), P.round_word.end(), round_word);
  std::copy(P.seq_ptr.begin(), P.seq_ptr.end(), seq_ptr);
  std::copy(P.round_flag.begin(), P.round_flag.end(), round_flag);
  return 0;
}

}  // extern "C"

