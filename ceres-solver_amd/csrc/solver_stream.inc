// solver_stream.inc — part of solver.hip (included there, after the solver struct and the operators): the upload hidden behind the evaluator (ceres_hip_values_begin / _ready / _end)

// ---- streamed upload: the evaluator's finished rows go up while it is still writing the later ones ----------------------------
namespace {
// (stream_mu held) the plan of the value streams, once per structure: plan.cc, PlanValueStreams
void plan_value_streams(ceres_hip_solver* s) {
  ValueStreamPlan P;
  PlanValueStreams(s->hs, &P);
  s->n_value_streams = P.streams;
  for (int k = 0; k < 2; ++k) { s->stream_lo[k].swap(P.lo[k]); s->stream_hi[k].swap(P.hi[k]); }
  s->stream_plan_ready = true;
}
}  // namespace

int ceres_hip_values_begin(ceres_hip_solver* s, const double* host_values, const double* host_residuals) {
  if (!s || !host_values || !host_residuals) return CERES_HIP_E_INVALID;
  if (!s->have_structure) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_set_structure has not been called");
  HIP_TRY(s, hipSetDevice(s->opt.device));
  std::lock_guard<std::mutex> lock(s->stream_mu);
  // (a second _begin would reset stream_row_sent under copies that are still queued; the open session stays as it is)
  if (s->streaming) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_values_begin between ceres_hip_values_begin and ceres_hip_values_end");
  if (!s->copy_stream) {
    HIP_TRY(s, hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    HIP_TRY(s, hipEventCreateWithFlags(&s->copy_done, hipEventDisableTiming));
  }
  if (!s->stream_plan_ready) plan_value_streams(s);
  // the previous step may still be reading own_values / own_b on the solver's stream: the copies wait for it
  HIP_TRY(s, hipEventRecord(s->copy_done, s->stream));
  HIP_TRY(s, hipStreamWaitEvent(s->copy_stream, s->copy_done, 0));
  s->stream_row_sent.assign(size_t(s->hs.nrb), 0);
  s->stream_host_values = host_values;
  s->stream_host_b = host_residuals;
  s->stream_rows_sent = 0; s->stream_bytes_early = 0; s->stream_bytes_late = 0;
  s->streaming = true;
  return 0;
}

namespace {
// (stream_mu held) enqueue the copies of row blocks [r0, r1) on the copy stream
int send_rows(ceres_hip_solver* s, int r0, int r1, int64_t* bytes) {
  const HostStructure& h = s->hs;
  for (int k = 0; k < s->n_value_streams; ++k) {
    const int64_t lo = s->stream_lo[k][size_t(r0)], hi = s->stream_hi[k][size_t(r1 - 1)];
    if (hi > lo) {
      HIP_TRY(s, hipMemcpyAsync(s->own_values + lo, s->stream_host_values + lo, sizeof(double) * size_t(hi - lo), hipMemcpyHostToDevice, s->copy_stream));
      *bytes += 8 * (hi - lo);
    }
  }
  const int64_t b0 = h.rpos[size_t(r0)], b1 = int64_t(h.rpos[size_t(r1 - 1)]) + h.rsz[size_t(r1 - 1)];
  if (b1 > b0) {
    HIP_TRY(s, hipMemcpyAsync(s->own_b + b0, s->stream_host_b + b0, sizeof(double) * size_t(b1 - b0), hipMemcpyHostToDevice, s->copy_stream));
    *bytes += 8 * (b1 - b0);
  }
  return 0;
}
}  // namespace

int ceres_hip_values_ready(ceres_hip_solver* s, int32_t first_row_block, int32_t num_row_blocks) {
  if (!s) return CERES_HIP_E_INVALID;
  if (num_row_blocks <= 0) return 0;
  // (no s->err on this path before the lock: several evaluator threads call it at once)
  if (hipSetDevice(s->opt.device) != hipSuccess) return CERES_HIP_E_HIP;
  std::lock_guard<std::mutex> lock(s->stream_mu);
  if (!s->streaming) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_values_ready outside ceres_hip_values_begin / _end");
  const int r0 = first_row_block, r1 = first_row_block + num_row_blocks;
  if (r0 < 0 || r1 > s->hs.nrb) return fail(s, CERES_HIP_E_INVALID, "row blocks [%d, %d) out of range", r0, r1);
  for (int r = r0; r < r1; ++r) {
    if (s->stream_row_sent[size_t(r)]) return fail(s, CERES_HIP_E_INVALID, "row block %d was announced twice", r);
    s->stream_row_sent[size_t(r)] = 1;
  }
  s->stream_rows_sent += num_row_blocks;
  if (s->n_value_streams == 0) return 0;   // a layout without monotone value streams: remembered, sent in _end
  return send_rows(s, r0, r1, &s->stream_bytes_early);
}

int ceres_hip_values_end(ceres_hip_solver* s, const double* host_column_scale) {
  if (!s) return CERES_HIP_E_INVALID;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  std::lock_guard<std::mutex> lock(s->stream_mu);
  if (!s->streaming) return fail(s, CERES_HIP_E_INVALID, "ceres_hip_values_end without ceres_hip_values_begin");
  s->streaming = false;
  const HostStructure& h = s->hs;
  if (s->n_value_streams == 0) {   // nothing went up early
    HIP_TRY(s, hipMemcpyAsync(s->own_values, s->stream_host_values, sizeof(double) * size_t(h.values_extent), hipMemcpyHostToDevice, s->copy_stream));
    HIP_TRY(s, hipMemcpyAsync(s->own_b, s->stream_host_b, sizeof(double) * size_t(h.num_rows), hipMemcpyHostToDevice, s->copy_stream));
    s->stream_bytes_late += 8 * (h.values_extent + h.num_rows);
  } else if (s->stream_rows_sent < h.nrb) {   // rows nobody announced: now, run by run
    for (int r = 0; r < h.nrb;) {
      if (s->stream_row_sent[size_t(r)]) { ++r; continue; }
      int e = r;
      while (e < h.nrb && !s->stream_row_sent[size_t(e)]) ++e;
      TRY(send_rows(s, r, e, &s->stream_bytes_late));
      r = e;
    }
  }
  HIP_TRY(s, hipEventRecord(s->copy_done, s->copy_stream));
  HIP_TRY(s, hipStreamWaitEvent(s->stream, s->copy_done, 0));   // (work queued behind it is ordered without relying on the host)
  // the HOST waits too: the copies enqueued above read the caller's (pinned) arrays asynchronously, and the caller may write, scale or
  // free them as soon as this returns (Ceres scales its Jacobian in place right behind the evaluation)
  HIP_TRY(s, hipEventSynchronize(s->copy_done));
  TRY(load_device(s, s->own_values, s->own_b, nullptr));
  if (host_column_scale) {   // BlockSparseMatrix::ScaleColumns on the copy in HBM (I/block_sparse_matrix.cc:403-450, I/trust_region_minimizer.cc:263-279)
    HIP_TRY(s, hipMemcpyAsync(s->scratch_vec, host_column_scale, sizeof(double) * size_t(h.num_cols), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, LaunchGenScaleColumns(s->G, s->own_values, s->scratch_vec, s->stream));
  }
  return 0;
}

int ceres_hip_get_stream_stats(const ceres_hip_solver* s, int64_t* bytes_early, int64_t* bytes_late, int32_t* value_streams) {
  if (!s) return CERES_HIP_E_INVALID;
  if (bytes_early) *bytes_early = s->stream_bytes_early;
  if (bytes_late) *bytes_late = s->stream_bytes_late;
  if (value_streams) *value_streams = s->n_value_streams;
  return 0;
}

