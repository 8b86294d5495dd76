// Bound constraints of the BAL front end (textually included by bal_frontend.inc after line_search.inc, whose Armijo search, option
// rules and gradient-only evaluator it uses).  A restatement of
//
//   ParameterBlock::Plus (the clamp)                   I/parameter_block.h:227-255
//   Program::IsBoundsConstrained / IsFeasible          I/program.cc:215-289
//   TrustRegionMinimizer: the initial projection, the projected gradient norm, DoLineSearch, the ambient step norm
//                                                      I/trust_region_minimizer.cc:103-108, 210-220, 281-302, 596-641, 726-748
//   LineSearchFunction / ArmijoLineSearch              I/line_search.cc:103-145, 281-366 (ls_armijo_search)
//   LineSearchPreprocessor: no bounds                  I/line_search_preprocessor.cc:47-51
//
// The setters, the feasibility checks, the projected search as a callback for ls_armijo_search, and the statistics.  The device side is
// kernels_bounds.hip.  ceres_hip_bal_minimize tests p->is_constrained before everything it does here: false on every handle that never
// set a bound that binds a free block.

struct BalBoundsState {
  std::vector<double> lower, upper;   // the caller's arrays (n_a each; empty: no bound on that side), as given
  LsSearchOptions search;             // the six line-search fields
  unsigned long long* d_counts = nullptr;   // kMaxVecGrid: the projection's per-workgroup counts
  unsigned long long* h_counts = nullptr;   // pinned
  double* d_ls_grad = nullptr;              // n_t: a sample's gradient (CUBIC)
  // the search of the iteration in progress (ceres_hip_bal_minimize logs it with the iteration)
  int32_t cur_iterations = -1, cur_success = 0;
  double cur_step = 1.0;
  // ceres_hip_bal_bounds_stats: of the last ceres_hip_bal_minimize on a constrained handle; reset by every ceres_hip_bal_set_bounds
  int32_t ran_constrained = 0, num_line_search_steps = 0, num_function_evaluations = 0, num_gradient_evaluations = 0;
  double line_search_seconds = 0.0;
  int64_t num_projected = 0;
  int32_t it_iterations[CERES_HIP_MAX_LOGGED_ITERATIONS], it_success[CERES_HIP_MAX_LOGGED_ITERATIONS];
  double it_step[CERES_HIP_MAX_LOGGED_ITERATIONS];
  void reset_stats() {
    ran_constrained = num_line_search_steps = num_function_evaluations = num_gradient_evaluations = 0;
    line_search_seconds = 0.0;
    num_projected = 0;
    cur_iterations = -1; cur_success = 0; cur_step = 1.0;
    for (int i = 0; i < CERES_HIP_MAX_LOGGED_ITERATIONS; ++i) { it_iterations[i] = -1; it_success[i] = 0; it_step[i] = 1.0; }
  }
};

void bal_bounds_free(ceres_hip_bal* p) {
  if (!p->bounds) return;
  if (p->bounds->h_counts) (void)hipHostFree(p->bounds->h_counts);
  delete p->bounds;
  p->bounds = nullptr;
}

namespace {

// the kernels' view of the bounds: the plain form where every block is free, else the loop's free-block list
BalBounds bal_bounds_args(const ceres_hip_bal* p) {
  BalBounds K;
  K.lower = p->d_lower; K.upper = p->d_upper; K.camera_width = p->cs;
  if (p->has_const) K.B = BalFreeBlocks{p->d_free_block, p->nfp, p->nfc};
  else K.B = BalFreeBlocks{nullptr, p->n_a, 0};
  return K;
}

// the step size the iteration's projected search settled on (1: it failed or has not run)
double bal_bounds_step_size(const ceres_hip_bal* p) { return p->bounds->cur_step; }

// is the state coordinate i part of a free block?  (block_name: "point 3" / "camera 0", index_in_block: the coordinate inside it)
bool bal_bounds_coordinate(const ceres_hip_bal* p, int64_t i, std::string* block_name, int* index_in_block) {
  const int64_t np3 = 3 * int64_t(p->np);
  const bool point = i < np3;
  const int64_t b = point ? i / 3 : (i - np3) / p->cs;
  if (index_in_block) *index_in_block = int(point ? i % 3 : (i - np3) % p->cs);
  if (block_name) *block_name = (point ? "point " : "camera ") + std::to_string(b);
  if (!p->has_const) return true;
  return (point ? p->pt_col[size_t(b)] : p->cam_col[size_t(b)]) >= 0;
}

// x = clamp(x) on the free blocks of a device state; *moved: the coordinates changed (exact)
int bal_bounds_project_device(ceres_hip_bal* p, double* d_state, int64_t* moved) {
  ceres_hip_solver* s = p->s;
  BalBoundsState* b = p->bounds;
  int n = 0;
  HIP_TRY(s, LaunchBoundsProject(bal_bounds_args(p), d_state, b->d_counts, &n, s->stream));
  HIP_TRY(s, hipMemcpyAsync(b->h_counts, b->d_counts, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  unsigned long long c = 0;
  for (int i = 0; i < n; ++i) c += b->h_counts[i];
  *moved = int64_t(c);
  return 0;
}

// Program::IsFeasible for the constant blocks, on the caller's host state: "" or Ceres' message with the block, the index and the
// three numbers
std::string bal_bounds_constant_infeasible(const ceres_hip_bal* p, const double* state) {
  const BalBoundsState* b = p->bounds;
  if (!p->has_const) return "";
  for (int64_t i = 0; i < p->n_a; ++i) {
    if (bal_bounds_coordinate(p, i, nullptr, nullptr)) continue;
    const double lo = b->lower.empty() ? -std::numeric_limits<double>::infinity() : b->lower[size_t(i)];
    const double hi = b->upper.empty() ? std::numeric_limits<double>::infinity() : b->upper[size_t(i)];
    if (!(state[i] < lo) && !(state[i] > hi)) continue;
    std::string block;
    int j = 0;
    bal_bounds_coordinate(p, i, &block, &j);
    return ls_format("ParameterBlock: %s is constant and its value is infeasible. First infeasible value is at index: %d. Lower bound: %.17g, "
                     "value: %.17g, upper bound: %.17g", block.c_str(), j, lo, state[i], hi);
  }
  return "";
}

// DoLineSearch, I/trust_region_minimizer.cc:596-641: the projected Armijo search along delta = step .* scale from the device state x
// (cost x_cost, scaled gradient p->d_grad).  phi(a) = cost(clamp(x + a delta)), evaluated in `cand`; per sample one host round trip of
// scalars.  Leaves the search's iterations, success and step size in p->bounds->cur_*; p->d_delta holds the unscaled full step.
int bal_bounds_line_search(ceres_hip_bal* p, const double* x, const double* scale, double* cand, double x_cost) {
  ceres_hip_solver* s = p->s;
  hipStream_t st = s->stream;
  BalBoundsState* b = p->bounds;
  PartialSums& P = p->parts;
  const auto t0 = std::chrono::steady_clock::now();
  const BalBounds K = bal_bounds_args(p);
  LsSearchOptions so = b->search;
  const bool cubic = so.interpolation_type == CERES_HIP_CUBIC;
  bool first = true;
  LsSample initial;
  initial.x = 0.0; initial.value = x_cost; initial.value_is_valid = true; initial.gradient_is_valid = true;
  // a sample: the trial point, its cost (the gradient-only evaluator's cost-only form unless CUBIC), g(x_a) . delta; the first one
  // also brings phi'(0) = g . delta and |delta|_inf, which the search reads only after it
  auto sample = [&](double a, bool want_gradient, LsSample* out) -> int {
    *out = LsSample();
    out->x = a;
    int ntp = 0; double* parts = nullptr;
    PartialSet cost, delta_max, grad_delta, dg, unused;
    TRY(bal_parts_room(p, 4 * kMaxVecGrid, &parts));
    HIP_TRY(s, LaunchBoundsTrialPoint(K, x, p->d_step, scale, first ? p->d_grad : nullptr, a, false, p->d_delta, cand, parts, &ntp, st));
    P.take(ntp); P.take(ntp);   // (|x|^2 and |cand - x|^2: the loop reads its own candidate's)
    delta_max = P.take(ntp); grad_delta = P.take(ntp);
    TRY(bal_ls_evaluate_enqueue(p, cand, want_gradient ? b->d_ls_grad : nullptr, &cost));
    if (want_gradient) TRY(bal_ls_dots_enqueue(p, p->d_delta, b->d_ls_grad, nullptr, &dg, &unused, &unused));
    TRY(bal_parts_collect(p));
    out->value = P.sum(cost);
    out->value_is_valid = std::isfinite(out->value);
    out->vector_x_is_valid = true;
    if (first) {
      initial.gradient = P.sum(grad_delta);
      so.direction_max_norm = P.max(delta_max);
      first = false;
    }
    if (!out->value_is_valid || !want_gradient) return 0;
    const double g = P.sum(dg);
    out->gradient = g;
    if (std::isfinite(g)) { out->gradient_is_valid = true; out->vector_gradient_is_valid = true; }
    return 0;
  };
  // The first sample (a = 1) before the search proper: its round trip carries phi'(0) and |delta|_inf, which ls_armijo_search takes at
  // its entry.  The search's own first evaluation is handed this sample.
  LsSample first_sample;
  TRY(sample(1.0, cubic, &first_sample));
  bool handed = false;
  LsEvaluate eval = [&](double a, bool want_gradient, LsSample* out) -> int {
    if (!handed) { handed = true; *out = first_sample; return 0; }
    return sample(a, want_gradient, out);
  };
  LsSearchSummary R;
  ls_armijo_search(so, eval, initial, 1.0, &R);
  if (R.rc != 0) return R.rc;
  b->cur_iterations = R.num_iterations;
  b->cur_success = R.success ? 1 : 0;
  b->cur_step = R.success ? R.optimal_point.x : 1.0;   // failure: delta stays whole
  b->num_line_search_steps += R.num_iterations;
  b->num_function_evaluations += R.num_function_evaluations;
  b->num_gradient_evaluations += R.num_gradient_evaluations;
  b->line_search_seconds += seconds_since(t0);
  return 0;
}

// the search of the iteration being logged, at the index of summary.iterations[]
void bal_bounds_log(ceres_hip_bal* p, int index) {
  BalBoundsState* b = p->bounds;
  if (index >= 0 && index < CERES_HIP_MAX_LOGGED_ITERATIONS) {
    b->it_iterations[index] = b->cur_iterations; b->it_success[index] = b->cur_success; b->it_step[index] = b->cur_step;
  }
  b->cur_iterations = -1; b->cur_success = 0; b->cur_step = 1.0;
}

}  // namespace

extern "C" {

int ceres_hip_bal_set_bounds(ceres_hip_bal* p, const double* lower, const double* upper, const ceres_hip_line_search_options* lso) try {
  auto refuse = [&](int code, const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_set_bounds: " + why;
    return code;
  };
  if (!p) return refuse(CERES_HIP_E_INVALID, "NULL problem handle");
  // the six fields DoLineSearch reads, by ls_validate's rules and wording: the other fields keep their (valid) defaults
  ceres_hip_line_search_options o;
  ceres_hip_line_search_default_options(&o);
  if (lso) {
    o.line_search_interpolation_type = lso->line_search_interpolation_type;
    o.min_line_search_step_size = lso->min_line_search_step_size;
    o.line_search_sufficient_function_decrease = lso->line_search_sufficient_function_decrease;
    o.max_line_search_step_contraction = lso->max_line_search_step_contraction;
    o.min_line_search_step_contraction = lso->min_line_search_step_contraction;
    o.max_num_line_search_step_size_iterations = lso->max_num_line_search_step_size_iterations;
    // (the one rule of the six that reads a seventh field: sufficient decrease < sufficient curvature decrease, a WOLFE field — kept
    // out of the way, the bare "> 0.0" and "< 1.0" remain)
    if (o.line_search_sufficient_function_decrease > 0.0 && o.line_search_sufficient_function_decrease < 1.0)
      o.line_search_sufficient_curvature_decrease = 0.5 * (o.line_search_sufficient_function_decrease + 1.0);
    bool unsupported = false;
    const std::string why = ls_validate(o, &unsupported);
    if (!why.empty()) return refuse(CERES_HIP_E_INVALID, why);
  }
  ceres_hip_solver* s = p->s;
  if (lower || upper) {
    if (p->camera_model == CERES_HIP_CAMERA_QUATERNION_MANIFOLD)
      return refuse(CERES_HIP_E_UNSUPPORTED, "bounds are not supported on handles with quaternion-manifold cameras");
    if (p->intrinsics_mask) return refuse(CERES_HIP_E_UNSUPPORTED, "bounds are not supported on handles with fixed intrinsics");
    if (s->world > 1) return refuse(CERES_HIP_E_UNSUPPORTED, "bounds are not supported on sharded handles");
  }
  const double inf = std::numeric_limits<double>::infinity(), dmax = std::numeric_limits<double>::max();
  const int64_t n = p->n_a;
  bool constrained = false;
  for (int64_t i = 0; i < n; ++i) {
    const double lo = lower ? lower[i] : -inf, hi = upper ? upper[i] : inf;
    if (std::isnan(lo) || std::isnan(hi))
      return refuse(CERES_HIP_E_INVALID, ls_format("%s bound %lld is NaN", std::isnan(lo) ? "lower" : "upper", (long long)i));
  }
  for (int64_t i = 0; i < n && (lower || upper); ++i) {
    if (!bal_bounds_coordinate(p, i, nullptr, nullptr)) continue;   // (a constant block's bounds are kept, never applied)
    const double lo = lower ? lower[i] : -inf, hi = upper ? upper[i] : inf;
    std::string block;
    int j = 0;
    if (lo >= hi && bal_bounds_coordinate(p, i, &block, &j))
      return refuse(CERES_HIP_E_INVALID, ls_format("ParameterBlock: %s has at least one infeasible bound. First infeasible bound is at index: %d. "
                                                   "Lower bound: %.17g, upper bound: %.17g", block.c_str(), j, lo, hi));
    // (shared intrinsics: a bound on one camera's intrinsics would be a bound on its group's block; bounds that constrain nothing pass)
    if (p->n_groups && (lo > -dmax || hi < dmax)) return refuse(CERES_HIP_E_UNSUPPORTED, "bounds are not supported on handles with shared intrinsics");
    constrained = constrained || lo > -dmax || hi < dmax;
  }
  if (constrained) {
    HIP_TRY(s, hipSetDevice(s->opt.device));
    BAL_TRY(p, bal_ls_prepare(p));   // the samples' evaluator (bal_ls_evaluate_enqueue)
    if (!p->bounds) {
      std::unique_ptr<BalBoundsState> b(new BalBoundsState);
      b->reset_stats();
      BAL_TRY(p, dev_alloc(s, &p->d_lower, size_t(n)));
      BAL_TRY(p, dev_alloc(s, &p->d_upper, size_t(n)));
      BAL_TRY(p, dev_alloc(s, &b->d_ls_grad, size_t(p->n_t)));
      BAL_TRY(p, dev_alloc(s, &b->d_counts, size_t(kMaxVecGrid)));
      HIP_TRY(s, hipHostMalloc(reinterpret_cast<void**>(&b->h_counts), sizeof(unsigned long long) * kMaxVecGrid));
      p->bounds = b.release();
    }
    // on the device: no bound = -inf / +inf, so that the clamp is the identity on that side for every value
    std::vector<double> lo(size_t(n), -inf), hi(size_t(n), inf);
    for (int64_t i = 0; i < n; ++i) {
      if (lower && lower[i] > -dmax) lo[size_t(i)] = lower[i];
      if (upper && upper[i] < dmax) hi[size_t(i)] = upper[i];
    }
    BAL_TRY(p, up(s, p->d_lower, lo.data(), size_t(n)));
    BAL_TRY(p, up(s, p->d_upper, hi.data(), size_t(n)));
    HIP_TRY(s, hipStreamSynchronize(s->stream));   // (the uploads read vectors that go out of scope here)
  }
  if (p->bounds) {
    BalBoundsState* b = p->bounds;
    if (lower) b->lower.assign(lower, lower + n); else b->lower.clear();
    if (upper) b->upper.assign(upper, upper + n); else b->upper.clear();
    b->search = ls_search_options(o);
    b->reset_stats();
  }
  p->is_constrained = constrained;
  return 0;
} catch (const std::exception& ex) {
  (p ? p->err : g_create_error) = std::string("ceres_hip_bal_set_bounds: ") + ex.what();
  return CERES_HIP_E_INVALID;
}

int ceres_hip_bal_project(ceres_hip_bal* p, double* state, int64_t* num_moved) {
  auto refuse = [&](const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_project: " + why;
    return CERES_HIP_E_INVALID;
  };
  if (!p) return refuse("NULL problem handle");
  if (!state) return refuse("NULL state");
  if (!num_moved) return refuse("NULL num_moved");
  *num_moved = 0;
  if (!p->is_constrained) return 0;
  ceres_hip_solver* s = p->s;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, up(s, p->d_cand, state, size_t(p->n_a)));   // (d_cand: scratch of the trust-region loop between its calls)
  BAL_TRY(p, bal_bounds_project_device(p, p->d_cand, num_moved));
  BAL_TRY(p, down(s, state, p->d_cand, size_t(p->n_a)));
  return 0;
}

int ceres_hip_bal_bounds_stats(const ceres_hip_bal* p, int32_t* is_constrained, int32_t* num_line_search_steps, int32_t* num_function_evaluations,
                               int32_t* num_gradient_evaluations, double* line_search_seconds, int64_t* num_projected,
                               int32_t* line_search_iterations, int32_t* line_search_success, double* step_size) {
  if (!p) {
    g_create_error = "ceres_hip_bal_bounds_stats: NULL problem handle";
    return CERES_HIP_E_INVALID;
  }
  const BalBoundsState* b = p->bounds;
  const bool ran = b && b->ran_constrained;
  if (is_constrained) *is_constrained = ran ? 1 : 0;
  if (num_line_search_steps) *num_line_search_steps = ran ? b->num_line_search_steps : 0;
  if (num_function_evaluations) *num_function_evaluations = ran ? b->num_function_evaluations : 0;
  if (num_gradient_evaluations) *num_gradient_evaluations = ran ? b->num_gradient_evaluations : 0;
  if (line_search_seconds) *line_search_seconds = ran ? b->line_search_seconds : 0.0;
  if (num_projected) *num_projected = ran ? b->num_projected : 0;
  for (int i = 0; i < CERES_HIP_MAX_LOGGED_ITERATIONS; ++i) {
    if (line_search_iterations) line_search_iterations[i] = ran ? b->it_iterations[i] : -1;
    if (line_search_success) line_search_success[i] = ran ? b->it_success[i] : 0;
    if (step_size) step_size[i] = ran ? b->it_step[i] : 1.0;
  }
  return 0;
}

int ceres_hip_debug_bal_bounded_step(ceres_hip_bal* p, const double* state, const double* v, double t, double* trial_out, double* x_norm,
                                     double* step_norm, double* projected_max_norm) {
  auto refuse = [&](const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_debug_bal_bounded_step: " + why;
    return CERES_HIP_E_INVALID;
  };
  if (!p) return refuse("NULL problem handle");
  if (!state || !v || !trial_out || !x_norm || !step_norm || !projected_max_norm) return refuse("NULL argument");
  if (!p->is_constrained) return refuse("the handle is not constrained");
  ceres_hip_solver* s = p->s;
  hipStream_t st = s->stream;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, up(s, p->d_x, state, size_t(p->n_a)));
  BAL_TRY(p, up(s, p->d_step, v, size_t(p->n_t)));
  HIP_TRY(s, hipMemcpyAsync(p->d_cand, p->d_x, sizeof(double) * p->n_a, hipMemcpyDeviceToDevice, st));   // (constant blocks: copied)
  const BalBounds K = bal_bounds_args(p);
  PartialSums& P = p->parts;
  int nt = 0, ng = 0; double* parts = nullptr;
  BAL_TRY(p, bal_parts_room(p, 4 * kMaxVecGrid, &parts));
  HIP_TRY(s, LaunchBoundsTrialPoint(K, p->d_x, p->d_step, nullptr, nullptr, t, false, p->d_delta, p->d_cand, parts, &nt, st));
  const PartialSet xn = P.take(nt), sn = P.take(nt);
  P.take(nt); P.take(nt);   // (max |delta| and g . delta: not asked for)
  BAL_TRY(p, bal_parts_room(p, kMaxVecGrid, &parts));
  HIP_TRY(s, LaunchBoundsGradientMax(K, p->d_x, p->d_step, nullptr, parts, &ng, st));
  const PartialSet m = P.take(ng);
  HIP_TRY(s, hipMemcpyAsync(trial_out, p->d_cand, sizeof(double) * p->n_a, hipMemcpyDeviceToHost, st));   // (waited for by the collect)
  BAL_TRY(p, bal_parts_collect(p));
  *x_norm = std::sqrt(P.sum(xn)); *step_norm = std::sqrt(P.sum(sn)); *projected_max_norm = P.max(m);
  return 0;
}

}  // extern "C"
