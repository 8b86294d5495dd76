// Inner iterations of the BAL front end: Solver::Options::use_inner_iterations / inner_iteration_ordering /
// inner_iteration_tolerance (include/ceres/solver.h:686-715), bundle_adjuster's --inner_iterations and --blocks_for_inner_iterations
// (examples/bundle_adjuster.cc:83-88, 190-243).  Textually included by bal_frontend.inc.
//
//   the ordering          the four explicit kinds of bundle_adjuster.cc:190-243; AUTOMATIC = CoordinateDescentMinimizer::CreateOrdering
//                         (I/coordinate_descent_minimizer.cc:268-273): ComputeRecursiveIndependentSetOrdering
//                         (I/parameter_block_ordering.cc:101-123), then Reverse()
//   one pass              CoordinateDescentMinimizer::Minimize (I/coordinate_descent_minimizer.cc:130-211): the groups in increasing id,
//                         every block of a group solved on its own with all others fixed (kernels_inner.hip)
//   in the outer loop     TrustRegionMinimizer::DoInnerIterationsIfNeeded (I/trust_region_minimizer.cc:509-587), in
//                         ceres_hip_bal_minimize

// Points of at most this many observations take a lane each (kernels_inner.hip, kInnerPointLane), longer ones a wave: the lane form
// evaluates a point's observations one after the other, so a long point holds its whole wave back; a wave per point pays a 64-lane
// butterfly for each of its 10 sums per evaluation, which short points (a few observations: most lanes idle) cannot repay.
// CERES_HIP_INNER_FORM=lane / wave forces one form for every point (tests; cameras always take a wave).
constexpr int kInnerLaneMaxObservations = 32;

struct BalInner {
  int32_t kind = CERES_HIP_INNER_NONE;   // the ordering below is this kind's
  int32_t num_groups = 0;
  std::vector<int32_t> group;            // per block in state order (points, then cameras); -1: outside the ordering
  std::vector<int32_t> automatic;        // the AUTOMATIC ordering once computed (its graph pass is the expensive one), and its groups
  int32_t automatic_groups = 0;
  std::vector<int32_t> seg;              // per group g: [3 g, 3 g + 3] begin of its lane points, wave points, cameras in d_blocks
  int form_env = -1;                     // the CERES_HIP_INNER_FORM the segments were cut for
  // device lists (made once per handle)
  int32_t* d_blocks = nullptr;           // n_p + n_c: the kind's blocks by group, then form
  int32_t *d_pt_ptr = nullptr, *d_cam_ptr = nullptr, *d_cam_pt = nullptr, *d_iters = nullptr;
  double2* d_cam_obs = nullptr;
  // the camera and pixel of every entry of the points' lists: the handle's rows — or, with constant blocks, lists of their own over ALL
  // the caller's observations (a free block's loop sees its observations against constant blocks too, removed rows included)
  const int32_t* d_pt_cam = nullptr;
  const double2* d_pt_obs = nullptr;
  std::vector<int32_t> pt_count;         // observations per point
};

namespace {

// The group of every block (points 0 .. n_p - 1, then cameras) for one of the CERES_HIP_INNER_* kinds; returns the number of groups.
// AUTOMATIC: repeatedly the greedy independent set of IndependentSetOrdering (I/graph_algorithms.h:97-152) on the Hessian graph (blocks
// are vertices, joined when they share an observation) with the vertices taken so far removed, vertices visited by increasing degree in
// what is left; the sets' order reversed.  Ceres breaks ties of degree by the ParameterBlock* address (VertexTotalOrdering), which no
// caller can reproduce; here ties go by position in the state vector — points before cameras, then by index — which gives Ceres' groups
// whenever no two tied vertices are joined by an edge (every tie order then takes the same set).  On ordinary BAL data every camera sees
// more points than any point has cameras: cameras are group 0, points group 1.
int inner_ordering(int32_t nc, int32_t np, int64_t no, const int32_t* cam, const int32_t* pt, int32_t kind, std::vector<int32_t>& group) {
  const int64_t nv = int64_t(np) + nc;
  group.assign(static_cast<size_t>(nv), -1);
  switch (kind) {
    case CERES_HIP_INNER_CAMERAS: std::fill(group.begin() + np, group.end(), 0); return 1;
    case CERES_HIP_INNER_POINTS: std::fill(group.begin(), group.begin() + np, 0); return 1;
    case CERES_HIP_INNER_CAMERAS_POINTS:
      std::fill(group.begin(), group.begin() + np, 1); std::fill(group.begin() + np, group.end(), 0); return 2;
    case CERES_HIP_INNER_POINTS_CAMERAS:
      std::fill(group.begin(), group.begin() + np, 0); std::fill(group.begin() + np, group.end(), 1); return 2;
    default: break;
  }
  // the Hessian graph: unique (point, camera) pairs, adjacency in CSR over vertices v (v < np: point v; else camera v - np)
  std::vector<int64_t> pairs(static_cast<size_t>(no));
  for (int64_t i = 0; i < no; ++i) pairs[i] = int64_t(pt[i]) * nc + cam[i];
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  std::vector<int64_t> adj_ptr(static_cast<size_t>(nv) + 1, 0);
  for (int64_t e : pairs) { ++adj_ptr[e / nc + 1]; ++adj_ptr[np + e % nc + 1]; }
  for (int64_t v = 0; v < nv; ++v) adj_ptr[v + 1] += adj_ptr[v];
  std::vector<int32_t> adj(static_cast<size_t>(adj_ptr[nv]));
  {
    std::vector<int64_t> cur(adj_ptr.begin(), adj_ptr.end() - 1);
    for (int64_t e : pairs) {
      const int32_t q = int32_t(e / nc), c = int32_t(np + e % nc);
      adj[cur[q]++] = c;
      adj[cur[c]++] = q;
    }
  }
  std::vector<int64_t> degree(static_cast<size_t>(nv));
  for (int64_t v = 0; v < nv; ++v) degree[v] = adj_ptr[v + 1] - adj_ptr[v];
  std::vector<int32_t> round_of(static_cast<size_t>(nv), -1);
  std::vector<char> color(static_cast<size_t>(nv));
  std::vector<int64_t> count, order(static_cast<size_t>(nv));
  int64_t covered = 0;
  int rounds = 0;
  while (covered < nv) {
    // the remaining vertices by (degree, position): a counting sort, stable in position
    int64_t max_deg = 0, left = 0;
    for (int64_t v = 0; v < nv; ++v) if (round_of[v] < 0) max_deg = std::max(max_deg, degree[v]);
    count.assign(static_cast<size_t>(max_deg) + 2, 0);
    for (int64_t v = 0; v < nv; ++v) if (round_of[v] < 0) ++count[degree[v] + 1];
    for (int64_t d = 0; d <= max_deg; ++d) count[d + 1] += count[d];
    for (int64_t v = 0; v < nv; ++v) if (round_of[v] < 0) { order[count[degree[v]]++] = v; ++left; }
    for (int64_t i = 0; i < left; ++i) color[order[i]] = 0;   // white
    for (int64_t i = 0; i < left; ++i) {
      const int64_t v = order[i];
      if (color[v] != 0) continue;
      color[v] = 2;   // black: in the set
      for (int64_t k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) if (round_of[adj[k]] < 0 && color[adj[k]] != 2) color[adj[k]] = 1;   // grey
    }
    for (int64_t i = 0; i < left; ++i) {
      const int64_t v = order[i];
      if (color[v] != 2) continue;
      round_of[v] = rounds;
      ++covered;
    }
    for (int64_t i = 0; i < left; ++i) {   // RemoveVertex: the neighbours left behind lose an edge
      const int64_t v = order[i];
      if (round_of[v] != rounds) continue;
      for (int64_t k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) if (round_of[adj[k]] < 0) --degree[adj[k]];
    }
    ++rounds;
  }
  for (int64_t v = 0; v < nv; ++v) group[v] = rounds - 1 - round_of[v];   // ParameterBlockOrdering::Reverse
  return rounds;
}

int inner_form_env() {
  const char* e = getenv("CERES_HIP_INNER_FORM");
  if (!e) return -1;
  if (!strcmp(e, "lane")) return kInnerPointLane;
  if (!strcmp(e, "wave")) return kInnerPointWave;
  return -1;
}

// The handle's blocks by group, then form (lane points, wave points, cameras), uploaded; I.group / I.num_groups / I.pt_count are set
int bal_inner_blocks(ceres_hip_bal* p, BalInner& I, int form_env) {
  ceres_hip_solver* s = p->s;
  const int np = p->np, nc = p->nc;
  std::vector<int32_t> blocks;
  blocks.reserve(static_cast<size_t>(np) + nc);
  I.seg.assign(3 * static_cast<size_t>(I.num_groups) + 1, 0);
  for (int g = 0; g < I.num_groups; ++g) {
    for (int f = 0; f < 3; ++f) {
      I.seg[3 * g + f] = int32_t(blocks.size());
      if (f < 2) {
        for (int q = 0; q < np; ++q) {
          if (I.group[q] != g) continue;
          const bool lane = form_env >= 0 ? form_env == kInnerPointLane : I.pt_count[q] <= kInnerLaneMaxObservations;
          if (lane == (f == 0)) blocks.push_back(q);
        }
      } else {
        for (int c = 0; c < nc; ++c) if (I.group[np + c] == g) blocks.push_back(c);
      }
    }
  }
  I.seg[3 * static_cast<size_t>(I.num_groups)] = int32_t(blocks.size());
  if (!blocks.empty()) {
    HIP_TRY(s, hipMemcpyAsync(I.d_blocks, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
  }
  I.kind = p->inner_blocks;
  I.form_env = form_env;
  return 0;
}


// bal_inner_plan on a handle with constant blocks: the ordering is the reduced program's — the Hessian graph of the free blocks, constant
// blocks in no group — and the lists run over all of the caller's observations: points in observation order, stable; cameras likewise
int bal_inner_plan_reduced(ceres_hip_bal* p, BalInner& I, int form_env) {
  ceres_hip_solver* s = p->s;
  const int np = p->np, nc = p->nc;
  const int64_t na = int64_t(p->all_cam.size());
  if (!I.d_blocks) {
    const BalGrouping by_pt = bal_group_by(na, np, [&](int64_t i) { return p->all_pt[i]; }), by_cam = bal_group_by(na, nc, [&](int64_t i) { return p->all_cam[i]; });
    I.pt_count.resize(static_cast<size_t>(np));
    for (int q = 0; q < np; ++q) I.pt_count[q] = by_pt.ptr[q + 1] - by_pt.ptr[q];
    const std::vector<int32_t> pcam = bal_gather(by_pt, p->all_cam.data()), cpt = bal_gather(by_cam, p->all_pt.data());
    const std::vector<double> pobs = bal_gather(by_pt, p->all_obs.data(), 2), cobs = bal_gather(by_cam, p->all_obs.data(), 2);
    int32_t* pc = nullptr;
    double2* po = nullptr;
    TRY(dev_alloc(s, &I.d_blocks, static_cast<size_t>(np) + nc));
    TRY(dev_alloc(s, &I.d_iters, static_cast<size_t>(np) + nc));
    TRY(dev_upload(s, &I.d_pt_ptr, by_pt.ptr));
    TRY(dev_upload(s, &pc, pcam));
    TRY(dev_upload_pixels(s, &po, pobs));
    TRY(dev_upload(s, &I.d_cam_ptr, by_cam.ptr));
    TRY(dev_upload(s, &I.d_cam_pt, cpt));
    TRY(dev_upload_pixels(s, &I.d_cam_obs, cobs));
    I.d_pt_cam = pc; I.d_pt_obs = po;
    HIP_TRY(s, hipStreamSynchronize(s->stream));   // (the uploads read host vectors that go out of scope here)
  }
  if (I.kind != p->inner_blocks) {
    std::vector<int32_t> fcam, fpt;   // the reduced program's residual blocks that join two free blocks: the graph's edges
    for (int64_t i = 0; i < na; ++i)
      if (p->cam_col[p->all_cam[i]] >= 0 && p->pt_col[p->all_pt[i]] >= 0) { fcam.push_back(p->all_cam[i]); fpt.push_back(p->all_pt[i]); }
    I.num_groups = inner_ordering(nc, np, int64_t(fcam.size()), fcam.data(), fpt.data(), p->inner_blocks, I.group);
    for (int q = 0; q < np; ++q) if (p->pt_col[q] < 0) I.group[q] = -1;
    for (int c = 0; c < nc; ++c) if (p->cam_col[c] < 0) I.group[np + c] = -1;
  }
  return bal_inner_blocks(p, I, form_env);
}

// The handle's inner-iteration lists for p->inner_blocks (cached per kind and form switch)
int bal_inner_plan(ceres_hip_bal* p) {
  ceres_hip_solver* s = p->s;
  if (!p->inner) p->inner = new BalInner;
  BalInner& I = *p->inner;
  const int form_env = inner_form_env();
  if (I.kind == p->inner_blocks && I.form_env == form_env) return 0;
  const int np = p->np, nc = p->nc;
  if (p->has_const) return bal_inner_plan_reduced(p, I, form_env);
  const int64_t no = p->no;
  BalHostRows H;
  if (!I.d_blocks) {
    I.d_pt_cam = p->d_row_cam; I.d_pt_obs = p->d_row_obs;   // the lists every kind uses: point row ranges, the camera-major list, iteration counts
    // the fused path's camera-major list (point and pixel of every entry), where it covers the rows: its camera ranges are the plan's
    const std::vector<int32_t>& cp = s->plan.cam_ptr;
    const bool plans = p->d_cm_obs && p->d_cm_pt && cp.size() == static_cast<size_t>(nc) + 1 && cp[nc] == no;
    TRY(bal_fetch_rows(p, kRowCam | kRowPt | (plans ? 0 : kRowPixel), H));
    const BalGrouping by_pt = bal_group_by(no, np, [&](int64_t r) { return H.pt[r]; });   // rows are grouped by point
    I.pt_count.resize(static_cast<size_t>(np));
    for (int q = 0; q < np; ++q) I.pt_count[q] = by_pt.ptr[q + 1] - by_pt.ptr[q];
    TRY(dev_alloc(s, &I.d_blocks, static_cast<size_t>(np) + nc));
    TRY(dev_alloc(s, &I.d_iters, static_cast<size_t>(np) + nc));
    TRY(dev_upload(s, &I.d_pt_ptr, by_pt.ptr));
    BalGrouping by_cam;   // else: rows in camera order, stable
    std::vector<int32_t> cpt;
    std::vector<double> cobs;
    if (plans) {
      TRY(dev_upload(s, &I.d_cam_ptr, cp));
      I.d_cam_pt = p->d_cm_pt; I.d_cam_obs = p->d_cm_obs;
    } else {
      by_cam = bal_group_by(no, nc, [&](int64_t r) { return H.cam[r]; });
      cpt = bal_gather(by_cam, H.pt.data()); cobs = bal_gather(by_cam, H.pixel.data(), 2);
      TRY(dev_upload(s, &I.d_cam_ptr, by_cam.ptr));
      TRY(dev_upload(s, &I.d_cam_pt, cpt));
      TRY(dev_upload_pixels(s, &I.d_cam_obs, cobs));
    }
    HIP_TRY(s, hipStreamSynchronize(s->stream));   // (the uploads read host vectors that go out of scope here)
  }
  if (I.kind != p->inner_blocks) {
    if (p->inner_blocks == CERES_HIP_INNER_AUTOMATIC && !I.automatic.empty()) {
      I.group = I.automatic; I.num_groups = I.automatic_groups;
    } else {   // the ordering is a function of the structure alone: rebuilt from the rows (camera, point per row)
      if (H.cam.empty()) TRY(bal_fetch_rows(p, kRowCam | kRowPt, H));
      I.num_groups = inner_ordering(nc, np, no, H.cam.data(), H.pt.data(), p->inner_blocks, I.group);
      if (p->inner_blocks == CERES_HIP_INNER_AUTOMATIC) { I.automatic = I.group; I.automatic_groups = I.num_groups; }
    }
  }
  return bal_inner_blocks(p, I, form_env);
}

// One CoordinateDescentMinimizer::Minimize pass at d_state (in place), enqueued on the solver's stream; iteration counts in I.d_iters.
int bal_inner_pass(ceres_hip_bal* p, double* d_state) {
  ceres_hip_solver* s = p->s;
  TRY(bal_inner_plan(p));
  const BalInner& I = *p->inner;
  for (int g = 0; g < I.num_groups; ++g) {
    for (int f = 0; f < 3; ++f) {
      InnerArgs A;
      A.state = d_state; A.cam_base = 3 * int64_t(p->np); A.loss = p->loss;
      A.blocks = I.d_blocks + I.seg[3 * g + f];
      A.n_blocks = I.seg[3 * g + f + 1] - I.seg[3 * g + f];
      if (f < 2) {
        A.ptr = I.d_pt_ptr; A.other = I.d_pt_cam; A.obs = I.d_pt_obs; A.iterations = I.d_iters;
      } else {
        A.ptr = I.d_cam_ptr; A.other = I.d_cam_pt; A.obs = I.d_cam_obs; A.iterations = I.d_iters + p->np;
      }
      HIP_TRY(s, LaunchInnerBlocks(A, f == 0 ? kInnerPointLane : f == 1 ? kInnerPointWave : kInnerCameraWave, s->stream));
    }
  }
  return 0;
}

}  // namespace

void bal_inner_free(ceres_hip_bal* p) {   // (device lists are the solver's allocations: freed with it)
  delete p->inner;
  p->inner = nullptr;
}

extern "C" {

int ceres_hip_debug_inner_iteration_ordering(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                             const int32_t* point_index, int32_t blocks, int32_t* group_of_block, int32_t* num_groups) try {
  if (num_cameras <= 0 || num_points <= 0 || num_observations <= 0 || !camera_index || !point_index || !group_of_block || !num_groups ||
      blocks < CERES_HIP_INNER_AUTOMATIC || blocks > CERES_HIP_INNER_POINTS_CAMERAS)
    return CERES_HIP_E_INVALID;
  for (int64_t i = 0; i < num_observations; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= num_cameras || point_index[i] < 0 || point_index[i] >= num_points) return CERES_HIP_E_INVALID;
  std::vector<int32_t> group;
  *num_groups = inner_ordering(num_cameras, num_points, num_observations, camera_index, point_index, blocks, group);
  memcpy(group_of_block, group.data(), sizeof(int32_t) * group.size());
  return 0;
} catch (const std::exception&) {
  return CERES_HIP_E_INVALID;
}

int ceres_hip_bal_set_inner_iterations(ceres_hip_bal* p, int32_t blocks, double tolerance) {
  auto invalid = [&](const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_set_inner_iterations: " + why;
    return CERES_HIP_E_INVALID;
  };
  if (!p) return invalid("NULL problem handle");
  if (blocks < CERES_HIP_INNER_NONE || blocks > CERES_HIP_INNER_POINTS_CAMERAS) return invalid("unknown blocks " + std::to_string(blocks));
  if (!std::isfinite(tolerance) || tolerance < 0.0) return invalid("tolerance must be finite and >= 0");   // (solver.cc:423-424)
  if (blocks != CERES_HIP_INNER_NONE && p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS) {   // (kernels_inner.hip: angle-axis blocks)
    p->err = "ceres_hip_bal_set_inner_iterations: inner iterations are not supported with quaternion cameras";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (blocks != CERES_HIP_INNER_NONE && p->n_groups) {   // (kernels_inner.hip: every camera block owns its nine coordinates)
    p->err = "ceres_hip_bal_set_inner_iterations: inner iterations are not supported on handles with shared intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (blocks != CERES_HIP_INNER_NONE && p->intrinsics_mask) {   // (kernels_inner.hip: camera blocks of nine free coordinates)
    p->err = "ceres_hip_bal_set_inner_iterations: inner iterations are not supported on handles with fixed intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  p->inner_blocks = blocks;
  p->inner_tolerance = tolerance;
  return 0;
}

int ceres_hip_bal_inner_iterate(ceres_hip_bal* p, double* state, double* cost_before, double* cost_after, int32_t* block_iterations) try {
  if (!p) return CERES_HIP_E_INVALID;
  ceres_hip_solver* s = p->s;
  auto refuse = [&](int code, const char* why) {
    p->err = std::string("ceres_hip_bal_inner_iterate: ") + why;
    return code;
  };
  if (!state || !cost_before || !cost_after) return refuse(CERES_HIP_E_INVALID, "NULL state or cost");
  if (p->camera_model != CERES_HIP_CAMERA_ANGLE_AXIS) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported with quaternion cameras");
  if (p->intrinsics_mask) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with fixed intrinsics");
  if (p->n_groups) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with shared intrinsics");
  if (p->is_constrained) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with bounds");   // (the passes do not project)
  if (p->inner_blocks == CERES_HIP_INNER_NONE) return refuse(CERES_HIP_E_INVALID, "no inner iterations set (ceres_hip_bal_set_inner_iterations)");
  if (s->world > 1) return refuse(CERES_HIP_E_UNSUPPORTED, "not on sharded handles");
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, up(s, p->d_cand, state, static_cast<size_t>(p->n_a)));
  BAL_TRY(p, bal_evaluate_device(p, p->d_cand, false, nullptr, nullptr, cost_before));
  BAL_TRY(p, bal_inner_pass(p, p->d_cand));
  BAL_TRY(p, bal_evaluate_device(p, p->d_cand, false, nullptr, nullptr, cost_after));
  BAL_TRY(p, down(s, state, p->d_cand, static_cast<size_t>(p->n_a)));
  if (block_iterations) {
    const BalInner& I = *p->inner;
    const size_t nb = static_cast<size_t>(p->np) + p->nc;
    HIP_TRY(s, hipMemcpy(block_iterations, I.d_iters, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < nb; ++v) if (I.group[v] < 0) block_iterations[v] = -1;
  }
  return 0;
} catch (const std::exception& ex) {
  p->err = std::string("ceres_hip_bal_inner_iterate: ") + ex.what();
  return CERES_HIP_E_INVALID;
}

int ceres_hip_bal_inner_iteration_stats(const ceres_hip_bal* p, int32_t* num_inner_iteration_steps, double* inner_iteration_seconds,
                                        int32_t* num_groups) {
  if (!p || !num_inner_iteration_steps || !inner_iteration_seconds || !num_groups) return CERES_HIP_E_INVALID;
  *num_inner_iteration_steps = p->inner_steps;
  *inner_iteration_seconds = p->inner_seconds;
  *num_groups = p->inner_groups_used;
  return 0;
}

}  // extern "C"
