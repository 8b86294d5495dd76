// Constant parameter blocks of the BAL front end: Problem::SetParameterBlockConstant, and what Program::RemoveFixedBlocks
// (I/program.cc:309-410) and the Schur ordering (I/reorder_program.cc:278-340) make of the problem.  Host code only; textually included
// by bal_frontend.inc (ceres_hip_bal_create_with_constant_blocks builds its handle from it, ceres_hip_debug_bal_reduce exposes it).

struct BalReduction {
  int32_t num_free_cameras = 0, num_free_points = 0;
  int64_t num_rows_e = 0;                    // rows with an E cell (a free point): they come first
  std::vector<int32_t> row_obs;              // kept row -> observation
  std::vector<int32_t> removed_obs;          // observations whose camera and point are both constant, in observation order
  std::vector<int32_t> camera_column, point_column;   // index among the free blocks, -1: constant
};

namespace {

// "" or why the problem is refused.  A residual block whose parameter blocks are all constant is removed; the others keep the project's
// order — grouped by point, stable in observation order — with the rows of constant points behind all rows that have an E cell.
std::string bal_reduce(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index, const int32_t* point_index,
                       const uint8_t* camera_is_constant, const uint8_t* point_is_constant, BalReduction& R) {
  if (num_cameras <= 0 || num_points <= 0 || num_observations <= 0 || !camera_index || !point_index) return "bad arguments";
  if (num_observations > int64_t(INT32_MAX)) return "more than 2^31 observations";
  for (int64_t i = 0; i < num_observations; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= num_cameras || point_index[i] < 0 || point_index[i] >= num_points)
      return "observation index out of range";
  R.camera_column.assign(size_t(num_cameras), -1);
  R.point_column.assign(size_t(num_points), -1);
  R.num_free_cameras = R.num_free_points = 0;
  for (int c = 0; c < num_cameras; ++c) if (!(camera_is_constant && camera_is_constant[c])) R.camera_column[c] = R.num_free_cameras++;
  for (int q = 0; q < num_points; ++q) if (!(point_is_constant && point_is_constant[q])) R.point_column[q] = R.num_free_points++;
  if (R.num_free_cameras == 0)
    return "every camera is constant: no F block is left (Ceres switches the linear solver there, LinearSolverForZeroEBlocks and its "
           "kin; this front end does not)";
  if (R.num_free_points == 0)
    return "every point is constant: no E block is left (Ceres switches the linear solver there, LinearSolverForZeroEBlocks; this front "
           "end does not)";
  R.row_obs.clear(); R.removed_obs.clear();
  std::vector<int32_t> tail;
  for (int64_t i = 0; i < num_observations; ++i) {
    const bool cf = R.camera_column[camera_index[i]] >= 0, pf = R.point_column[point_index[i]] >= 0;
    if (pf) R.row_obs.push_back(int32_t(i));
    else if (cf) tail.push_back(int32_t(i));
    else R.removed_obs.push_back(int32_t(i));
  }
  std::stable_sort(R.row_obs.begin(), R.row_obs.end(), [&](int32_t a, int32_t b) { return point_index[a] < point_index[b]; });
  R.num_rows_e = int64_t(R.row_obs.size());
  R.row_obs.insert(R.row_obs.end(), tail.begin(), tail.end());
  if (R.row_obs.empty()) return "no residual block is left: every observation has a constant camera and a constant point";
  return "";
}

}  // namespace

extern "C" int ceres_hip_debug_bal_reduce(int32_t num_cameras, int32_t num_points, int64_t num_observations, const int32_t* camera_index,
                                          const int32_t* point_index, const uint8_t* camera_is_constant, const uint8_t* point_is_constant,
                                          int64_t* num_rows, int64_t* num_rows_e, int32_t* row_observation, int32_t* camera_column,
                                          int32_t* point_column) try {
  BalReduction R;
  const std::string why = bal_reduce(num_cameras, num_points, num_observations, camera_index, point_index, camera_is_constant, point_is_constant, R);
  if (!why.empty()) {
    g_create_error = "ceres_hip_debug_bal_reduce: " + why;
    return CERES_HIP_E_INVALID;
  }
  if (num_rows) *num_rows = int64_t(R.row_obs.size());
  if (num_rows_e) *num_rows_e = R.num_rows_e;
  if (row_observation) memcpy(row_observation, R.row_obs.data(), sizeof(int32_t) * R.row_obs.size());
  if (camera_column) memcpy(camera_column, R.camera_column.data(), sizeof(int32_t) * R.camera_column.size());
  if (point_column) memcpy(point_column, R.point_column.data(), sizeof(int32_t) * R.point_column.size());
  return 0;
} catch (const std::exception& ex) {
  g_create_error = std::string("ceres_hip_debug_bal_reduce: ") + ex.what();
  return CERES_HIP_E_INVALID;
}
