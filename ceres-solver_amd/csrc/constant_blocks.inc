// Constant parameter blocks of the BAL front end: Problem::SetParameterBlockConstant, and what Program::RemoveFixedBlocks
// (I/program.cc:309-410) and the Schur ordering (I/reorder_program.cc:278-340) make of the problem: BalReduction and bal_reduce of
// bal_layout.h, which every handle is laid out from; ceres_hip_debug_bal_reduce exposes them.  Textually included by bal_frontend.inc.

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
