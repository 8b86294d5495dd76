// C++ host-side mirror of the BAL front end of include/ceres_hip.h: what
// examples/bal_problem.{h,cc} (the reader), ceres::internal::Evaluator (Evaluate) and
// TrustRegionMinimizer::Minimize are to bundle_adjuster, over the C ABI.  Header-only, no Ceres.
#ifndef CERES_HIP_HOST_BAL_PROBLEM_H_
#define CERES_HIP_HOST_BAL_PROBLEM_H_

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "ceres_hip.h"
#include "hip_linear_solver.h"

namespace ceres_hip {

// AngleAxisToQuaternion / QuaternionToAngleAxis (include/ceres/rotation.h), quaternion [w x y z]
inline void AngleAxisToQuaternion(const double* a, double* q) {
  const double theta = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  double k = 0.5;
  q[0] = 1.0;
  if (theta != 0.0) { k = std::sin(0.5 * theta) / theta; q[0] = std::cos(0.5 * theta); }
  for (int i = 0; i < 3; ++i) q[1 + i] = a[i] * k;
}
inline void QuaternionToAngleAxis(const double* q, double* a) {
  const double sin_theta = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double k = 2.0;
  if (sin_theta != 0.0) {
    const double sign = std::copysign(1.0, q[0]);   // (theta > pi / 2: the angle 2 theta - 2 pi, within [-pi, pi])
    k = 2.0 * std::atan2(sign * sin_theta, sign * q[0]) / sin_theta;
  }
  for (int i = 0; i < 3; ++i) a[i] = q[1 + i] * k;
}

// examples/bal_problem.cc:75-135 — "cameras points observations", one "camera point x y" line per
// observation, then 9 doubles per camera and 3 per point.
struct BalData {
  int num_cameras = 0, num_points = 0;
  std::vector<int32_t> camera_index, point_index;
  std::vector<double> observations;  // 2 per observation
  std::vector<double> parameters;    // file order: cameras, then points

  static BalData Read(const std::string& filename) {
    BalData d;
    FILE* f = std::fopen(filename.c_str(), "r");
    if (!f) throw std::runtime_error("cannot open " + filename);
    long long n_obs = 0;
    bool ok = std::fscanf(f, "%d %d %lld", &d.num_cameras, &d.num_points, &n_obs) == 3 && n_obs >= 0;
    if (ok) {
      d.camera_index.resize(n_obs); d.point_index.resize(n_obs); d.observations.resize(2 * n_obs);
      for (long long i = 0; ok && i < n_obs; ++i)
        ok = std::fscanf(f, "%d %d %lf %lf", &d.camera_index[i], &d.point_index[i], &d.observations[2 * i],
                         &d.observations[2 * i + 1]) == 4;
      d.parameters.resize(9 * size_t(d.num_cameras) + 3 * size_t(d.num_points));
      for (size_t i = 0; ok && i < d.parameters.size(); ++i) ok = std::fscanf(f, "%lf", &d.parameters[i]) == 1;
    }
    std::fclose(f);
    if (!ok) throw std::runtime_error(filename + " is not a BAL file");
    return d;
  }
  // state of the reduced, Schur-ordered program: points first, then cameras — 10 doubles per camera for the quaternion camera models
  // (CERES_HIP_CAMERA_*), converted as BALProblem(filename, use_quaternions = true) does (examples/bal_problem.cc:110-131)
  std::vector<double> State(int camera_model = CERES_HIP_CAMERA_ANGLE_AXIS) const {
    std::vector<double> x(parameters.begin() + 9 * size_t(num_cameras), parameters.end());
    if (camera_model == CERES_HIP_CAMERA_ANGLE_AXIS) {
      x.insert(x.end(), parameters.begin(), parameters.begin() + 9 * size_t(num_cameras));
      return x;
    }
    for (int c = 0; c < num_cameras; ++c) {
      const double* cam = parameters.data() + 9 * size_t(c);
      double q[4];
      AngleAxisToQuaternion(cam, q);
      x.insert(x.end(), q, q + 4);
      x.insert(x.end(), cam + 3, cam + 9);
    }
    return x;
  }
  // the cameras of a state back in BAL order (BALProblem::WriteToFile, examples/bal_problem.cc:157-160): 9 per camera, then 3 per point
  std::vector<double> Parameters(const std::vector<double>& state, int camera_model = CERES_HIP_CAMERA_ANGLE_AXIS) const {
    const size_t np3 = 3 * size_t(num_points), cs = camera_model == CERES_HIP_CAMERA_ANGLE_AXIS ? 9 : 10;
    std::vector<double> p(9 * size_t(num_cameras) + np3);
    for (int c = 0; c < num_cameras; ++c) {
      const double* cam = state.data() + np3 + cs * c;
      double* out = p.data() + 9 * size_t(c);
      if (cs == 9) { for (int i = 0; i < 9; ++i) out[i] = cam[i]; continue; }
      QuaternionToAngleAxis(cam, out);
      for (int i = 0; i < 6; ++i) out[3 + i] = cam[4 + i];
    }
    for (size_t i = 0; i < np3; ++i) p[9 * size_t(num_cameras) + i] = state[i];
    return p;
  }
};

class HipBalProblem {
 public:
  // camera_model: CERES_HIP_CAMERA_* (bundle_adjuster --use_quaternions [--use_manifolds]: QUATERNION [_MANIFOLD]); BalData::State(camera_model)
  // is the matching state
  // camera_is_constant / point_is_constant (Problem::SetParameterBlockConstant; ParameterBlock::IsConstant() per block): empty = none
  // constant, else one entry per camera / point, non-zero = constant.  With any entry the handle is the reduced program
  // (ceres_hip_bal_create_with_constant_blocks): the state keeps its full layout, the gradient and the Jacobian's columns are the free
  // blocks' (ReducedSizes); without, the entry point this class always used.
  // camera_coordinate_is_constant (SubsetManifold(9, ...) on every camera block): empty = none, else nine entries, non-zero = constant
  // on all cameras — only the intrinsics, coordinates 6 .. 8, of the angle-axis camera (ceres_hip_bal_create_with_fixed_intrinsics: the
  // state stays nine per camera, a camera is CameraTangentSize() wide in the gradient and the Jacobian; what such a handle refuses is
  // listed in include/ceres_hip.h).
  // camera_group (shared intrinsics: one [f k1 k2] parameter block per group beside a 6-wide pose block per camera, as
  // examples/libmv_bundle_adjuster.cc:697-728 adds its residual blocks): empty = none, else one group id in [0, num_groups) per camera,
  // every id used; angle-axis cameras only, not together with constant points or a coordinate mask
  // (ceres_hip_bal_create_with_shared_intrinsics: the state stays nine per camera, a group's intrinsics bit-identical in its cameras;
  // the gradient is [points | free cameras' poses | groups], CameraTangentSize() is 6; camera_is_constant holds poses constant).
  HipBalProblem(const LinearSolver::Options& options, const BalData& d, int camera_model = CERES_HIP_CAMERA_ANGLE_AXIS,
                const std::vector<uint8_t>& camera_is_constant = {}, const std::vector<uint8_t>& point_is_constant = {},
                const std::vector<uint8_t>& camera_coordinate_is_constant = {}, const std::vector<int32_t>& camera_group = {}) {
    if (!camera_group.empty() && (camera_group.size() != size_t(d.num_cameras) || !point_is_constant.empty() || !camera_coordinate_is_constant.empty()))
      throw std::invalid_argument("HipBalProblem: camera_group has one entry per camera and excludes constant points and a coordinate mask");
    if ((!camera_is_constant.empty() && camera_is_constant.size() != size_t(d.num_cameras)) ||
        (!point_is_constant.empty() && point_is_constant.size() != size_t(d.num_points)))
      throw std::invalid_argument("HipBalProblem: a constant-block mask has one entry per block");
    const size_t cs = camera_model == CERES_HIP_CAMERA_ANGLE_AXIS ? 9 : 10;
    if (!camera_coordinate_is_constant.empty() && camera_coordinate_is_constant.size() != cs)
      throw std::invalid_argument("HipBalProblem: the camera coordinate mask has one entry per camera state double");
    camera_tangent_size_ = camera_model == CERES_HIP_CAMERA_QUATERNION ? 10 : 9;
    for (uint8_t m : camera_coordinate_is_constant) camera_tangent_size_ -= m != 0;
    ceres_hip_options o{};
    o.solver_type = options.type;
    o.preconditioner_type = options.preconditioner_type;
    o.min_num_iterations = options.min_num_iterations;
    o.max_num_iterations = options.max_num_iterations;
    o.residual_reset_period = options.residual_reset_period;
    o.device = options.device;
    if (!camera_group.empty()) {
      for (int32_t g : camera_group) num_intrinsics_groups_ = std::max(num_intrinsics_groups_, g + 1);
      camera_tangent_size_ = 6;
      handle_ = ceres_hip_bal_create_with_shared_intrinsics(&o, camera_model, d.num_cameras, d.num_points, int64_t(d.camera_index.size()),
                                                            d.camera_index.data(), d.point_index.data(), d.observations.data(),
                                                            camera_is_constant.empty() ? nullptr : camera_is_constant.data(),
                                                            camera_group.data(), num_intrinsics_groups_);
    } else if (!camera_coordinate_is_constant.empty())
      handle_ = ceres_hip_bal_create_with_fixed_intrinsics(&o, camera_model, d.num_cameras, d.num_points, int64_t(d.camera_index.size()),
                                                           d.camera_index.data(), d.point_index.data(), d.observations.data(),
                                                           camera_is_constant.empty() ? nullptr : camera_is_constant.data(),
                                                           point_is_constant.empty() ? nullptr : point_is_constant.data(),
                                                           camera_coordinate_is_constant.data());
    else if (camera_is_constant.empty() && point_is_constant.empty())
      handle_ = ceres_hip_bal_create_with_camera(&o, camera_model, d.num_cameras, d.num_points, int64_t(d.camera_index.size()),
                                                 d.camera_index.data(), d.point_index.data(), d.observations.data());
    else
      handle_ = ceres_hip_bal_create_with_constant_blocks(&o, camera_model, d.num_cameras, d.num_points, int64_t(d.camera_index.size()),
                                                          d.camera_index.data(), d.point_index.data(), d.observations.data(),
                                                          camera_is_constant.empty() ? nullptr : camera_is_constant.data(),
                                                          point_is_constant.empty() ? nullptr : point_is_constant.data());
    if (!handle_) throw std::runtime_error(std::string(ceres_hip_bal_last_error(nullptr)));
    num_blocks_ = int64_t(d.num_points) + d.num_cameras;
    ceres_hip_bal_sizes(handle_, &num_parameters_, &num_residuals_, &num_jacobian_values_);
    ceres_hip_bal_num_effective_parameters(handle_, &num_effective_parameters_);
  }
  ~HipBalProblem() { ceres_hip_bal_destroy(handle_); }
  HipBalProblem(const HipBalProblem&) = delete;
  HipBalProblem& operator=(const HipBalProblem&) = delete;

  int NumParameters() const { return int(num_parameters_); }   // Evaluator::NumParameters, I/evaluator.h:151
  int NumResiduals() const { return int(num_residuals_); }     // Evaluator::NumResiduals, :158
  int NumEffectiveParameters() const { return int(num_effective_parameters_); }   // Evaluator::NumEffectiveParameters: the gradient's length
  int CameraTangentSize() const { return camera_tangent_size_; }   // Jacobian columns per free camera (Manifold::TangentSize of the block)
  int NumIntrinsicsGroups() const { return num_intrinsics_groups_; }   // shared intrinsics: the 3-wide blocks behind the poses (0: none)
  // The blocks Covariance numbers: points, cameras and, with shared intrinsics, the groups behind them
  int64_t NumCovarianceBlocks() const { return num_blocks_ + num_intrinsics_groups_; }
  // What Program::RemoveFixedBlocks left: rows kept, rows with an E cell (they come first), rows removed (both blocks constant), free
  // cameras, free points; any pointer may be null
  bool ReducedSizes(int64_t* num_rows, int64_t* num_rows_e, int64_t* num_rows_removed, int32_t* num_free_cameras, int32_t* num_free_points) const {
    return ceres_hip_bal_reduced_sizes(handle_, num_rows, num_rows_e, num_rows_removed, num_free_cameras, num_free_points) == CERES_HIP_OK;
  }
  // Solver::Summary::fixed_cost at state: the removed rows' cost with the loss in force (Minimize's costs include it)
  bool FixedCost(const double* state, double* fixed_cost) { return ceres_hip_bal_fixed_cost(handle_, state, fixed_cost) == CERES_HIP_OK; }
  // row_observation[r] = the observation of kept row r (NumResiduals() / 2 entries)
  std::vector<int32_t> RowOrder() const {
    std::vector<int32_t> rows(size_t(num_residuals_ / 2));
    if (ceres_hip_bal_get_row_order(handle_, rows.data()) != CERES_HIP_OK) throw std::runtime_error("ceres_hip_bal_get_row_order");
    return rows;
  }
  // The loss of every residual block, ScaledLoss(loss, scale): loss_type CERES_HIP_LOSS_*, a / b its constructor arguments
  // (bundle_adjuster --robustify: SetLoss(CERES_HIP_LOSS_HUBER, 1.0)).  Applies to the later Evaluate / Minimize calls.
  void SetLoss(int loss_type, double a, double b = 1.0, double scale = 1.0) {
    if (ceres_hip_bal_set_loss(handle_, loss_type, a, b, scale) != CERES_HIP_OK)
      throw std::invalid_argument(std::string(ceres_hip_bal_last_error(handle_)));
  }
  // Inner iterations (Solver::Options::use_inner_iterations / inner_iteration_ordering / inner_iteration_tolerance): blocks
  // CERES_HIP_INNER_* (bundle_adjuster --blocks_for_inner_iterations), NONE switches them off.  Applies to the later Minimize calls.
  void SetInnerIterations(int blocks, double tolerance = 1e-3) {
    if (ceres_hip_bal_set_inner_iterations(handle_, blocks, tolerance) != CERES_HIP_OK)
      throw std::invalid_argument(std::string(ceres_hip_bal_last_error(handle_)));
  }
  // Trust-region strategy (Solver::Options::trust_region_strategy_type, dogleg_type; bundle_adjuster --trust_region_strategy --dogleg):
  // CERES_HIP_LEVENBERG_MARQUARDT, or CERES_HIP_DOGLEG with CERES_HIP_TRADITIONAL_DOGLEG / CERES_HIP_SUBSPACE_DOGLEG.  DOGLEG needs a
  // DENSE_SCHUR problem (Ceres refuses it with iterative solvers).  Applies to the later Minimize calls.
  void SetTrustRegionStrategy(int strategy, int dogleg_type = CERES_HIP_TRADITIONAL_DOGLEG) {
    if (ceres_hip_bal_set_trust_region_strategy(handle_, strategy, dogleg_type) != CERES_HIP_OK)
      throw std::invalid_argument(std::string(ceres_hip_bal_last_error(handle_)));
  }
  // One coordinate-descent pass (CoordinateDescentMinimizer::Minimize) at state, in / out; block_iterations may be null
  bool InnerIterate(double* state, double* cost_before, double* cost_after, int32_t* block_iterations = nullptr) {
    return ceres_hip_bal_inner_iterate(handle_, state, cost_before, cost_after, block_iterations) == CERES_HIP_OK;
  }
  // Of the last Minimize: Solver::Summary::num_inner_iteration_steps, inner_iteration_time_in_seconds; groups of the ordering
  bool InnerIterationStats(int32_t* num_inner_iteration_steps, double* inner_iteration_seconds, int32_t* num_groups) const {
    return ceres_hip_bal_inner_iteration_stats(handle_, num_inner_iteration_steps, inner_iteration_seconds, num_groups) == CERES_HIP_OK;
  }
  // Evaluator::Evaluate (I/evaluator.h:116-124); residuals / gradient / jacobian values may be null
  bool Evaluate(const double* state, double* cost, double* residuals, double* gradient, double* jacobian_values) {
    return ceres_hip_bal_evaluate(handle_, state, cost, residuals, gradient, jacobian_values) == CERES_HIP_OK;
  }
  // TrustRegionMinimizer::Minimize; state in/out
  ceres_hip_minimizer_summary Minimize(const ceres_hip_minimizer_options& options, double* state) {
    ceres_hip_minimizer_summary s{};
    if (ceres_hip_bal_minimize(handle_, &options, state, &s) != CERES_HIP_OK)
      throw std::runtime_error(std::string("ceres_hip_bal_minimize: ") + ceres_hip_bal_last_error(handle_));
    return s;
  }
  // Evaluator::Evaluate(state, cost, nullptr, gradient, nullptr) without a Jacobian in memory; gradient (NumEffectiveParameters()
  // doubles) may be null: the cost alone
  bool EvaluateGradient(const double* state, double* cost, double* gradient) {
    return ceres_hip_bal_evaluate_gradient(handle_, state, cost, gradient) == CERES_HIP_OK;
  }
  // LineSearchMinimizer::Minimize (Solver::Options::minimizer_type = LINE_SEARCH; bundle_adjuster --line_search); state in/out.
  // Options from ceres_hip_line_search_default_options; an invalid combination throws with Ceres' message.
  ceres_hip_line_search_summary MinimizeLineSearch(const ceres_hip_line_search_options& options, double* state) {
    ceres_hip_line_search_summary s{};
    if (ceres_hip_bal_minimize_line_search(handle_, &options, state, &s) != CERES_HIP_OK)
      throw std::runtime_error(std::string(ceres_hip_bal_last_error(handle_)));
    return s;
  }
  // ceres::Covariance::Compute + GetCovarianceBlockInTangentSpace for the (a, b) block pairs, numbered in state order (point q is q,
  // camera c is num_points + c): blocks_out = the dim(a) x dim(b) row-major blocks back to back (3 per point, 9 or 10 per camera; zeros
  // for a pair with a constant block).  With camera_group: camera c's block is its 6-wide POSE and group g is block
  // num_points + num_cameras + g (3 wide, never constant) — NumCovarianceBlocks() blocks in all.  DENSE_SCHUR handles only.  Options from ceres_hip_covariance_default_options.  A refused call
  // throws; a rank-deficient problem returns with termination_type = CERES_HIP_FAILURE and its message, blocks_out untouched.
  ceres_hip_covariance_summary Covariance(const ceres_hip_covariance_options& options, const double* state,
                                          const std::vector<int32_t>& block_a, const std::vector<int32_t>& block_b, double* blocks_out) {
    if (block_a.size() != block_b.size()) throw std::invalid_argument("HipBalProblem::Covariance: block_a and block_b differ in length");
    ceres_hip_covariance_summary s{};
    if (ceres_hip_bal_covariance(handle_, &options, state, int64_t(block_a.size()), block_a.data(), block_b.data(), blocks_out, &s) != CERES_HIP_OK)
      throw std::runtime_error(std::string(ceres_hip_bal_last_error(handle_)));
    return s;
  }
  // Problem::SetParameterLowerBound / SetParameterUpperBound for every coordinate of the state at once (NumParameters() doubles each,
  // an empty vector: no bound on that side, both empty: clears).  line_search_options: the fields of the projected search Minimize then
  // runs (Solver::Options::line_search_interpolation_type, min_line_search_step_size, ...), null: the defaults.  A refused call throws
  // with Ceres' message (an infeasible bound, an option out of range).  Applies to the later Minimize calls.
  void SetBounds(const std::vector<double>& lower, const std::vector<double>& upper,
                 const ceres_hip_line_search_options* line_search_options = nullptr) {
    if ((!lower.empty() && int64_t(lower.size()) != num_parameters_) || (!upper.empty() && int64_t(upper.size()) != num_parameters_))
      throw std::invalid_argument("HipBalProblem::SetBounds: a bounds vector must have NumParameters() entries or none");
    if (ceres_hip_bal_set_bounds(handle_, lower.empty() ? nullptr : lower.data(), upper.empty() ? nullptr : upper.data(), line_search_options) !=
        CERES_HIP_OK)
      throw std::invalid_argument(std::string(ceres_hip_bal_last_error(handle_)));
  }
  // Program::Plus(state, 0): state clamped to the bounds on the free blocks, in / out; *num_moved: the coordinates changed
  bool Project(double* state, int64_t* num_moved) { return ceres_hip_bal_project(handle_, state, num_moved) == CERES_HIP_OK; }
  // Of the last Minimize: Solver::Summary::is_constrained, num_line_search_steps, the searches' evaluations and seconds, the
  // coordinates the initial projection moved; per logged iteration (arrays of CERES_HIP_MAX_LOGGED_ITERATIONS, may be null) the
  // search's iterations (-1: none ran), success and step size.  Any pointer may be null.
  bool BoundsStats(int32_t* is_constrained, int32_t* num_line_search_steps, int32_t* num_function_evaluations, int32_t* num_gradient_evaluations,
                   double* line_search_seconds, int64_t* num_projected, int32_t* line_search_iterations = nullptr,
                   int32_t* line_search_success = nullptr, double* step_size = nullptr) const {
    return ceres_hip_bal_bounds_stats(handle_, is_constrained, num_line_search_steps, num_function_evaluations, num_gradient_evaluations,
                                      line_search_seconds, num_projected, line_search_iterations, line_search_success, step_size) == CERES_HIP_OK;
  }

 private:
  ceres_hip_bal* handle_ = nullptr;
  int64_t num_parameters_ = 0, num_residuals_ = 0, num_jacobian_values_ = 0, num_effective_parameters_ = 0;
  int camera_tangent_size_ = 9;
  int32_t num_intrinsics_groups_ = 0;
  int64_t num_blocks_ = 0;   // points + cameras
};

}  // namespace ceres_hip
#endif
