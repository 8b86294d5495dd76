// The line search minimizer of the BAL front end (textually included by bal_frontend.inc, after dogleg.inc whose polynomial root finder
// it shares).  A restatement, statement by statement, of
//
//   LineSearchMinimizer::Minimize                      I/line_search_minimizer.cc:67-479
//   ArmijoLineSearch / WolfeLineSearch (bracket, zoom) I/line_search.cc:210-880
//   SteepestDescent / NonlinearConjugateGradient / LBFGS   I/line_search_direction.cc:45-143
//   LowRankInverseHessian                              I/low_rank_inverse_hessian.cc:87-177 (on the device: kernels_line_search.hip)
//   FindInterpolatingPolynomial / MinimizePolynomial   I/polynomial.cc:277-392
//   LineSearchOptionsAreValid                          I/solver.cc:454-501
//
// The line searches are written against an abstract "evaluate at step size" callable, so that ceres_hip_debug_line_search (a caller's
// univariate function, no device) and the device minimizer run the same code.  A sample of the device minimizer owns a SLOT of a small
// pool of device vectors (vector_x ambient, vector_gradient tangent): samples are copied by copying the slot's handle, never the data,
// and a slot returns to the pool when its last sample goes.

namespace {

struct LsSample {   // FunctionSample, I/function_sample.h
  double x = 0.0, value = 0.0, gradient = 0.0;
  bool value_is_valid = false, gradient_is_valid = false, vector_x_is_valid = false, vector_gradient_is_valid = false;
  std::shared_ptr<int> slot;   // device minimizer: the pool slot holding vector_x / vector_gradient
  // device minimizer, read back with the sample's value: |position|^2, |vector_x - position|^2, and the norms of
  // vector_x - Plus(vector_x, -vector_gradient) (the last two only with the gradient)
  double x_norm2 = 0.0, step_norm2 = 0.0, gradient_norm2 = 0.0, gradient_max = 0.0;
};
// evaluate at a step size; a non-zero return is an error of the machinery (a HIP error), not an invalid sample
using LsEvaluate = std::function<int(double x, bool want_gradient, LsSample* out)>;

struct LsSearchOptions {   // LineSearch::Options
  int interpolation_type = CERES_HIP_CUBIC;
  double sufficient_decrease = 1e-4, max_step_contraction = 1e-3, min_step_contraction = 0.6, min_step_size = 1e-9;
  int max_num_iterations = 20;
  double sufficient_curvature_decrease = 0.9, max_step_expansion = 10.0;
  double direction_max_norm = 1.0;   // LineSearchFunction::DirectionInfinityNorm
};
struct LsSearchSummary {   // LineSearch::Summary
  bool success = false;
  LsSample optimal_point;
  int num_function_evaluations = 0, num_gradient_evaluations = 0, num_iterations = 0;
  std::string error;
  int rc = 0;   // an error of the machinery stops the search: success stays false
};

std::string ls_format(const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

double ls_poly_eval(const std::vector<double>& poly, double x) {   // EvaluatePolynomial: Horner, highest power first
  double v = 0.0;
  for (double c : poly) v = v * x + c;
  return v;
}

// FindInterpolatingPolynomial: one equation per valid value / gradient, solved by LU with FULL pivoting and threshold 0 — a pivot
// that is exactly zero ends the elimination and the unknowns left get 0 (Eigen's FullPivLU(...).setThreshold(0.0).solve()).
std::vector<double> ls_find_interpolating_polynomial(const std::vector<LsSample>& samples) {
  int nc = 0;
  for (const LsSample& s : samples) nc += int(s.value_is_valid) + int(s.gradient_is_valid);
  const int degree = nc - 1;
  std::vector<double> A(size_t(nc) * nc, 0.0), b(nc, 0.0);
  int row = 0;
  for (const LsSample& s : samples) {
    if (s.value_is_valid) {
      for (int j = 0; j <= degree; ++j) A[row * nc + j] = std::pow(s.x, degree - j);
      b[row++] = s.value;
    }
    if (s.gradient_is_valid) {
      for (int j = 0; j < degree; ++j) A[row * nc + j] = (degree - j) * std::pow(s.x, degree - j - 1);
      b[row++] = s.gradient;
    }
  }
  std::vector<int> col(nc);
  for (int j = 0; j < nc; ++j) col[j] = j;
  int rank = 0;
  for (int k = 0; k < nc; ++k) {
    int pr = k, pc = k;
    double big = 0.0;
    for (int i = k; i < nc; ++i)
      for (int j = k; j < nc; ++j)
        if (std::fabs(A[i * nc + j]) > big) { big = std::fabs(A[i * nc + j]); pr = i; pc = j; }
    if (big == 0.0) break;
    if (pr != k) { for (int j = 0; j < nc; ++j) std::swap(A[k * nc + j], A[pr * nc + j]); std::swap(b[k], b[pr]); }
    if (pc != k) { for (int i = 0; i < nc; ++i) std::swap(A[i * nc + k], A[i * nc + pc]); std::swap(col[k], col[pc]); }
    for (int i = k + 1; i < nc; ++i) {
      const double f = A[i * nc + k] / A[k * nc + k];
      A[i * nc + k] = 0.0;
      for (int j = k + 1; j < nc; ++j) A[i * nc + j] -= f * A[k * nc + j];
      b[i] -= f * b[k];
    }
    ++rank;
  }
  std::vector<double> y(nc, 0.0), poly(nc, 0.0);
  for (int i = rank - 1; i >= 0; --i) {
    double v = b[i];
    for (int j = i + 1; j < rank; ++j) v -= A[i * nc + j] * y[j];
    y[i] = v / A[i * nc + i];
  }
  for (int i = 0; i < rank; ++i) poly[col[i]] = y[i];
  return poly;
}

// MinimizePolynomial: the midpoint, both ends, then the real parts of ALL roots of the derivative (the reference's "overkill": roots
// with an imaginary part included) that lie in the interval
void ls_minimize_polynomial(const std::vector<double>& poly, double x_min, double x_max, double* optimal_x, double* optimal_value) {
  *optimal_x = (x_min + x_max) / 2.0;
  *optimal_value = ls_poly_eval(poly, *optimal_x);
  const double v_min = ls_poly_eval(poly, x_min);
  if (v_min < *optimal_value) { *optimal_value = v_min; *optimal_x = x_min; }
  const double v_max = ls_poly_eval(poly, x_max);
  if (v_max < *optimal_value) { *optimal_value = v_max; *optimal_x = x_max; }
  if (poly.size() <= 2) return;
  const int degree = int(poly.size()) - 1;
  double der[5], re[4];
  for (int i = 0; i < degree; ++i) der[i] = (degree - i) * poly[i];
  const int nr = dl_poly_real_parts(der, degree, re);   // (dogleg.inc: closed forms up to the quadratic, Aberth-Ehrlich above)
  if (nr < 0) return;   // "Unable to find the critical points of the interpolating polynomial."
  for (int i = 0; i < nr; ++i) {
    if (re[i] < x_min || re[i] > x_max) continue;
    const double v = ls_poly_eval(poly, re[i]);
    if (v < *optimal_value) { *optimal_value = v; *optimal_x = re[i]; }
  }
}

void ls_minimize_interpolating_polynomial(const std::vector<LsSample>& samples, double x_min, double x_max, double* optimal_x,
                                          double* optimal_value, std::vector<double>* poly_out = nullptr) {
  const std::vector<double> poly = ls_find_interpolating_polynomial(samples);
  ls_minimize_polynomial(poly, x_min, x_max, optimal_x, optimal_value);
  for (const LsSample& s : samples) {
    if (s.x < x_min || s.x > x_max) continue;
    const double v = ls_poly_eval(poly, s.x);
    if (v < *optimal_value) { *optimal_x = s.x; *optimal_value = v; }
  }
  if (poly_out) *poly_out = poly;
}

// LineSearch::InterpolatingPolynomialMinimizingStepSize, I/line_search.cc:210-276
double ls_interpolating_step_size(int type, const LsSample& lowerbound, const LsSample& previous, const LsSample& current,
                                  double min_step_size, double max_step_size) {
  if (!current.value_is_valid || (type == CERES_HIP_BISECTION && max_step_size <= current.x))
    return std::min(std::max(current.x * 0.5, min_step_size), max_step_size);   // invalid sample, or BISECTION contracting
  if (type == CERES_HIP_BISECTION) return max_step_size;   // BISECTION "expanding": always the maximum step
  std::vector<LsSample> samples;
  samples.push_back(lowerbound);
  auto value_only = [](const LsSample& s) {
    LsSample v;
    v.x = s.x; v.value = s.value; v.value_is_valid = true;
    return v;
  };
  if (type == CERES_HIP_QUADRATIC) {   // function values, and the gradient at the lower bound
    samples.push_back(value_only(current));
    if (previous.value_is_valid) samples.push_back(value_only(previous));
  } else {   // CUBIC: function values and gradients
    samples.push_back(current);
    if (previous.value_is_valid) samples.push_back(previous);
  }
  double step_size = 0.0, unused = 0.0;
  ls_minimize_interpolating_polynomial(samples, min_step_size, max_step_size, &step_size, &unused);
  return step_size;
}

#define LS_EVAL(x, want_gradient, out)                                       \
  do {                                                                       \
    ++S->num_function_evaluations;                                           \
    if (want_gradient) ++S->num_gradient_evaluations;                        \
    S->rc = eval((x), (want_gradient), (out));                               \
    if (S->rc != 0) { S->error = "Line search failed: evaluation error."; return; } \
  } while (0)

// ArmijoLineSearch::DoSearch, I/line_search.cc:281-366
void ls_armijo_search(const LsSearchOptions& o, const LsEvaluate& eval, const LsSample& initial_position, double step_size_estimate, LsSearchSummary* S) {
  const double initial_cost = initial_position.value, initial_gradient = initial_position.gradient;
  LsSample previous, current;
  const bool want_gradient = o.interpolation_type == CERES_HIP_CUBIC;
  LS_EVAL(step_size_estimate, want_gradient, &current);
  while (!current.value_is_valid || current.value > (initial_cost + o.sufficient_decrease * initial_gradient * current.x)) {
    ++S->num_iterations;
    if (S->num_iterations >= o.max_num_iterations) {
      S->error = ls_format("Line search failed: Armijo failed to find a point satisfying the sufficient decrease condition within "
                           "specified max_num_iterations: %d.", o.max_num_iterations);
      return;
    }
    const double step_size = ls_interpolating_step_size(o.interpolation_type, initial_position, previous, current,
                                                        o.max_step_contraction * current.x, o.min_step_contraction * current.x);
    if (step_size * o.direction_max_norm < o.min_step_size) {
      S->error = ls_format("Line search failed: step_size too small: %.5e with descent_direction_max_norm: %.5e.", step_size, o.direction_max_norm);
      return;
    }
    previous = current;
    LS_EVAL(step_size, want_gradient, &current);
  }
  S->optimal_point = current;
  S->success = true;
}
#undef LS_EVAL

#define LS_EVAL(x, out)                                                      \
  do {                                                                       \
    ++S->num_function_evaluations;                                           \
    ++S->num_gradient_evaluations;                                           \
    S->rc = eval((x), true, (out));                                          \
    if (S->rc != 0) { S->error = "Line search failed: evaluation error."; return false; } \
  } while (0)

// WolfeLineSearch::BracketingPhase, I/line_search.cc:500-693
bool ls_wolfe_bracket(const LsSearchOptions& o, const LsEvaluate& eval, const LsSample& initial_position, double step_size_estimate,
                      LsSample* bracket_low, LsSample* bracket_high, bool* do_zoom_search, LsSearchSummary* S) {
  LsSample previous = initial_position, current;
  const double dmax = o.direction_max_norm;
  *do_zoom_search = false;
  *bracket_low = initial_position;
  LS_EVAL(step_size_estimate, &current);
  while (true) {
    ++S->num_iterations;
    if (current.value_is_valid && (current.value > (initial_position.value + o.sufficient_decrease * initial_position.gradient * current.x) ||
                                   (previous.value_is_valid && current.value > previous.value))) {
      *do_zoom_search = true;   // Armijo violated, or past a minimum of f relative to the previous step
      *bracket_low = previous;
      *bracket_high = current;
      break;
    }
    if (current.value_is_valid && std::fabs(current.gradient) <= -o.sufficient_curvature_decrease * initial_position.gradient) {
      *bracket_low = current;   // the strong Wolfe conditions hold: no zoom
      *bracket_high = current;
      break;
    } else if (current.value_is_valid && current.gradient >= 0) {
      *do_zoom_search = true;   // Armijo holds, f' >= 0: past a minimum; note the inverse ordering
      *bracket_low = current;
      *bracket_high = previous;
      break;
    } else if (current.value_is_valid && std::fabs(current.x - previous.x) * dmax < o.min_step_size) {
      *bracket_low = current;   // the bracket shrank below the tolerance: the Armijo point found
      break;
    } else if (S->num_iterations >= o.max_num_iterations) {
      S->error = ls_format("Line search failed: Wolfe bracketing phase failed to find a point satisfying strong Wolfe conditions, or a "
                           "bracket containing such a point within specified max_num_iterations: %d", o.max_num_iterations);
      if (current.value_is_valid && current.value < bracket_low->value) *bracket_low = current;
      break;
    }
    // a valid f(current) that met no criterion: expand; an invalid one: contract without inverting the bracket
    const double min_step_size = current.value_is_valid ? current.x : previous.x;
    const double max_step_size = current.value_is_valid ? current.x * o.max_step_expansion : current.x;
    const LsSample unused_previous;
    const double step_size = ls_interpolating_step_size(o.interpolation_type, previous, unused_previous, current, min_step_size, max_step_size);
    if (step_size * dmax < o.min_step_size) {
      S->error = ls_format("Line search failed: step_size too small: %.5e with descent_direction_max_norm: %.5e", step_size, dmax);
      return false;
    }
    if (current.value_is_valid) previous = current;
    LS_EVAL(step_size, &current);
  }
  if (*do_zoom_search && std::fabs(bracket_high->x - bracket_low->x) * dmax < o.min_step_size) *do_zoom_search = false;
  return true;
}

// WolfeLineSearch::ZoomPhase, I/line_search.cc:699-882
bool ls_wolfe_zoom(const LsSearchOptions& o, const LsEvaluate& eval, const LsSample& initial_position, LsSample bracket_low, LsSample bracket_high,
                   LsSample* solution, LsSearchSummary* S) {
  if (bracket_low.gradient * (bracket_high.x - bracket_low.x) >= 0) {
    S->error = ls_format("Line search failed: Wolfe zoom phase passed a bracket which does not satisfy: bracket_low.gradient * "
                         "(bracket_high.x - bracket_low.x) < 0 [%.8e !< 0], the most likely cause of which is the cost function "
                         "returning inconsistent gradient & function values.", bracket_low.gradient * (bracket_high.x - bracket_low.x));
    solution->value_is_valid = false;
    return false;
  }
  const int num_bracketing_iterations = S->num_iterations;
  const double dmax = o.direction_max_norm;
  while (true) {
    *solution = bracket_low;   // the best Armijo point so far
    if (S->num_iterations >= o.max_num_iterations) {
      S->error = ls_format("Line search failed: Wolfe zoom phase failed to find a point satisfying strong Wolfe conditions within "
                           "specified max_num_iterations: %d, (num iterations taken for bracketing: %d).", o.max_num_iterations,
                           num_bracketing_iterations);
      return false;
    }
    if (std::fabs(bracket_high.x - bracket_low.x) * dmax < o.min_step_size) {
      S->error = ls_format("Line search failed: Wolfe zoom bracket width: %.5e too small with descent_direction_max_norm: %.5e.",
                           std::fabs(bracket_high.x - bracket_low.x), dmax);
      return false;
    }
    ++S->num_iterations;
    // the interpolation wants its samples ordered by step size, not by f
    const LsSample& lower_bound_step = bracket_low.x < bracket_high.x ? bracket_low : bracket_high;
    const LsSample& upper_bound_step = bracket_low.x < bracket_high.x ? bracket_high : bracket_low;
    const LsSample unused_previous;
    const double step_size = ls_interpolating_step_size(o.interpolation_type, lower_bound_step, unused_previous, upper_bound_step,
                                                        lower_bound_step.x, upper_bound_step.x);
    LS_EVAL(step_size, solution);
    if (!solution->value_is_valid || !solution->gradient_is_valid) {
      S->error = ls_format("Line search failed: Wolfe Zoom phase found step_size: %.5e, for which function is invalid, between low_step: "
                           "%.5e and high_step: %.5e at which function is valid.", solution->x, bracket_low.x, bracket_high.x);
      return false;
    }
    if (solution->value > (initial_position.value + o.sufficient_decrease * initial_position.gradient * solution->x) ||
        solution->value >= bracket_low.value) {
      bracket_high = *solution;   // no sufficient decrease, or no better than the lowest sample: the new upper bound
      continue;
    }
    if (std::fabs(solution->gradient) <= -o.sufficient_curvature_decrease * initial_position.gradient) break;   // strong Wolfe
    else if (solution->gradient * (bracket_high.x - bracket_low.x) >= 0) bracket_high = bracket_low;
    bracket_low = *solution;
  }
  return true;
}
#undef LS_EVAL

// WolfeLineSearch::DoSearch, I/line_search.cc:371-482
void ls_wolfe_search(const LsSearchOptions& o, const LsEvaluate& eval, const LsSample& initial_position, double step_size_estimate, LsSearchSummary* S) {
  bool do_zoom_search = false;
  LsSample solution, bracket_low, bracket_high;
  if (!ls_wolfe_bracket(o, eval, initial_position, step_size_estimate, &bracket_low, &bracket_high, &do_zoom_search, S)) return;
  if (!do_zoom_search) {   // a strong Wolfe point, or the best Armijo point where bracketing stopped for an artificial reason
    S->optimal_point = bracket_low;
    S->success = true;
    return;
  }
  if (!ls_wolfe_zoom(o, eval, initial_position, bracket_low, bracket_high, &solution, S) && !solution.value_is_valid) return;
  if (S->rc != 0) return;
  S->optimal_point = (!solution.value_is_valid || solution.value > bracket_low.value) ? bracket_low : solution;
  S->success = true;
}

// LineSearch::Search.  initial_position: x = 0, the cost and the directional derivative there (valid), and the position's slot.
void ls_search(int line_search_type, const LsSearchOptions& o, const LsEvaluate& eval, const LsSample& initial_position, double step_size_estimate,
               LsSearchSummary* S) {
  *S = LsSearchSummary();
  if (line_search_type == CERES_HIP_ARMIJO) ls_armijo_search(o, eval, initial_position, step_size_estimate, S);
  else ls_wolfe_search(o, eval, initial_position, step_size_estimate, S);
}

// LineSearchOptionsAreValid with Ceres' wording; "" = valid.  *unsupported: BFGS.
std::string ls_validate(const ceres_hip_line_search_options& o, bool* unsupported) {
  *unsupported = false;
  auto violated = [](const char* name, double v, const char* constraint) {
    std::ostringstream ss;
    ss << "Invalid configuration. Solver::Options::" << name << " = " << v << ". Violated constraint: Solver::Options::" << name << " " << constraint;
    return ss.str();
  };
  auto violated2 = [](const char* x, double vx, const char* y, double vy, const char* op) {
    std::ostringstream ss;
    ss << "Invalid configuration. Solver::Options::" << x << " = " << vx << ". Solver::Options::" << y << " = " << vy
       << ". Violated constraint: Solver::Options::" << x << op << " Solver::Options::" << y << ".";
    return ss.str();
  };
  if (!(o.max_num_iterations >= 0)) return violated("max_num_iterations", o.max_num_iterations, ">= 0");
  if (!(o.function_tolerance >= 0.0)) return violated("function_tolerance", o.function_tolerance, ">= 0.0");
  if (!(o.gradient_tolerance >= 0.0)) return violated("gradient_tolerance", o.gradient_tolerance, ">= 0.0");
  if (!(o.parameter_tolerance >= 0.0)) return violated("parameter_tolerance", o.parameter_tolerance, ">= 0.0");
  if (o.line_search_direction_type < CERES_HIP_STEEPEST_DESCENT || o.line_search_direction_type > CERES_HIP_BFGS)
    return "Invalid configuration. Unknown line_search_direction_type " + std::to_string(o.line_search_direction_type) + ".";
  if (o.nonlinear_conjugate_gradient_type < CERES_HIP_FLETCHER_REEVES || o.nonlinear_conjugate_gradient_type > CERES_HIP_HESTENES_STIEFEL)
    return "Invalid configuration. Unknown nonlinear_conjugate_gradient_type " + std::to_string(o.nonlinear_conjugate_gradient_type) + ".";
  if (o.line_search_type < CERES_HIP_ARMIJO || o.line_search_type > CERES_HIP_WOLFE)
    return "Invalid configuration. Unknown line_search_type " + std::to_string(o.line_search_type) + ".";
  if (o.line_search_interpolation_type < CERES_HIP_BISECTION || o.line_search_interpolation_type > CERES_HIP_CUBIC)
    return "Invalid configuration. Unknown line_search_interpolation_type " + std::to_string(o.line_search_interpolation_type) + ".";
  if (!(o.max_num_line_search_direction_restarts >= 0))
    return violated("max_num_line_search_direction_restarts", o.max_num_line_search_direction_restarts, ">= 0");
  if (!(o.max_lbfgs_rank > 0)) return violated("max_lbfgs_rank", o.max_lbfgs_rank, "> 0");
  if (!(o.min_line_search_step_size > 0.0)) return violated("min_line_search_step_size", o.min_line_search_step_size, "> 0.0");
  if (!(o.max_line_search_step_contraction > 0.0)) return violated("max_line_search_step_contraction", o.max_line_search_step_contraction, "> 0.0");
  if (!(o.max_line_search_step_contraction < 1.0)) return violated("max_line_search_step_contraction", o.max_line_search_step_contraction, "< 1.0");
  if (!(o.max_line_search_step_contraction < o.min_line_search_step_contraction))
    return violated2("max_line_search_step_contraction", o.max_line_search_step_contraction, "min_line_search_step_contraction",
                     o.min_line_search_step_contraction, "<");
  if (!(o.min_line_search_step_contraction <= 1.0)) return violated("min_line_search_step_contraction", o.min_line_search_step_contraction, "<= 1.0");
  if (!(o.max_num_line_search_step_size_iterations >= 1))
    return violated("max_num_line_search_step_size_iterations", o.max_num_line_search_step_size_iterations,
                    ">= (options.minimizer_type == ceres::TRUST_REGION ? 0 : 1)");
  if (!(o.line_search_sufficient_function_decrease > 0.0))
    return violated("line_search_sufficient_function_decrease", o.line_search_sufficient_function_decrease, "> 0.0");
  if (!(o.line_search_sufficient_function_decrease < o.line_search_sufficient_curvature_decrease))
    return violated2("line_search_sufficient_function_decrease", o.line_search_sufficient_function_decrease,
                     "line_search_sufficient_curvature_decrease", o.line_search_sufficient_curvature_decrease, "<");
  if (!(o.line_search_sufficient_curvature_decrease < 1.0))
    return violated("line_search_sufficient_curvature_decrease", o.line_search_sufficient_curvature_decrease, "< 1.0");
  if (!(o.max_line_search_step_expansion > 1.0)) return violated("max_line_search_step_expansion", o.max_line_search_step_expansion, "> 1.0");
  if ((o.line_search_direction_type == CERES_HIP_BFGS || o.line_search_direction_type == CERES_HIP_LBFGS) && o.line_search_type != CERES_HIP_WOLFE)
    return "Invalid configuration: Solver::Options::line_search_type = ARMIJO. When using (L)BFGS, Solver::Options::line_search_type must be "
           "set to WOLFE.";
  // (the reference only warns here and goes on; a BISECTION that cannot halve is refused)
  if (o.line_search_interpolation_type == CERES_HIP_BISECTION && (o.max_line_search_step_contraction > 0.5 || o.min_line_search_step_contraction < 0.5)) {
    std::ostringstream ss;
    ss << "Line search interpolation type is BISECTION, but specified max_line_search_step_contraction: " << o.max_line_search_step_contraction
       << ", and min_line_search_step_contraction: " << o.min_line_search_step_contraction << ", prevent bisection (0.5) scaling.";
    return ss.str();
  }
  if (o.line_search_direction_type == CERES_HIP_BFGS) {
    *unsupported = true;
    return "BFGS keeps a dense num_parameters x num_parameters inverse Hessian and is not offered: use CERES_HIP_LBFGS (L-BFGS).";
  }
  return "";
}

LsSearchOptions ls_search_options(const ceres_hip_line_search_options& o) {
  LsSearchOptions so;
  so.interpolation_type = o.line_search_interpolation_type;
  so.min_step_size = o.min_line_search_step_size;
  so.sufficient_decrease = o.line_search_sufficient_function_decrease;
  so.max_step_contraction = o.max_line_search_step_contraction;
  so.min_step_contraction = o.min_line_search_step_contraction;
  so.max_num_iterations = o.max_num_line_search_step_size_iterations;
  so.sufficient_curvature_decrease = o.line_search_sufficient_curvature_decrease;
  so.max_step_expansion = o.max_line_search_step_expansion;
  return so;
}

}  // namespace

// What the gradient-only evaluator and the minimizer keep on a handle: built on first use, freed by ceres_hip_bal_destroy (the device
// buffers with the solver's other allocations).
struct BalLineSearch {
  LsGradArgs G;                 // the structure part of the evaluator's arguments (device pointers)
  int64_t* d_blocks = nullptr;  // BalFreeBlocks::block for every handle
  double* d_dir = nullptr;      // the search direction (tangent)
  std::vector<double*> slot_x, slot_g;   // the sample pool
  std::vector<int> free_slots;
  // L-BFGS
  LbfgsArgs L;
  double* lbfgs_history = nullptr;   // 2 x lbfgs_capacity x n_t doubles
  int lbfgs_capacity = 0;            // the rank the history and the per-slot scalars were allocated for
  int lbfgs_rank = 0;                // the rank of the call in progress (<= lbfgs_capacity)
  int64_t lbfgs_bytes = 0;           // the history's allocation
};

namespace {

constexpr int kLsMaxSlots = 12;

// give the history and the per-slot scalars back before a larger rank's replace them
void ls_release_history(ceres_hip_solver* s, BalLineSearch* ls) {
  const int64_t cap = std::max(ls->lbfgs_capacity, 1);
  dev_release(s, ls->lbfgs_history, ls->lbfgs_bytes);
  dev_release(s, ls->L.sy, cap * int64_t(sizeof(double))); dev_release(s, ls->L.alpha, cap * int64_t(sizeof(double)));
  dev_release(s, ls->L.order, cap * int64_t(sizeof(int32_t)));
  ls->lbfgs_history = nullptr; ls->L.sy = nullptr; ls->L.alpha = nullptr; ls->L.order = nullptr; ls->L.S = nullptr; ls->L.Y = nullptr;
  ls->lbfgs_capacity = 0; ls->lbfgs_bytes = 0;
}

BalFreeBlocks ls_blocks(const ceres_hip_bal* p) { return BalFreeBlocks{p->ls->d_blocks, p->nfp, p->nfc}; }

// The point pass's row_pdst and long-point list, the camera pass's lists and chunks: the rows grouped by camera (bal_group_by).
int bal_ls_prepare(ceres_hip_bal* p) {
  if (p->ls) return 0;
  ceres_hip_solver* s = p->s;
  if (p->n_t > int64_t(INT32_MAX) || p->no > int64_t(INT32_MAX) - 64) return fail(s, CERES_HIP_E_UNSUPPORTED, "line search: more than 2^31 tangent entries or rows");
  const int64_t no = p->no;
  BalHostRows H;
  TRY(bal_fetch_rows(p, kRowCam | kRowPt | kRowPixel, H));
  std::unique_ptr<BalLineSearch> ls(new BalLineSearch);
  // point pass
  std::vector<int32_t> pdst(no), long_dst, long_w0, long_w1;
  std::vector<char> seen(size_t(p->nfp), 0);
  for (int64_t r = 0; r < no; ++r) { const int pc = bal_point_column(p, H.pt[r]); pdst[r] = pc >= 0 ? 3 * pc : -1; }
  for (int64_t a = 0; a < no;) {
    int64_t b = a + 1;
    while (b < no && pdst[b] == pdst[a]) ++b;
    if (pdst[a] >= 0) {
      if (seen[pdst[a] / 3]) return fail(s, CERES_HIP_E_UNSUPPORTED, "line search: the rows of a point are not consecutive");
      seen[pdst[a] / 3] = 1;
      if (a / 64 != (b - 1) / 64) { long_dst.push_back(pdst[a]); long_w0.push_back(int32_t(a / 64)); long_w1.push_back(int32_t((b - 1) / 64)); }
    }
    a = b;
  }
  for (char c : seen) if (!c) return fail(s, CERES_HIP_E_UNSUPPORTED, "line search: a free point without a row");
  // camera pass: the rows of every free camera in ascending order, cut into chunks of 64
  const BalGrouping by_cam = bal_group_by(no, p->nfc, [&](int64_t r) { return bal_camera_column(p, H.cam[r]); });
  const std::vector<int32_t>& cptr = by_cam.ptr;
  std::vector<int32_t> ch_cam, ch_start, ch_len, ch_dst, fin_dst, fin_first, fin_count;
  int32_t n_partials = 0;
  for (int c = 0; c < p->nfc; ++c) {
    const int32_t len = cptr[c + 1] - cptr[c], nch = (len + 63) / 64, dst = int32_t(3 * int64_t(p->nfp) + int64_t(p->cw) * c);
    if (len == 0) return fail(s, CERES_HIP_E_UNSUPPORTED, "line search: a free camera without a row");
    if (nch > 1) { fin_dst.push_back(dst); fin_first.push_back(n_partials); fin_count.push_back(nch); }
    for (int k = 0; k < nch; ++k) {
      ch_cam.push_back(H.cam[by_cam.perm[cptr[c]]]); ch_start.push_back(cptr[c] + 64 * k); ch_len.push_back(std::min(64, len - 64 * k));
      ch_dst.push_back(nch > 1 ? -(n_partials++) - 1 : dst);
    }
  }
  const std::vector<int32_t> cm_pt = bal_gather(by_cam, H.pt.data());
  const std::vector<double> cm_obs = bal_gather(by_cam, H.pixel.data(), 2);
  const std::vector<int64_t> blocks = bal_free_block_offsets(p->nc, p->np, p->cs, p->cam_col, p->pt_col);   // (no constants: no maps, every block)
  LsGradArgs& G = ls->G;
  int32_t *d_pdst, *d_ldst, *d_lw0, *d_lw1, *d_ccam, *d_cstart, *d_clen, *d_cdst, *d_cmpt, *d_fdst, *d_ffirst, *d_fcount;
  double2* d_cmobs;
  TRY(dev_upload(s, &d_pdst, pdst)); TRY(dev_upload(s, &d_ldst, long_dst)); TRY(dev_upload(s, &d_lw0, long_w0)); TRY(dev_upload(s, &d_lw1, long_w1));
  TRY(dev_upload(s, &d_ccam, ch_cam)); TRY(dev_upload(s, &d_cstart, ch_start)); TRY(dev_upload(s, &d_clen, ch_len)); TRY(dev_upload(s, &d_cdst, ch_dst));
  TRY(dev_upload(s, &d_cmpt, cm_pt)); TRY(dev_upload_pixels(s, &d_cmobs, cm_obs));
  TRY(dev_upload(s, &d_fdst, fin_dst)); TRY(dev_upload(s, &d_ffirst, fin_first)); TRY(dev_upload(s, &d_fcount, fin_count));
  TRY(dev_upload(s, &ls->d_blocks, blocks));
  TRY(dev_alloc(s, &G.wave_parts, size_t(6 * ((no + 63) / 64))));
  TRY(dev_alloc(s, &G.chunk_parts, size_t(kLsChunkPitch) * size_t(std::max(n_partials, 1))));
  TRY(dev_alloc(s, &ls->d_dir, size_t(p->n_t)));
  HIP_TRY(s, hipStreamSynchronize(s->stream));   // (the uploads read host vectors that go out of scope here)
  G.n_rows = no; G.row_cam = p->d_row_cam; G.row_pt = p->d_row_pt; G.row_obs = p->d_row_obs; G.row_pdst = d_pdst;
  G.cam_base = 3 * int64_t(p->np);
  G.n_long = int32_t(long_dst.size()); G.long_dst = d_ldst; G.long_w0 = d_lw0; G.long_w1 = d_lw1;
  G.n_chunks = int32_t(ch_cam.size()); G.chunk_cam = d_ccam; G.chunk_start = d_cstart; G.chunk_len = d_clen; G.chunk_dst = d_cdst;
  G.cm_pt = d_cmpt; G.cm_obs = d_cmobs;
  G.n_fin = int32_t(fin_dst.size()); G.fin_dst = d_fdst; G.fin_first = d_ffirst; G.fin_count = d_fcount;
  p->ls = ls.release();
  return 0;
}

// enqueue cost (and gradient) at a device state; *cost: the set of the cost's partial sums
int bal_ls_evaluate_enqueue(ceres_hip_bal* p, const double* d_state, double* d_gradient, PartialSet* cost) {
  LsGradArgs A = p->ls->G;
  A.state = d_state; A.grad = d_gradient; A.loss = p->loss;
  TRY(bal_parts_room(p, kMaxEvalGrid, &A.cost_partials));
  int nparts = 0;
  HIP_TRY(p->s, LaunchLsGradient(A, d_gradient != nullptr, p->camera_model, &nparts, p->s->stream));
  *cost = p->parts.take(nparts);
  return 0;
}
// a . b, a . c (0 without c) and max |a| of tangent vectors, enqueued: the three sets of ls_dots_kernel
int bal_ls_dots_enqueue(ceres_hip_bal* p, const double* a, const double* b, const double* c, PartialSet* ab, PartialSet* ac, PartialSet* amax) {
  int nd = 0; double* parts = nullptr;
  TRY(bal_parts_room(p, 3 * kMaxVecGrid, &parts));
  HIP_TRY(p->s, LaunchLsDots(a, b, c, p->n_t, parts, &nd, p->s->stream));
  *ab = p->parts.take(nd); *ac = p->parts.take(nd); *amax = p->parts.take(nd);
  return 0;
}

}  // namespace

void bal_ls_free(ceres_hip_bal* p) {
  if (!p->ls) return;
  delete p->ls;
  p->ls = nullptr;
}

extern "C" {

void ceres_hip_line_search_default_options(ceres_hip_line_search_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;   // include/ceres/solver.h defaults
  o->line_search_direction_type = CERES_HIP_LBFGS;
  o->nonlinear_conjugate_gradient_type = CERES_HIP_FLETCHER_REEVES;
  o->max_lbfgs_rank = 20;
  o->use_approximate_eigenvalue_bfgs_scaling = 0;
  o->line_search_type = CERES_HIP_WOLFE;
  o->line_search_interpolation_type = CERES_HIP_CUBIC;
  o->max_num_line_search_step_size_iterations = 20;
  o->max_num_line_search_direction_restarts = 5;
  o->min_line_search_step_size = 1e-9;
  o->line_search_sufficient_function_decrease = 1e-4;
  o->max_line_search_step_contraction = 1e-3;
  o->min_line_search_step_contraction = 0.6;
  o->line_search_sufficient_curvature_decrease = 0.9;
  o->max_line_search_step_expansion = 10.0;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
}

int ceres_hip_bal_evaluate_gradient(ceres_hip_bal* p, const double* state, double* cost, double* gradient) {
  if (!p || !state || !cost) {
    (p ? p->err : g_create_error) = std::string("ceres_hip_bal_evaluate_gradient: ") + (!state ? "NULL state" : !cost ? "NULL cost" : "NULL problem handle");
    return CERES_HIP_E_INVALID;
  }
  ceres_hip_solver* s = p->s;
  if (s->world > 1) {
    p->err = "ceres_hip_bal_evaluate_gradient: not supported on sharded handles";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->n_groups) {   // (kernels_line_search.hip sums nine columns per camera, none over a group)
    p->err = "ceres_hip_bal_evaluate_gradient: not supported on handles with shared intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  if (p->intrinsics_mask) {   // (kernels_line_search.hip sums nine columns per camera)
    p->err = "ceres_hip_bal_evaluate_gradient: not supported on handles with fixed intrinsics";
    return CERES_HIP_E_UNSUPPORTED;
  }
  HIP_TRY(s, hipSetDevice(s->opt.device));
  BAL_TRY(p, bal_ls_prepare(p));
  BAL_TRY(p, up(s, p->d_cand, state, size_t(p->n_a)));   // (d_cand, d_delta: scratch of the trust-region loop between its calls)
  PartialSet c;
  BAL_TRY(p, bal_ls_evaluate_enqueue(p, p->d_cand, gradient ? p->d_delta : nullptr, &c));
  BAL_TRY(p, bal_parts_collect(p));
  *cost = p->parts.sum(c);
  if (gradient) BAL_TRY(p, down(s, gradient, p->d_delta, size_t(p->n_t)));
  return 0;
}

int ceres_hip_bal_minimize_line_search(ceres_hip_bal* p, const ceres_hip_line_search_options* o, double* state, ceres_hip_line_search_summary* S) {
  auto refuse = [&](int code, const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_minimize_line_search: " + why;
    return code;
  };
  if (!o) return refuse(CERES_HIP_E_INVALID, "NULL options");
  if (!state) return refuse(CERES_HIP_E_INVALID, "NULL state");
  if (!S) return refuse(CERES_HIP_E_INVALID, "NULL summary");
  {   // (the options before the handle: every rule is checked before any device call, and without a device)
    bool unsupported = false;
    const std::string why = ls_validate(*o, &unsupported);
    if (!why.empty()) return refuse(unsupported ? CERES_HIP_E_UNSUPPORTED : CERES_HIP_E_INVALID, why);
  }
  if (!p) return refuse(CERES_HIP_E_INVALID, "NULL problem handle");
  ceres_hip_solver* s = p->s;
  if (s->world > 1) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on sharded handles");
  if (p->intrinsics_mask) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with fixed intrinsics");
  if (p->n_groups) return refuse(CERES_HIP_E_UNSUPPORTED, "not supported on handles with shared intrinsics");
  if (p->is_constrained) return refuse(CERES_HIP_E_INVALID, "LINE_SEARCH Minimizer does not support bounds.");   // I/line_search_preprocessor.cc:47-51
  hipStream_t st = s->stream;
  HIP_TRY(s, hipSetDevice(s->opt.device));
  const auto t_start = std::chrono::steady_clock::now();
  memset(S, 0, sizeof(*S));
  BAL_TRY(p, bal_ls_prepare(p));
  BalLineSearch* ls = p->ls;
  const int64_t na = p->n_a, nt = p->n_t;
  const bool lbfgs = o->line_search_direction_type == CERES_HIP_LBFGS;
  if (lbfgs) {
    // The history and its per-slot scalars: allocated on the first call with LBFGS for that call's rank and kept on the handle; a later
    // call of a rank up to it uses the front of the same buffers, a larger rank replaces them (the old ones are freed first: no
    // kernel of an earlier call is in flight, every call ends synchronised).
    const int rank = o->max_lbfgs_rank;
    if (!ls->L.parts) {   // the rank-independent part, once
      BAL_TRY(p, dev_alloc(s, &ls->L.scale, size_t(1))); BAL_TRY(p, dev_alloc(s, &ls->L.count, size_t(1)));
      BAL_TRY(p, dev_alloc(s, &ls->L.parts, size_t(4 * kMaxVecGrid)));
    }
    if (rank > ls->lbfgs_capacity) {
      ls_release_history(s, ls);
      const int64_t bytes = 2 * int64_t(rank) * nt * int64_t(sizeof(double));
      ls->lbfgs_capacity = rank; ls->lbfgs_bytes = bytes;   // (what ls_release_history takes back where an allocation below fails)
      if (dev_alloc(s, &ls->lbfgs_history, size_t(2) * size_t(rank) * size_t(nt)) != 0) {
        ls_release_history(s, ls);
        p->err = "ceres_hip_bal_minimize_line_search: the L-BFGS history of " + std::to_string(bytes) + " bytes could not be allocated: " + s->err;
        return CERES_HIP_E_HIP;
      }
      if (dev_alloc(s, &ls->L.sy, size_t(rank)) != 0 || dev_alloc(s, &ls->L.alpha, size_t(rank)) != 0 || dev_alloc(s, &ls->L.order, size_t(rank)) != 0) {
        ls_release_history(s, ls);   // (all of it or none: the next call starts over)
        return bal_fail(p, CERES_HIP_E_HIP);
      }
    }
    ls->L.n = nt; ls->L.rank = rank; ls->lbfgs_rank = rank;
    ls->L.S = ls->lbfgs_history; ls->L.Y = ls->lbfgs_history + int64_t(rank) * nt;
  }
  ls->L.use_scaling = o->use_approximate_eigenvalue_bfgs_scaling ? 1 : 0;
  S->lbfgs_history_bytes = lbfgs ? ls->lbfgs_bytes : 0;
  S->termination_type = CERES_HIP_NO_CONVERGENCE_T;

  // the sample pool: a slot = {vector_x (ambient), vector_gradient (tangent)}; handles return their slot when the last copy goes
  ls->free_slots.clear();
  for (int k = int(ls->slot_x.size()) - 1; k >= 0; --k) ls->free_slots.push_back(k);
  BAL_TRY(p, up(s, p->d_x, state, size_t(na)));   // (d_x keeps the caller's state: the constant blocks of every slot are copied from it)
  // Plus writes free blocks only, so a slot's constant blocks are the caller's doubles: written once per call into the slots the handle
  // has, and into a new slot when it is allocated — not per trial point
  auto carry_constants = [&](int k) -> int {
    if (p->has_const) HIP_TRY(s, hipMemcpyAsync(ls->slot_x[k], p->d_x, sizeof(double) * na, hipMemcpyDeviceToDevice, st));
    return 0;
  };
  for (int k = 0; k < int(ls->slot_x.size()); ++k) BAL_TRY(p, carry_constants(k));
  auto acquire = [&](std::shared_ptr<int>* out) -> int {
    if (ls->free_slots.empty()) {
      if (int(ls->slot_x.size()) >= kLsMaxSlots) return fail(s, CERES_HIP_E_HIP, "line search: the sample pool is exhausted");
      double *vx = nullptr, *vg = nullptr;
      TRY(dev_alloc(s, &vx, size_t(na))); TRY(dev_alloc(s, &vg, size_t(nt)));
      ls->slot_x.push_back(vx); ls->slot_g.push_back(vg);
      ls->free_slots.push_back(int(ls->slot_x.size()) - 1);
      TRY(carry_constants(int(ls->slot_x.size()) - 1));
    }
    const int k = ls->free_slots.back();
    ls->free_slots.pop_back();
    std::vector<int>* pool = &ls->free_slots;
    *out = std::shared_ptr<int>(new int(k), [pool](int* q) { pool->push_back(*q); delete q; });
    return 0;
  };
  double fixed_cost = 0.0;
  if (p->has_const) BAL_TRY(p, bal_fixed_cost_device(p, p->d_x, &fixed_cost));

  // one evaluation's partial sums (and a trial point's, enqueued before it), copied and added after ONE synchronisation
  PartialSums& P = p->parts;
  // cost, gradient and the gradient norms at slot k (vector_x already there); direction != nullptr: also direction . gradient
  auto evaluate_slot = [&](int k, bool want_gradient, const double* direction, LsSample* out) -> int {
    const auto t0 = std::chrono::steady_clock::now();
    PartialSet cost, norm2, norm_max, dg, unused;
    TRY(bal_ls_evaluate_enqueue(p, ls->slot_x[k], want_gradient ? ls->slot_g[k] : nullptr, &cost));
    ++S->num_function_evaluations;
    if (want_gradient) {
      ++S->num_gradient_evaluations;
      int nn = 0; double* parts = nullptr;
      TRY(bal_parts_room(p, 2 * kMaxVecGrid, &parts));
      HIP_TRY(s, LaunchLsGradientNorms(ls_blocks(p), p->camera_model, ls->slot_x[k], ls->slot_g[k], parts, &nn, st));
      norm2 = P.take(nn); norm_max = P.take(nn);
      if (direction) TRY(bal_ls_dots_enqueue(p, direction, ls->slot_g[k], nullptr, &dg, &unused, &unused));
    }
    TRY(bal_parts_collect(p));
    out->value = P.sum(cost);
    out->value_is_valid = std::isfinite(out->value);
    if (want_gradient) {
      out->gradient_norm2 = P.sum(norm2); out->gradient_max = P.max(norm_max);
      if (direction) out->gradient = P.sum(dg);
    }
    S->evaluation_seconds += seconds_since(t0);
    return 0;
  };
  auto finish = [&](int term, const std::string& msg) {
    S->termination_type = term;
    snprintf(S->message, sizeof(S->message), "%s", msg.c_str());
  };
  auto log_iter = [&](const ceres_hip_line_search_iteration& it) {
    if (S->num_iterations_logged < CERES_HIP_MAX_LOGGED_ITERATIONS) S->iterations[S->num_iterations_logged++] = it;
  };

  // State of LineSearchMinimizer: the current point is a sample (slot: x and gradient); previous: the sample before it
  LsSample cur, prev;
  double cur_cost = 0, prev_cost = 0, cur_dirderiv = 0, prev_step_size = 0, prev_gnorm2 = 0;
  BAL_TRY(p, acquire(&cur.slot));
  HIP_TRY(s, hipMemcpyAsync(ls->slot_x[*cur.slot], p->d_x, sizeof(double) * na, hipMemcpyDeviceToDevice, st));
  BAL_TRY(p, evaluate_slot(*cur.slot, true, nullptr, &cur));
  int rc = 0;
  auto write_back = [&]() -> int {
    S->final_cost = cur_cost + fixed_cost;
    TRY(down(s, state, ls->slot_x[*cur.slot], size_t(na)));
    S->total_seconds = seconds_since(t_start);
    return 0;
  };
  if (!cur.value_is_valid) {
    finish(CERES_HIP_MINIMIZER_FAILURE, "Initial cost and jacobian evaluation failed.");
    S->total_seconds = seconds_since(t_start);
    return 0;
  }
  cur_cost = cur.value;
  S->initial_cost = cur_cost + fixed_cost;
  ceres_hip_line_search_iteration it{};
  it.cost = cur_cost + fixed_cost; it.gradient_norm = std::sqrt(cur.gradient_norm2); it.gradient_max_norm = cur.gradient_max;
  if (it.gradient_max_norm <= o->gradient_tolerance) {
    finish(CERES_HIP_CONVERGENCE, ls_format("Gradient tolerance reached. Gradient max norm: %e <= %e", it.gradient_max_norm, o->gradient_tolerance));
    BAL_TRY(p, write_back());
    return 0;
  }
  log_iter(it);
  if (lbfgs) HIP_TRY(s, LaunchLbfgsReset(ls->L, st));
  int lbfgs_updates = 0;   // the host's upper bound on the live history
  int iteration = 0, restarts = 0;
  double* dir = ls->d_dir;
  LsSearchOptions so = ls_search_options(*o);

  while (true) {
    if (iteration >= o->max_num_iterations) { finish(CERES_HIP_NO_CONVERGENCE_T, "Maximum number of iterations reached."); break; }
    ++iteration;
    it = ceres_hip_line_search_iteration{};
    const double* g = ls->slot_g[*cur.slot];
    // the direction; d . g and max |d| come back in one round trip
    const auto td = std::chrono::steady_clock::now();
    bool line_search_status = true;
    double dmax = 0;
    PartialSet dots_ab, dots_ac, dots_max;
    auto direction_dots = [&]() -> int {   // d . g and max |d| of the direction in `dir`
      TRY(bal_ls_dots_enqueue(p, dir, g, nullptr, &dots_ab, &dots_ac, &dots_max));
      TRY(bal_parts_collect(p));
      cur_dirderiv = P.sum(dots_ab); dmax = P.max(dots_max);
      return 0;
    };
    auto steepest = [&]() -> int {
      HIP_TRY(s, LaunchLsCombine(-1.0, g, 0.0, nullptr, 0.0, nullptr, dir, nt, st));
      return direction_dots();
    };
    if (iteration == 1 || o->line_search_direction_type == CERES_HIP_STEEPEST_DESCENT) {
      BAL_TRY(p, steepest());
    } else if (lbfgs) {
      // Update(previous.search_direction * previous.step_size, gradient - previous.gradient), then -H g: no synchronisation until d . g
      HIP_TRY(s, LaunchLbfgsUpdate(ls->L, prev_step_size, dir, g, ls->slot_g[*prev.slot], -1, st));
      lbfgs_updates = std::min(lbfgs_updates + 1, ls->lbfgs_rank);
      // THE EXCEPTION — the one read-back that does not come from the stage's device buffer: LaunchLbfgsDirection leaves d . g and
      // max |d| in its own L.parts (sets 2 and 3, kMaxVecGrid apart); they are copied into pinned storage taken from the stage
      int nd = 0; double* unused = nullptr;
      HIP_TRY(s, LaunchLbfgsDirection(ls->L, g, dir, lbfgs_updates, &nd, st));
      BAL_TRY(p, bal_parts_room(p, 2 * kMaxVecGrid, &unused));
      const PartialSet both = P.take(2 * kMaxVecGrid);
      P.drop();
      HIP_TRY(s, hipMemcpyAsync(P.host(both), ls->L.parts + 2 * kMaxVecGrid, sizeof(double) * 2 * kMaxVecGrid, hipMemcpyDeviceToHost, st));
      HIP_TRY(s, hipStreamSynchronize(st));
      cur_dirderiv = P.sum(PartialSet{both.offset, nd}); dmax = P.max(PartialSet{both.offset + kMaxVecGrid, nd});
      if (cur_dirderiv >= 0.0) line_search_status = false;   // the inverse Hessian approximation is not positive definite
    } else {   // NonlinearConjugateGradient
      const double* gp = ls->slot_g[*prev.slot];
      double beta = 0.0;
      if (o->nonlinear_conjugate_gradient_type == CERES_HIP_FLETCHER_REEVES) {
        beta = cur.gradient_norm2 / prev_gnorm2;
      } else {   // g . (g - g_prev) and d_prev . (g - g_prev): the change is formed once, in the pool's scratch of the step vector
        HIP_TRY(s, LaunchLsCombine(1.0, g, -1.0, gp, 0.0, nullptr, p->d_step, nt, st));
        BAL_TRY(p, bal_ls_dots_enqueue(p, p->d_step, g, dir, &dots_ab, &dots_ac, &dots_max));
        BAL_TRY(p, bal_parts_collect(p));
        const double g_dg = P.sum(dots_ab), d_dg = P.sum(dots_ac);
        beta = o->nonlinear_conjugate_gradient_type == CERES_HIP_POLAK_RIBIERE ? g_dg / prev_gnorm2 : g_dg / d_dg;
      }
      HIP_TRY(s, LaunchLsCombine(beta, dir, -1.0, g, 0.0, nullptr, dir, nt, st));   // -g + beta d_prev
      BAL_TRY(p, direction_dots());
      if (cur_dirderiv > -o->function_tolerance) BAL_TRY(p, steepest());   // "Restarting non-linear conjugate gradients"
    }
    if (!line_search_status && restarts >= o->max_num_line_search_direction_restarts) {
      finish(CERES_HIP_MINIMIZER_FAILURE, ls_format("Line search direction failure: specified max_num_line_search_direction_restarts: %d reached.",
                                                    o->max_num_line_search_direction_restarts));
      --iteration;
      break;
    } else if (!line_search_status) {   // a fresh direction object and steepest descent
      ++restarts;
      HIP_TRY(s, LaunchLbfgsReset(ls->L, st));
      lbfgs_updates = 0;
      BAL_TRY(p, steepest());
    }
    S->direction_seconds += seconds_since(td);
    const double initial_step_size = (iteration == 1 || !line_search_status) ? std::min(1.0, 1.0 / cur.gradient_max)
                                                                             : std::min(1.0, 2.0 * (cur_cost - prev_cost) / cur_dirderiv);
    if (initial_step_size < 0.0) {
      finish(CERES_HIP_MINIMIZER_FAILURE, ls_format("Numerical failure in line search, initial_step_size is negative: %.5e, directional_derivative: "
                                                    "%.5e, (current_cost - previous_cost): %.5e", initial_step_size, cur_dirderiv, cur_cost - prev_cost));
      --iteration;
      break;
    }
    // LineSearchFunction::Evaluate: vector_x = Plus(position, x direction), then the evaluator; everything of one trial point is
    // enqueued together and read back with one synchronisation
    const double* position = ls->slot_x[*cur.slot];
    double position_norm2 = 0.0;   // |position|^2: every trial point of this search reads it back (the search evaluates at least one)
    LsEvaluate eval = [&](double x, bool want_gradient, LsSample* out) -> int {
      *out = LsSample();
      out->x = x;
      TRY(acquire(&out->slot));
      int ntp = 0; double* parts = nullptr;
      TRY(bal_parts_room(p, 2 * kMaxVecGrid, &parts));
      HIP_TRY(s, LaunchLsTrialPoint(ls_blocks(p), p->camera_model, position, dir, x, ls->slot_x[*out->slot], parts, &ntp, st));
      const PartialSet x_norm2 = P.take(ntp), step_norm2 = P.take(ntp);
      out->vector_x_is_valid = true;
      TRY(evaluate_slot(*out->slot, want_gradient, dir, out));
      out->x_norm2 = P.sum(x_norm2); out->step_norm2 = P.sum(step_norm2);
      position_norm2 = out->x_norm2;
      if (!out->value_is_valid || !want_gradient) return 0;
      if (!std::isfinite(out->gradient)) return 0;
      out->gradient_is_valid = true; out->vector_gradient_is_valid = true;
      return 0;
    };
    so.direction_max_norm = dmax;
    LsSample initial_position;
    initial_position.x = 0.0; initial_position.value = cur_cost; initial_position.gradient = cur_dirderiv;
    initial_position.value_is_valid = true; initial_position.gradient_is_valid = true;
    initial_position.slot = cur.slot; initial_position.vector_x_is_valid = true;
    LsSearchSummary lss;
    ls_search(o->line_search_type, so, eval, initial_position, initial_step_size, &lss);
    if (lss.rc != 0) { rc = lss.rc; break; }
    if (!lss.success) {
      finish(CERES_HIP_MINIMIZER_FAILURE, ls_format("Numerical failure in line search, failed to find a valid step size, (did not run out of "
                                                    "iterations) using initial_step_size: %.5e, initial_cost: %.5e, initial_gradient: %.5e.",
                                                    initial_step_size, cur_cost, cur_dirderiv));
      --iteration;
      break;
    }
    LsSample opt = lss.optimal_point;
    lss.optimal_point = LsSample();
    if (opt.slot == cur.slot) {   // (the initial position itself came back — no sample beat it before the search had to stop: a step
      // of zero; its gradient is evaluated again below, as the reference does, and that is the only evaluation counted)
      opt.x_norm2 = position_norm2; opt.step_norm2 = 0.0; opt.vector_gradient_is_valid = false;
    }
    prev_step_size = opt.x;
    prev = cur; prev_cost = cur_cost; prev_gnorm2 = cur.gradient_norm2;
    if (!opt.vector_gradient_is_valid) {   // the accepted point's gradient is reused where the search has it; otherwise evaluated here
      LsSample e2;
      if ((rc = evaluate_slot(*opt.slot, true, nullptr, &e2)) != 0) break;
      if (!e2.value_is_valid) { finish(CERES_HIP_MINIMIZER_FAILURE, "Cost and jacobian evaluation failed."); --iteration; break; }
      opt.value = e2.value; opt.gradient_norm2 = e2.gradient_norm2; opt.gradient_max = e2.gradient_max;
    }
    cur = opt;
    cur_cost = opt.value;
    it.step_norm = std::sqrt(opt.step_norm2);
    const double x_norm = std::sqrt(opt.x_norm2);
    it.gradient_max_norm = cur.gradient_max; it.gradient_norm = std::sqrt(cur.gradient_norm2);
    it.cost_change = prev_cost - cur_cost;
    it.cost = cur_cost + fixed_cost;
    it.step_size = prev_step_size;
    it.line_search_function_evaluations = lss.num_function_evaluations;
    it.line_search_gradient_evaluations = lss.num_gradient_evaluations;
    it.line_search_iterations = lss.num_iterations;
    log_iter(it);
    S->num_line_search_steps += lss.num_iterations;
    ++S->num_successful_steps;
    // the termination tests in the reference's order: parameter, gradient, function tolerance
    if (it.step_norm <= o->parameter_tolerance * (x_norm + o->parameter_tolerance)) {
      finish(CERES_HIP_CONVERGENCE, ls_format("Parameter tolerance reached. Relative step_norm: %e <= %e.",
                                              it.step_norm / (x_norm + o->parameter_tolerance), o->parameter_tolerance));
      break;
    }
    if (it.gradient_max_norm <= o->gradient_tolerance) {
      finish(CERES_HIP_CONVERGENCE, ls_format("Gradient tolerance reached. Gradient max norm: %e <= %e", it.gradient_max_norm, o->gradient_tolerance));
      break;
    }
    if (std::fabs(it.cost_change) <= o->function_tolerance * std::fabs(prev_cost)) {
      finish(CERES_HIP_CONVERGENCE, ls_format("Function tolerance reached. |cost_change|/cost: %e <= %e", std::fabs(it.cost_change) / prev_cost,
                                              o->function_tolerance));
      break;
    }
  }
  S->num_iterations = iteration;
  S->num_line_search_direction_restarts = restarts;
  if (rc != 0) return bal_fail(p, rc);
  BAL_TRY(p, write_back());
  prev = LsSample(); cur = LsSample();
  return 0;
}

int ceres_hip_debug_line_search(const ceres_hip_line_search_options* o, ceres_hip_univariate_fn fn, void* user, double step_size_estimate,
                                double initial_cost, double initial_gradient, ceres_hip_line_search_result* out) {
  if (!o || !fn || !out) {
    g_create_error = "ceres_hip_debug_line_search: NULL options, function or result";
    return CERES_HIP_E_INVALID;
  }
  memset(out, 0, sizeof(*out));
  bool unsupported = false;
  ceres_hip_line_search_options v = *o;
  if (v.line_search_type == CERES_HIP_ARMIJO && v.line_search_direction_type != CERES_HIP_NONLINEAR_CONJUGATE_GRADIENT)
    v.line_search_direction_type = CERES_HIP_STEEPEST_DESCENT;   // (no direction here: only the line search's own rules apply)
  const std::string why = ls_validate(v, &unsupported);
  if (!why.empty() && !unsupported) {
    g_create_error = "ceres_hip_debug_line_search: " + why;
    return CERES_HIP_E_INVALID;
  }
  if (!(step_size_estimate >= 0.0)) {
    g_create_error = "ceres_hip_debug_line_search: step_size_estimate must be >= 0";
    return CERES_HIP_E_INVALID;
  }
  LsEvaluate eval = [&](double x, bool want_gradient, LsSample* s) -> int {
    *s = LsSample();
    s->x = x;
    s->vector_x_is_valid = true;
    double value = 0.0, gradient = 0.0;
    if (fn(x, want_gradient ? 1 : 0, &value, &gradient, user) != 0 || !std::isfinite(value)) return 0;
    s->value = value; s->value_is_valid = true;
    if (!want_gradient || !std::isfinite(gradient)) return 0;
    s->gradient = gradient; s->gradient_is_valid = true; s->vector_gradient_is_valid = true;
    return 0;
  };
  LsSample initial_position;
  initial_position.value = initial_cost; initial_position.gradient = initial_gradient;
  initial_position.value_is_valid = true; initial_position.gradient_is_valid = true; initial_position.vector_x_is_valid = true;
  LsSearchSummary S;
  ls_search(v.line_search_type, ls_search_options(v), eval, initial_position, step_size_estimate, &S);
  out->success = S.success ? 1 : 0;
  out->num_function_evaluations = S.num_function_evaluations;
  out->num_gradient_evaluations = S.num_gradient_evaluations;
  out->num_iterations = S.num_iterations;
  out->optimal_step_size = S.optimal_point.x;
  out->optimal_value = S.optimal_point.value;
  snprintf(out->error, sizeof(out->error), "%s", S.error.c_str());
  return 0;
}

int ceres_hip_debug_minimize_interpolating_polynomial(int32_t n, const double* x, const double* value, const int32_t* value_valid,
                                                      const double* gradient, const int32_t* gradient_valid, double x_min, double x_max,
                                                      double* optimal_x, double* optimal_value, double* coefficients_out) {
  if (n < 1 || n > 6 || !x || !value || !value_valid || !gradient || !gradient_valid || !optimal_x || !optimal_value) {
    g_create_error = "ceres_hip_debug_minimize_interpolating_polynomial: 1 to 6 samples and no NULL array";
    return CERES_HIP_E_INVALID;
  }
  std::vector<LsSample> samples(n);
  int nc = 0;
  for (int i = 0; i < n; ++i) {
    samples[i].x = x[i]; samples[i].value = value[i]; samples[i].gradient = gradient[i];
    samples[i].value_is_valid = value_valid[i] != 0; samples[i].gradient_is_valid = gradient_valid[i] != 0;
    nc += int(samples[i].value_is_valid) + int(samples[i].gradient_is_valid);
  }
  if (nc < 1 || nc > 6) {
    g_create_error = "ceres_hip_debug_minimize_interpolating_polynomial: 1 to 6 valid values and gradients";
    return CERES_HIP_E_INVALID;
  }
  std::vector<double> poly;
  ls_minimize_interpolating_polynomial(samples, x_min, x_max, optimal_x, optimal_value, &poly);
  if (coefficients_out) for (size_t i = 0; i < poly.size(); ++i) coefficients_out[i] = poly[i];
  return 0;
}

int ceres_hip_debug_lbfgs_direction(int64_t n, int32_t rank, int32_t use_scaling, int32_t num_updates, const double* delta_x,
                                    const double* delta_gradient, const double* gradient, double* direction_out, int32_t* accepted_out) {
  if (n <= 0 || rank <= 0 || num_updates < 0 || (num_updates > 0 && (!delta_x || !delta_gradient)) || !gradient || !direction_out) {
    g_create_error = "ceres_hip_debug_lbfgs_direction: bad arguments";
    return CERES_HIP_E_INVALID;
  }
  std::vector<void*> bufs;
  auto release = [&]() { for (void* q : bufs) (void)hipFree(q); };
  auto check = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    g_create_error = std::string("ceres_hip_debug_lbfgs_direction: ") + what + ": " + hipGetErrorString(e);
    release();
    return false;
  };
  auto alloc = [&](size_t bytes, void** out) {
    hipError_t e = hipMalloc(out, bytes ? bytes : 8);
    if (e == hipSuccess) bufs.push_back(*out);
    return e;
  };
  if (!check(hipSetDevice(0), "hipSetDevice")) return CERES_HIP_E_HIP;
  const size_t vb = sizeof(double) * size_t(n);
  LbfgsArgs L;
  L.n = n; L.rank = rank; L.use_scaling = use_scaling ? 1 : 0;
  double *hist = nullptr, *dx = nullptr, *dg = nullptr, *g = nullptr, *d = nullptr;
  void* q = nullptr;
  if (!check(alloc(2 * vb * size_t(rank), &q), "the history")) return CERES_HIP_E_HIP;
  hist = static_cast<double*>(q);
  L.S = hist; L.Y = hist + int64_t(rank) * n;
  if (!check(alloc(vb * size_t(std::max(num_updates, 1)), &q), "delta_x")) return CERES_HIP_E_HIP;
  dx = static_cast<double*>(q);
  if (!check(alloc(vb * size_t(std::max(num_updates, 1)), &q), "delta_gradient")) return CERES_HIP_E_HIP;
  dg = static_cast<double*>(q);
  if (!check(alloc(vb, &q), "gradient")) return CERES_HIP_E_HIP;
  g = static_cast<double*>(q);
  if (!check(alloc(vb, &q), "direction")) return CERES_HIP_E_HIP;
  d = static_cast<double*>(q);
  if (!check(alloc(sizeof(double) * size_t(rank), &q), "scalars")) return CERES_HIP_E_HIP;
  L.sy = static_cast<double*>(q);
  if (!check(alloc(sizeof(double) * size_t(rank), &q), "scalars")) return CERES_HIP_E_HIP;
  L.alpha = static_cast<double*>(q);
  if (!check(alloc(sizeof(double), &q), "scalars")) return CERES_HIP_E_HIP;
  L.scale = static_cast<double*>(q);
  if (!check(alloc(sizeof(int32_t) * size_t(rank), &q), "scalars")) return CERES_HIP_E_HIP;
  L.order = static_cast<int32_t*>(q);
  if (!check(alloc(sizeof(int32_t), &q), "scalars")) return CERES_HIP_E_HIP;
  L.count = static_cast<int32_t*>(q);
  if (!check(alloc(sizeof(double) * 4 * kMaxVecGrid, &q), "partials")) return CERES_HIP_E_HIP;
  L.parts = static_cast<double*>(q);
  if (!check(alloc(sizeof(int32_t) * size_t(std::max(num_updates, 1)), &q), "the log")) return CERES_HIP_E_HIP;
  L.accepted = static_cast<int32_t*>(q);
  hipStream_t st = nullptr;
  if (num_updates > 0) {
    if (!check(hipMemcpy(dx, delta_x, vb * size_t(num_updates), hipMemcpyHostToDevice), "copy")) return CERES_HIP_E_HIP;
    if (!check(hipMemcpy(dg, delta_gradient, vb * size_t(num_updates), hipMemcpyHostToDevice), "copy")) return CERES_HIP_E_HIP;
  }
  if (!check(hipMemcpy(g, gradient, vb, hipMemcpyHostToDevice), "copy")) return CERES_HIP_E_HIP;
  if (!check(LaunchLbfgsReset(L, st), "reset")) return CERES_HIP_E_HIP;
  for (int k = 0; k < num_updates; ++k)
    if (!check(LaunchLbfgsUpdate(L, 1.0, dx + int64_t(k) * n, dg + int64_t(k) * n, nullptr, k, st), "update")) return CERES_HIP_E_HIP;
  int nparts = 0;
  if (!check(LaunchLbfgsDirection(L, g, d, std::min(num_updates, rank), &nparts, st), "direction")) return CERES_HIP_E_HIP;
  if (!check(hipMemcpy(direction_out, d, vb, hipMemcpyDeviceToHost), "copy back")) return CERES_HIP_E_HIP;
  if (accepted_out && num_updates > 0 &&
      !check(hipMemcpy(accepted_out, L.accepted, sizeof(int32_t) * size_t(num_updates), hipMemcpyDeviceToHost), "copy back"))
    return CERES_HIP_E_HIP;
  release();
  return 0;
}

}  // extern "C"
