// Dogleg trust region of the BAL front end: Solver::Options::trust_region_strategy_type = DOGLEG and dogleg_type
// (include/ceres/solver.h), bundle_adjuster's --trust_region_strategy=dogleg --dogleg=traditional_dogleg|subspace_dogleg.
// Textually included by bal_frontend.inc.
//
//   DoglegStrategy::ComputeStep       I/dogleg_strategy.cc:79-174   dogleg_step (below)
//   ComputeGaussNewtonStep            :517-616   lm_step_loaded with radius = 1 / mu: its D = sqrt(clamp(d) / radius) is Ceres'
//                                                diagonal * sqrt(mu); its (negated) solution is gn / diagonal
//   ComputeTraditionalDoglegStep      :201-264   dl_traditional
//   ComputeSubspaceModel              :648-719   dl_subspace_model, from 2x2 Gram matrices (below)
//   ComputeSubspaceDoglegStep         :266-345   dl_subspace
//   FindMinimumOnTrustRegionBoundary  :419-515   dl_boundary_minimum; the quartic's roots: FindPolynomialRoots, I/polynomial.cc:187-246
//   StepAccepted / StepRejected / StepIsInvalid  :618-646, in ceres_hip_bal_minimize
//
// Every step lies in span{a, b}, a = gradient / diagonal and b = gn / diagonal, so it is held as two coefficients (u, v): step =
// u a + v b on the device, and u gradient + v gn in the strategy's scaled space.  One pass over J per Jacobian (kernels_dogleg.hip)
// gives |Ja|^2, Ja.Jb, |Jb|^2, Ja.f, Jb.f, from which the Cauchy point, the subspace model and the model cost change of every step
// follow on the host; a rejected step (reuse) costs no pass at all.  The Gauss-Newton solve forms no model cost change of its own
// (lm_step_loaded's no_model_cost: no kJx pass, no back-substitution partials).  A fresh step synchronises with the host twice: once for the
// solve's status and finite check (which decide a mu retry), once for the partial sums of the two kernels below.  Ceres forms J step
// explicitly for the model cost change (I/trust_region_minimizer.cc:420-438); the scalar form -(u Ja + v Jb).(f + (u Ja + v Jb) / 2)
// agrees with it up to rounding.

struct DoglegState {
  int type = CERES_HIP_TRADITIONAL_DOGLEG;
  double radius = 0.0, mu = 1e-8, step_norm = 0.0;   // kMinMu, I/dogleg_strategy.cc:50-77
  bool reuse = false;
  // of the last fresh ComputeStep
  double gg = 0, ggn = 0, nn = 0;                    // |gradient|^2, gradient.gn, |gn|^2 (scaled space)
  double jaa = 0, jab = 0, jbb = 0, jaf = 0, jbf = 0;
  double alpha = 0;                                  // the Cauchy point is -alpha gradient
  // the subspace: basis Q = [gradient gn] T (T: 2x2, column-major), model 1/2 x'Bx + g'x
  bool one_dim = false;
  double T[4] = {0, 0, 0, 0}, sB[4] = {0, 0, 0, 0}, sg[2] = {0, 0};
};

namespace {

constexpr double kDoglegMaxMu = 1.0, kDoglegMinMu = 1e-8, kDoglegMuIncrease = 10.0;

// The real parts of all roots of c[0] y^d + ... + c[d] (d = size - 1 <= 4), after dropping leading zero coefficients, as
// FindPolynomialRoots returns them: linear and quadratic polynomials in closed form (the quadratic's stable form), cubics and quartics
// by Aberth-Ehrlich iteration on the monic polynomial (simultaneous Newton steps, each corrected by the other roots' pull).  Returns the
// number of roots, -1 if a coefficient is not finite.
int dl_poly_real_parts(const double* coef, int size, double* re) {
  for (int i = 0; i < size; ++i) if (!std::isfinite(coef[i])) return -1;
  int i0 = 0;
  while (i0 < size - 1 && coef[i0] == 0.0) ++i0;
  const double* c = coef + i0;
  const int deg = size - 1 - i0;
  if (deg == 0) return 0;
  if (deg == 1) { re[0] = -c[1] / c[0]; return 1; }
  if (deg == 2) {
    const double a = c[0], b = c[1], cc = c[2];
    const double D = b * b - 4 * a * cc;
    const double sD = std::sqrt(std::fabs(D));
    if (D >= 0) {
      if (b >= 0) { re[0] = (-b - sD) / (2.0 * a); re[1] = (2.0 * cc) / (-b - sD); }
      else { re[0] = (2.0 * cc) / (-b + sD); re[1] = (-b + sD) / (2.0 * a); }
    } else {
      re[0] = re[1] = -b / (2.0 * a);
    }
    return 2;
  }
  using cd = std::complex<double>;
  double m[5];
  for (int k = 0; k <= deg; ++k) m[k] = c[k] / c[0];
  // start on a circle that holds every root (Fujiwara's bound), off the real axis
  double bound = 0.0;
  for (int k = 1; k <= deg; ++k) bound = std::max(bound, std::pow(std::fabs(m[k]), 1.0 / k));
  bound = 2.0 * std::max(bound, std::numeric_limits<double>::min());
  cd z[4];
  for (int k = 0; k < deg; ++k) z[k] = std::polar(bound, 2.0 * M_PI * k / deg + 0.4);
  const double eps = std::numeric_limits<double>::epsilon();
  for (int it = 0; it < 500; ++it) {
    bool moved = false;
    for (int k = 0; k < deg; ++k) {
      cd pv = 1.0, dp = 0.0;
      for (int j = 1; j <= deg; ++j) { dp = dp * z[k] + pv; pv = pv * z[k] + m[j]; }
      if (pv == 0.0) continue;   // an exact root
      if (dp == 0.0) { z[k] *= cd(1.0 + 1e-8, 1e-8); moved = true; continue; }   // (a stationary point: nudge it)
      const cd w = pv / dp;
      cd pull = 0.0;
      for (int j = 0; j < deg; ++j) if (j != k) pull += 1.0 / (z[k] - z[j]);
      const cd step = w / (1.0 - w * pull);
      z[k] -= step;
      if (std::abs(step) > 4.0 * eps * std::abs(z[k])) moved = true;
    }
    if (!moved) break;
  }
  for (int k = 0; k < deg; ++k) re[k] = z[k].real();
  return deg;
}

// x = -(M)^-1 g for a 2x2 M by LU with partial pivoting (ComputeSubspaceStepFromRoot, :448-454)
void dl_solve2(const double M[4], const double g[2], double x[2]) {
  double a00 = M[0], a01 = M[1], a10 = M[2], a11 = M[3], g0 = g[0], g1 = g[1];
  if (std::fabs(a10) > std::fabs(a00)) { std::swap(a00, a10); std::swap(a01, a11); std::swap(g0, g1); }
  const double l = a10 / a00;
  const double y1 = (g1 - l * g0) / (a11 - l * a01);
  const double y0 = (g0 - a01 * y1) / a00;
  x[0] = -y0; x[1] = -y1;
}

double dl_model(const double B[4], const double g[2], const double x[2]) {   // EvaluateSubspaceModel, :456-460
  return 0.5 * (x[0] * (B[0] * x[0] + B[1] * x[1]) + x[1] * (B[2] * x[0] + B[3] * x[1])) + g[0] * x[0] + g[1] * x[1];
}

// FindMinimumOnTrustRegionBoundary (:473-515) and the first-order check of ComputeSubspaceDoglegStep (:318-336): 0, or
// CERES_HIP_DOGLEG_NO_ROOT / CERES_HIP_DOGLEG_COSINE — the two cases where the strategy takes the traditional step instead
int dl_boundary_minimum(const double B[4], const double g[2], double radius, double x[2]) {
  x[0] = x[1] = 0.0;
  // the quartic of MakePolynomialForBoundaryConstrainedProblem (:419-446)
  const double detB = B[0] * B[3] - B[2] * B[1], trB = B[0] + B[3], r2 = radius * radius;
  const double adj[4] = {B[3], -B[1], -B[2], B[0]};
  const double ag0 = adj[0] * g[0] + adj[1] * g[1], ag1 = adj[2] * g[0] + adj[3] * g[1];
  const double gag = g[0] * ag0 + g[1] * ag1;
  const double poly[5] = {r2, 2.0 * r2 * trB, r2 * (trB * trB + 2.0 * detB) - (g[0] * g[0] + g[1] * g[1]), -2.0 * (gag - r2 * detB * trB),
                          r2 * detB * detB - (ag0 * ag0 + ag1 * ag1)};
  double roots[4];
  const int nr = dl_poly_real_parts(poly, 5, roots);
  double best = std::numeric_limits<double>::max();
  bool valid = false;
  for (int i = 0; i < nr; ++i) {
    const double M[4] = {B[0] + roots[i], B[1], B[2], B[3] + roots[i]};
    double xi[2];
    dl_solve2(M, g, xi);
    const double nx = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1]);
    if (nx > 0) {
      const double xs[2] = {radius / nx * xi[0], radius / nx * xi[1]};
      const double f = dl_model(B, g, xs);
      valid = true;
      if (f < best) { best = f; x[0] = xi[0]; x[1] = xi[1]; }
    }
  }
  if (!valid) return CERES_HIP_DOGLEG_NO_ROOT;
  const double gm[2] = {B[0] * x[0] + B[1] * x[1] + g[0], B[2] * x[0] + B[3] * x[1] + g[1]};
  const double cosine = -(x[0] * gm[0] + x[1] * gm[1]) / (std::sqrt(x[0] * x[0] + x[1] * x[1]) * std::sqrt(gm[0] * gm[0] + gm[1] * gm[1]));
  if (cosine < 0.99) return CERES_HIP_DOGLEG_COSINE;
  return 0;
}

// ComputeTraditionalDoglegStep: (u, v) of the step u gradient + v gn; sets step_norm
void dl_traditional(DoglegState& st, double* u, double* v) {
  const double gnorm = std::sqrt(st.gg), gn_norm = std::sqrt(st.nn), r = st.radius;
  if (gn_norm <= r) { *u = 0.0; *v = 1.0; st.step_norm = gn_norm; return; }
  if (gnorm * st.alpha >= r) { *u = -(r / gnorm); *v = 0.0; st.step_norm = r; return; }
  const double b_dot_a = -st.alpha * st.ggn;
  const double a_sq = std::pow(st.alpha * gnorm, 2.0);
  const double bma = a_sq - 2 * b_dot_a + std::pow(gn_norm, 2);
  const double c = b_dot_a - a_sq;
  const double d = std::sqrt(c * c + bma * (std::pow(r, 2.0) - a_sq));
  const double beta = (c <= 0) ? (d - c) / bma : (r * r - a_sq) / (d + c);
  *u = -st.alpha * (1.0 - beta);
  *v = beta;
  st.step_norm = std::sqrt((*u) * (*u) * st.gg + 2.0 * (*u) * (*v) * st.ggn + (*v) * (*v) * st.nn);
}

// ComputeSubspaceModel from the Gram matrices of [gradient, gn] and [J a, J b].  The basis is the column-pivoting QR of [gradient, gn]
// (ColPivHouseholderQR): the longer column first (the gradient on a tie), R from the Gram matrix, and the rank rule this project uses
// for Eigen's default threshold: |R_ii| > 2 eps max_j |R_jj|.  Then Q = [gradient gn] T, subspace_g = Q' gradient and subspace_B =
// (J D^-1 Q)'(J D^-1 Q) = T' [Ja Jb]'[Ja Jb] T.  Returns false for rank 0 (the step is a FAILURE).
// R_22 comes from the Gram matrix, sqrt(|c_2|^2 - R_12^2), and that difference carries an absolute error of a few eps |c_2|^2: below
// kDoglegGramFloor |c_2| = 4 sqrt(eps) |c_2| (columns within ~6e-8 rad of parallel) R_22 is rounding noise, and the second basis vector
// built from it would not be orthogonal to the first.  Such a basis counts as rank 1 here (the 1-D step along the gradient), where a
// Householder QR could still see rank 2; in that case the subspace is 1-D to within 6e-8 anyway.
constexpr double kDoglegGramFloor = 5.960464477539063e-08;   // 4 sqrt(eps)
bool dl_subspace_model(DoglegState& st) {
  const int piv = st.nn > st.gg ? 1 : 0;
  const double n0 = piv ? st.nn : st.gg, n1 = piv ? st.gg : st.nn;
  const double r11 = std::sqrt(n0);
  const double r12 = r11 > 0 ? st.ggn / r11 : 0.0;
  double r22 = std::sqrt(std::max(0.0, n1 - r12 * r12));
  if (r22 <= kDoglegGramFloor * std::sqrt(n1)) r22 = 0.0;
  const double thr = 2.0 * std::numeric_limits<double>::epsilon() * std::max(r11, r22);
  const int rank = (r11 > thr) + (r22 > thr);
  if (rank == 0) return false;
  st.one_dim = rank == 1;
  if (st.one_dim) return true;
  // T columns in the (gradient, gn) coordinates: q1 = e_piv / r11, q2 = (e_other - (r12 / r11) e_piv) / r22
  double T[4] = {0, 0, 0, 0};   // column-major: T[0], T[1] = q1; T[2], T[3] = q2
  T[piv] = 1.0 / r11;
  T[2 + (1 - piv)] = 1.0 / r22;
  T[2 + piv] = -(r12 / r11) / r22;
  for (int k = 0; k < 4; ++k) st.T[k] = T[k];
  const double gq[2] = {st.gg, st.ggn};   // [gradient gn]' gradient
  st.sg[0] = T[0] * gq[0] + T[1] * gq[1];
  st.sg[1] = T[2] * gq[0] + T[3] * gq[1];
  const double H[4] = {st.jaa, st.jab, st.jab, st.jbb};
  double HT[4];   // H T, column-major
  for (int j = 0; j < 2; ++j) {
    HT[2 * j] = H[0] * T[2 * j] + H[1] * T[2 * j + 1];
    HT[2 * j + 1] = H[2] * T[2 * j] + H[3] * T[2 * j + 1];
  }
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) st.sB[2 * i + j] = T[2 * i] * HT[2 * j] + T[2 * i + 1] * HT[2 * j + 1];
  return true;
}

// ComputeSubspaceDoglegStep
void dl_subspace(DoglegState& st, double* u, double* v) {
  const double gn_norm = std::sqrt(st.nn), r = st.radius;
  if (gn_norm <= r) { *u = 0.0; *v = 1.0; st.step_norm = gn_norm; return; }
  if (st.one_dim) { *u = -(r / std::sqrt(st.gg)); *v = 0.0; st.step_norm = r; return; }
  double x[2];
  if (dl_boundary_minimum(st.sB, st.sg, r, x) != 0) { dl_traditional(st, u, v); return; }
  *u = st.T[0] * x[0] + st.T[2] * x[1];
  *v = st.T[1] * x[0] + st.T[3] * x[1];
  st.step_norm = r;
}

// DoglegStrategy::ComputeStep on the loaded (scaled) Jacobian, whose J^T f is in p->d_grad: the step into d_step and, in *lr, the
// linear solver's summary (0 iterations for a reused step), the model cost change and step_is_finite; *solves = the linear solves run.
int dogleg_step(ceres_hip_bal* p, DoglegState& st, const ceres_hip_minimizer_options* o, bool& reuse_diagonal, double* d_step,
                ceres_hip_lm_result* lr, int* solves) {
  ceres_hip_solver* s = p->s;
  hipStream_t stream = s->stream;
  memset(lr, 0, sizeof(*lr));
  *solves = 0;
  if (!st.reuse) {
    st.reuse = true;
    lr->linear_solver.termination_type = CERES_HIP_FAILURE;
    // ComputeGaussNewtonStep: tolerances 0 (DENSE_SCHUR solves exactly), D = diagonal sqrt(mu); a failed or non-finite solve raises mu
    while (st.mu < kDoglegMaxMu) {
      ceres_hip_lm_options lo{};
      lo.radius = 1.0 / st.mu; lo.min_diagonal = o->min_lm_diagonal; lo.max_diagonal = o->max_lm_diagonal; lo.eta = 0.0;
      lo.reuse_diagonal = reuse_diagonal ? 1 : 0;
      // (no_model_cost: the LM step forms no model cost change of its own — no pass over J, the Gram pass below gives every step's)
      TRY(lm_step_loaded(s, &lo, p->d_dl_b, lr, true));
      HIP_TRY(s, hipStreamSynchronize(stream));
      ++*solves;
      reuse_diagonal = true;
      const int term = lr->linear_solver.termination_type;
      if (term == CERES_HIP_FATAL_ERROR) return 0;
      if (term == CERES_HIP_FAILURE || !lr->step_is_finite) {
        st.mu *= kDoglegMuIncrease;
        lr->linear_solver.termination_type = CERES_HIP_FAILURE;
        continue;
      }
      break;
    }
    lr->step_is_finite = 0;
    lr->model_cost_change = 0.0;
    if (lr->linear_solver.termination_type == CERES_HIP_FAILURE) return 0;
    // the strategy's vectors and the pass over J; s->lm_diag holds the clamped column norms lm_step_loaded formed
    int n3 = 0, n5 = 0;
    double* parts = nullptr;   // (both kernels interleave their scalars: three, then five to a workgroup)
    TRY(bal_parts_room(p, 3 * kDoglegGrid, &parts));
    HIP_TRY(s, LaunchDoglegPrep(s->lm_diag, p->d_grad, p->d_dl_b, p->d_dl_a, p->n_t, parts, &n3, stream));
    const PartialSet set3 = p->parts.take(3 * n3);
    TRY(bal_parts_room(p, 5 * kDoglegGrid, &parts));
    HIP_TRY(s, LaunchJacobianGram(s->G, s->values, p->d_dl_a, p->d_dl_b, s->b, parts, &n5, stream));
    const PartialSet set5 = p->parts.take(5 * n5);
    TRY(bal_parts_collect(p));
    const double *h3 = p->parts.host(set3), *h5 = p->parts.host(set5);
    double v3[3] = {0, 0, 0}, v5[5] = {0, 0, 0, 0, 0};
    for (int q = 0; q < n3; ++q) for (int k = 0; k < 3; ++k) v3[k] += h3[3 * q + k];   // fixed order: deterministic
    for (int q = 0; q < n5; ++q) for (int k = 0; k < 5; ++k) v5[k] += h5[5 * q + k];
    st.gg = v3[0]; st.ggn = v3[1]; st.nn = v3[2];
    st.jaa = v5[0]; st.jab = v5[1]; st.jbb = v5[2]; st.jaf = v5[3]; st.jbf = v5[4];
    st.alpha = st.gg / st.jaa;   // ComputeCauchyPoint, :185-199
    if (st.type == CERES_HIP_SUBSPACE_DOGLEG && !dl_subspace_model(st)) {
      lr->linear_solver.termination_type = CERES_HIP_FAILURE;
      return 0;
    }
  } else {
    lr->linear_solver.termination_type = CERES_HIP_SUCCESS;   // (a reused step: no solve, 0 iterations)
  }
  double u = 0, v = 0;
  if (st.type == CERES_HIP_SUBSPACE_DOGLEG) dl_subspace(st, &u, &v);
  else dl_traditional(st, &u, &v);
  HIP_TRY(s, LaunchAxpby(u, p->d_dl_a, v, p->d_dl_b, d_step, p->n_t, stream));
  lr->model_cost_change = -(u * st.jaf + v * st.jbf) - 0.5 * (u * u * st.jaa + 2.0 * u * v * st.jab + v * v * st.jbb);
  lr->step_is_finite = 1;
  return 0;
}

// the strategy's device vectors (once per handle: the solver's allocations, freed with it)
int dogleg_alloc(ceres_hip_bal* p) {
  if (p->d_dl_a) return 0;
  ceres_hip_solver* s = p->s;
  if (dev_alloc(s, &p->d_dl_a, size_t(p->n_t)) || dev_alloc(s, &p->d_dl_b, size_t(p->n_t))) {
    p->d_dl_a = nullptr;
    return CERES_HIP_E_HIP;
  }
  return 0;
}

}  // namespace

extern "C" {

int ceres_hip_bal_set_trust_region_strategy(ceres_hip_bal* p, int32_t strategy, int32_t dogleg_type) {
  auto refuse = [&](int code, const std::string& why) {
    (p ? p->err : g_create_error) = "ceres_hip_bal_set_trust_region_strategy: " + why;
    return code;
  };
  if (!p) return refuse(CERES_HIP_E_INVALID, "NULL problem handle");
  if (strategy != CERES_HIP_LEVENBERG_MARQUARDT && strategy != CERES_HIP_DOGLEG)
    return refuse(CERES_HIP_E_INVALID, "unknown strategy " + std::to_string(strategy));
  if (strategy == CERES_HIP_DOGLEG) {
    if (dogleg_type != CERES_HIP_TRADITIONAL_DOGLEG && dogleg_type != CERES_HIP_SUBSPACE_DOGLEG)
      return refuse(CERES_HIP_E_INVALID, "unknown dogleg_type " + std::to_string(dogleg_type));
    const int t = p->s->opt.solver_type;
    if (t == CERES_HIP_ITERATIVE_SCHUR || t == CERES_HIP_CGNR)   // Solver::Options::IsValid, I/solver.cc:431-438
      return refuse(CERES_HIP_E_INVALID,
                    "DOGLEG only supports exact factorization based linear solvers. If you want to use an iterative solver please use "
                    "LEVENBERG_MARQUARDT as the trust_region_strategy_type");
    if (p->s->world > 1) return refuse(CERES_HIP_E_UNSUPPORTED, "DOGLEG is not supported on sharded handles");
    p->dogleg_type = dogleg_type;
  }
  p->tr_strategy = strategy;
  return 0;
}

int ceres_hip_debug_dogleg_subspace_minimum(const double* B, const double* g, double radius, double* x) {
  if (!B || !g || !x) return CERES_HIP_E_INVALID;
  return dl_boundary_minimum(B, g, radius, x);
}

}  // extern "C"
