// mtg_objective_lane.h -- per-lane algorithm of the nonlinear time objective's soft-constraint term.
//
// What it replaces, per segment: the inner loop of PolynomialOptimization<N>::computeMaximumOfMagnitude
// (impl/polynomial_optimization_linear_impl.h:466-497) as called once per constrained derivative by
// PolynomialOptimizationNonLinear<N>::evaluateMaximumMagnitudeAsSoftConstraint (impl/polynomial_optimization_nonlinear_impl.h:
// 767-795): the LARGEST magnitude ||p^(der)(t)|| over the segment, all dimensions.  The reference's candidates are the segment
// start, the real roots of the magnitude derivative inside the segment and the end of the LAST segment; here every segment also
// evaluates its own end, which is the next segment's start for the derivatives this entry accepts (1 .. N/2 - 1: continuous
// across vertices), so the maximum over the trajectory is the same set's.  One read of the segment's D x N coefficients serves
// every constrained derivative; the searches run one after the other through real_roots_unit of mtg_extrema_lane.h on the same
// two root buffers.  Minima and extremum times are not tracked.
// The cost arithmetic of the callers (:556-615, :660-742, :745-763) is here too, so that device and host form one expression.
// Same code runs on the device (mtg_objective.hip) and on the host (mtg_objective_host.cpp).
#pragma once

#include "mtg_segment_lane.h"

namespace mtgo {

constexpr int kMaxConstraints = 4;   // MTG_MAX_MAGNITUDE_CONSTRAINTS
constexpr int kMinCoeffs = 4;        // derivative 1 needs N / 2 - 1 >= 1
constexpr int kMaxDimension = 4;     // the lane keeps D x N coefficients in registers

struct Constraints {   // ordered as the caller added them (addMaximumMagnitudeConstraint)
  int n;
  int derivative[kMaxConstraints];
  double value[kMaxConstraints];
};

// what the entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         const Constraints& c) {
  if (!mtgs::shape_ok(n_coeffs, kMinCoeffs, n_segments, dimension, kMaxDimension, batch, ts_b, ts_k)) return false;
  if (c.n < 0 || c.n > kMaxConstraints) return false;
  for (int q = 0; q < c.n; ++q)
    if (c.derivative[q] < 1 || c.derivative[q] > n_coeffs / 2 - 1 || !(c.value[q] > 0.0)) return false;
  return true;
}

// || p^(DER)(t) || over DC dimensions
template <int NC, int DC, int DER>
MTGX_HD double magnitude_at(const double (&p)[DC][NC], double t) {
  return mtgs::magnitude_at<NC, DC, DER, false>(p, nullptr, t);
}

// largest ||p^(DER)|| over [0, T]: start, interior critical points, end
template <int NC, int DC, int DER, class Roots>
MTGX_HD double magnitude_max(const double (&p)[DC][NC], double T, Roots& roots) {
  constexpr int L = 2 * (NC - DER) - 2;
  double g[L];
  mtgs::magnitude_derivative<NC, DC, DER, false>(p, nullptr, T, g);
  int base = 0;
  const int cnt = mtgx::real_roots_unit<L, Roots>(g, roots, base);
  double best = fmax(magnitude_at<NC, DC, DER>(p, 0.0), magnitude_at<NC, DC, DER>(p, T));
  for (int i = 0; i < cnt; ++i) best = fmax(best, magnitude_at<NC, DC, DER>(p, roots[base + i] * T));
  // A NaN or Inf among the coefficients this derivative reads leaves no finite candidate: each value is NaN (fma(inf, 0, x) at
  // t = 0) or +inf, and fmax drops a NaN beside an +inf.  Both are reported as NaN -- "no maximum" -- which the callers' folds
  // keep (include/mtg_hip.h); so is a magnitude that overflows from finite coefficients.
  return best < INFINITY ? best : NAN;
}

// One derivative order of one segment: searched if any constraint names it, and reported to each of them
template <int NC, int DC, int DER, class Roots, class Emit>
MTGX_HD void search_order(const double (&p)[DC][NC], double T, const Constraints& con, Roots& roots, Emit& emit) {
  if constexpr (DER <= NC / 2 - 1) {
    bool wanted = false;
#pragma unroll
    for (int q = 0; q < kMaxConstraints; ++q) wanted = wanted || (q < con.n && con.derivative[q] == DER);
    if (!wanted) return;
    const double m = magnitude_max<NC, DC, DER, Roots>(p, T, roots);
#pragma unroll
    for (int q = 0; q < kMaxConstraints; ++q)
      if (q < con.n && con.derivative[q] == DER) emit(q, m);
  }
}

// One segment.  c = [D][N] coefficients (increasing powers), N <= NC and D <= DC (the tails are zero-padded: a dimension of
// zeros adds nothing to the magnitude or to its derivative), T = segment time.  roots: roots_len(NC) elements.
// emit(q, m): m = maximum of constraint q's derivative over the segment.  The searches are laid out one derivative ORDER after
// the other, straight-line: a loop over the constraints with a switch on the order let the compiler hoist every order's
// scaled coefficient tables in front of the loop, side by side, and spill them (2.4 KB of scratch per lane at N = 10).
template <int NC, int DC, class Roots, class Emit>
MTGX_HD void segment_maxima(const double* c, int N, int D, double T, const Constraints& con, Roots& roots, Emit&& emit) {
  double p[DC][NC];
  mtgs::load_padded(c, N, D, p);
  search_order<NC, DC, 1, Roots>(p, T, con, roots, emit);
  search_order<NC, DC, 2, Roots>(p, T, con, roots, emit);
  search_order<NC, DC, 3, Roots>(p, T, con, roots, emit);
  search_order<NC, DC, 4, Roots>(p, T, con, roots, emit);
  search_order<NC, DC, 5, Roots>(p, T, con, roots, emit);
}

// the two root buffers of the largest search (derivative 1: g has 2 (NC - 1) - 2 coefficients)
constexpr int roots_len(int nc) { return 2 * (2 * nc - 5); }

// ---- the callers' arithmetic -------------------------------------------------------------------------------------------
// time-cost kinds: NonlinearOptimizationParameters::TimeAllocMethod (polynomial_optimization_nonlinear.h)
constexpr int kSquaredTime = 0, kRichterTime = 1, kMellingerOuterLoop = 2, kSquaredTimeAndConstraints = 3,
              kRichterTimeAndConstraints = 4;
MTGX_HD bool is_richter(int kind) { return kind == kRichterTime || kind == kRichterTimeAndConstraints; }

MTGX_HD double time_cost(int kind, double time_penalty, double total_time) {   // :576-585, :703-712
  return is_richter(kind) ? total_time * time_penalty : total_time * total_time * time_penalty;
}

// one term of evaluateMaximumMagnitudeAsSoftConstraint (:780-786)
MTGX_HD double soft_term(double maximum, double limit, double weight, double maximum_cost) {
  const double abs_violation = maximum - limit;
  const double relative_violation = abs_violation / limit;
  return fmin(maximum_cost, exp(relative_violation * weight));
}

}  // namespace mtgo
