// mtg_feasibility_lane.h -- per-lane algorithm of the batched analytic input-feasibility check.
//
// What it replaces, per segment: FeasibilityAnalytic::checkInputFeasibility(const Segment&)
// (mav_trajectory_generation_ros/src/feasibility_analytic.cpp:42-233): thrust limits, velocity limit, yaw rate / yaw
// acceleration limits and Mueller's recursive roll/pitch-rate bound, first failing check decides.  Three magnitude root
// searches (thrust = acceleration + g, velocity, jerk over dimensions 0-2) and two single-axis ones (yaw) on ONE read of the
// segment's coefficients, all through real_roots_unit of mtg_extrema_lane.h; the candidate lists of thrust and jerk are kept
// (time, value) for the section selection of the roll/pitch recursion.  A check whose limit is absent is not computed.
//
// The recursion (:177-233) has only two outcomes, feasible and indeterminable, and returns the first that is not feasible:
// the verdict is "a section shorter than min_section_time_s can be reached by splitting only sections whose bound exceeds the
// limit", whatever the order of the visits.  The walk below is the reference's depth-first order without a stack: a section is
// (depth, path bits) and its end points are recomputed from [0, T] by the reference's own (t1 + t2) / 2 -- NOT as T j / 2^d,
// which rounds differently.
// Same code runs on the device (mtg_feasibility.hip) and on the host (mtg_feasibility_host.cpp).
#pragma once

#include "mtg_segment_lane.h"

namespace mtgf {

// result codes: enum InputFeasibilityResult (feasibility_base.h:34-50)
constexpr int kFeasible = 0, kIndeterminable = 1, kThrustHigh = 2, kThrustLow = 3, kVelocity = 4, kRollPitchRates = 5,
              kYawRates = 6, kYawAcc = 7;
constexpr int kMinCoeffs = 5;    // the jerk polynomial is at least linear: its squared magnitude has a derivative to search
constexpr int kNumBounds = 6;    // thrust min, thrust max, velocity max, top-level roll/pitch bound, |yaw rate| max, |yaw acc| max

struct Limits {   // NaN = absent (InputConstraints::hasConstraint false); values are magnitudes (addConstraint stores |value|)
  double f_min, f_max, v_max, omega_xy_max, omega_z_max, omega_z_dot_max;
  double min_section_time_s;
  double gravity;   // thrust = || a + (0, 0, gravity) ||
};
MTGX_HD bool has(double limit) { return limit == limit; }

// what both entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         const Limits& lim) {
  return mtgs::shape_ok(n_coeffs, kMinCoeffs, n_segments, dimension, 32, batch, ts_b, ts_k) &&
         lim.min_section_time_s == lim.min_section_time_s && lim.gravity == lim.gravity;
}

// base(DER, i) of polynomial.cpp:145-160 as a compile-time-foldable product
MTGX_HD double ff(int i, int der) { return mtgx::falling_factorial(i, der); }

// || p^(DER)(t) + off || over dimensions 0-2
template <int NC, int DER>
MTGX_HD double magnitude3_at(const double (&p)[3][NC], const double (&off)[3], double t) {
  return mtgs::magnitude_at<NC, 3, DER, true>(p, off, t);
}

// real roots in tau = t / T in [0, 1] of the derivative of || p^(DER) + off ||^2: count returned, ascending at roots[base + i]
template <int NC, int DER, class Roots>
MTGX_HD int magnitude3_roots(const double (&p)[3][NC], const double (&off)[3], double T, Roots& roots, int& base) {
  double g[2 * (NC - DER) - 2];
  mtgs::magnitude_derivative<NC, 3, DER, true>(p, off, T, g);
  return mtgx::real_roots_unit<2 * (NC - DER) - 2, Roots>(g, roots, base);
}

// max(|min|, |max|) of y^(DER) over [0, T] (Polynomial::computeMinMax: end points + real roots of y^(DER+1))
template <int NC, int DER, class Roots>
MTGX_HD double axis_abs_max(const double (&y)[NC], double T, Roots& roots) {
  constexpr int L = NC - DER - 1;   // coefficient count of y^(DER+1)
  double g[L];
  double tp = 1.0;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    g[j] = y[j + DER + 1] * ff(j + DER + 1, DER + 1) * tp;
    tp *= T;
  }
  int base = 0;
  const int cnt = mtgx::real_roots_unit<L, Roots>(g, roots, base);
  double best = 0.0;
  for (int i = -2; i < cnt; ++i) {
    const double t = i == -2 ? 0.0 : (i == -1 ? T : roots[base + i] * T);
    double r = 0.0;
#pragma unroll
    for (int k = NC - 1; k >= DER; --k) r = fma(r, t, ff(k, DER) * y[k]);
    best = fmax(best, fabs(r));
  }
  return best;
}

// Mueller's bound of the section [t1, t2] from the candidates whose time lies inside it (segment.cpp:161-185: the section's
// own end points are not evaluated).  A section without candidates gives sqrt(lowest / max) = NaN, and NaN > limit is false.
template <class Cand>
MTGX_HD double section_bound(double t1, double t2, double T, double f0, double fT, double j0, double jT, Cand& fc, int nf,
                             Cand& jc, int nj) {
  double f_min = DBL_MAX, j_max = -DBL_MAX;
  if (!(0.0 < t1 || 0.0 > t2)) { f_min = fmin(f_min, f0); j_max = fmax(j_max, j0); }
  if (!(T < t1 || T > t2)) { f_min = fmin(f_min, fT); j_max = fmax(j_max, jT); }
  for (int i = 0; i < nf; ++i) {
    const double t = fc[2 * i];
    if (!(t < t1 || t > t2)) f_min = fmin(f_min, fc[2 * i + 1]);
  }
  for (int i = 0; i < nj; ++i) {
    const double t = jc[2 * i];
    if (!(t < t1 || t > t2)) j_max = fmax(j_max, jc[2 * i + 1]);
  }
  return f_min > 1.0e-6 ? sqrt(j_max / f_min) : DBL_MAX;   // (divide-by-zero protection, :201-205)
}

// recursiveRollPitchFeasibility over [0, T]; top = the bound of [0, T] itself (NaN if T is shorter than a section)
template <class Cand>
MTGX_HD int roll_pitch_sections(double T, double f0, double fT, double j0, double jT, Cand& fc, int nf, Cand& jc, int nj,
                                double limit, double min_section, double& top) {
  top = NAN;
  unsigned long long path = 0;   // bit l (from the top): 0 = first half, 1 = second half
  int depth = 0;
  for (;;) {
    double t1 = 0.0, t2 = T;
    for (int l = depth - 1; l >= 0; --l) {
      const double t_half = (t1 + t2) / 2;
      if ((path >> l) & 1ull) t1 = t_half; else t2 = t_half;
    }
    if (t2 - t1 < min_section) return kIndeterminable;
    const double bound = section_bound(t1, t2, T, f0, fT, j0, jT, fc, nf, jc, nj);
    if (depth == 0) top = bound;
    if (bound > limit) {
      if (depth >= 62) return kIndeterminable;   // (min_section_time_s == 0: the reference recurses without end)
      path <<= 1;
      ++depth;
      continue;
    }
    while (depth > 0 && (path & 1ull)) { path >>= 1; --depth; }   // this section is feasible: on to the next one
    if (depth == 0) return kFeasible;
    path |= 1ull;
  }
}

// One segment.  c = [D][N] coefficients (increasing powers), N <= NC (the tail is zero-padded: identically-zero leading levels
// of the derivative chains fall through), T = segment time.  roots: 2 * (2 * NC - 5) elements (the velocity search's two
// buffers, the largest); cand: 2 * (2 * NC - 7) + 2 * (2 * NC - 9) elements ((time, value) of the thrust roots, then of the
// jerk roots).  bounds[kNumBounds]: NaN where not computed.
template <int NC, class Roots, class Cand>
MTGX_HD int segment_check(const double* c, int N, int D, double T, const Limits& lim, Roots& roots, Cand& cand, Cand& cand_jerk,
                          double (&bounds)[kNumBounds]) {
#pragma unroll
  for (int q = 0; q < kNumBounds; ++q) bounds[q] = NAN;
  if (!(D == 3 || D == 4)) return kIndeterminable;
  double p[3][NC];
  mtgs::load_padded(c, N, D, p);
  const double zero[3] = {0.0, 0.0, 0.0};
  const double grav[3] = {0.0, 0.0, lim.gravity};
  const bool want_xy = has(lim.omega_xy_max);
  int verdict = kFeasible;

  double f0 = 0.0, fT = 0.0;
  int nf = 0;
  if (has(lim.f_min) || has(lim.f_max) || want_xy) {
    int base = 0;
    nf = magnitude3_roots<NC, 2, Roots>(p, grav, T, roots, base);
    f0 = magnitude3_at<NC, 2>(p, grav, 0.0);
    fT = magnitude3_at<NC, 2>(p, grav, T);
    double lo = fmin(f0, fT), hi = fmax(f0, fT);
    for (int i = 0; i < nf; ++i) {
      const double t = roots[base + i] * T;
      const double v = magnitude3_at<NC, 2>(p, grav, t);
      cand[2 * i] = t;
      cand[2 * i + 1] = v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    bounds[0] = lo;
    bounds[1] = hi;
    if (has(lim.f_min) && lo < lim.f_min) verdict = kThrustLow;   // low is tested before high (:155-172)
    else if (has(lim.f_max) && hi > lim.f_max) verdict = kThrustHigh;
  }

  if (has(lim.v_max)) {
    int base = 0;
    const int nv = magnitude3_roots<NC, 1, Roots>(p, zero, T, roots, base);
    double hi = fmax(magnitude3_at<NC, 1>(p, zero, 0.0), magnitude3_at<NC, 1>(p, zero, T));
    for (int i = 0; i < nv; ++i) hi = fmax(hi, magnitude3_at<NC, 1>(p, zero, roots[base + i] * T));
    bounds[2] = hi;
    if (verdict == kFeasible && hi > lim.v_max) verdict = kVelocity;
  }

  if (D == 4 && (has(lim.omega_z_max) || has(lim.omega_z_dot_max))) {
    double y[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) y[i] = i < N ? c[3 * N + i] : 0.0;
    if (has(lim.omega_z_max)) {
      bounds[4] = axis_abs_max<NC, 1, Roots>(y, T, roots);
      if (verdict == kFeasible && bounds[4] > lim.omega_z_max) verdict = kYawRates;
    }
    if (has(lim.omega_z_dot_max)) {
      bounds[5] = axis_abs_max<NC, 2, Roots>(y, T, roots);
      if (verdict == kFeasible && bounds[5] > lim.omega_z_dot_max) verdict = kYawAcc;
    }
  }

  if (want_xy) {
    int base = 0;
    const int nj = magnitude3_roots<NC, 3, Roots>(p, zero, T, roots, base);
    const double j0 = magnitude3_at<NC, 3>(p, zero, 0.0), jT = magnitude3_at<NC, 3>(p, zero, T);
    for (int i = 0; i < nj; ++i) {
      const double t = roots[base + i] * T;
      cand_jerk[2 * i] = t;
      cand_jerk[2 * i + 1] = magnitude3_at<NC, 3>(p, zero, t);
    }
    double top;
    const int r = roll_pitch_sections(T, f0, fT, j0, jT, cand, nf, cand_jerk, nj, lim.omega_xy_max, lim.min_section_time_s, top);
    bounds[3] = top;
    if (verdict == kFeasible) verdict = r;
  }
  return verdict;
}

// element counts of the two per-segment work areas (doubles)
constexpr int roots_len(int nc) { return 2 * (2 * nc - 5); }
constexpr int cand_thrust_len(int nc) { return 2 * (2 * nc - 7); }
constexpr int cand_jerk_len(int nc) { return 2 * (2 * nc - 9); }

}  // namespace mtgf
