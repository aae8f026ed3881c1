// mtg_recursive_lane.h -- per-lane algorithm of the batched recursive input-feasibility check.
//
// What it replaces, per segment: FeasibilityRecursive::checkInputFeasibility(const Segment&)
// (mav_trajectory_generation_ros/src/feasibility_recursive.cpp:42-297), Mueller's recursive test: per section [t1, t2] the
// thrust, velocity and jerk of every axis are bounded by their single-axis extrema, the bounds decide "feasible", "infeasible"
// or "split the section in two".  It needs only single-axis roots: the real roots in [0, T] of the acceleration, jerk and snap
// polynomials of x, y, z (degree N - 3, N - 4, N - 5), found ONCE per segment through real_roots_unit of mtg_extrema_lane.h --
// one search per axis, whose upper derivative levels ARE the jerk and snap polynomials -- and kept as times; a section selects
// the ones inside it (Polynomial::selectMinMaxFromRoots, polynomial.cpp:32-63, 85-100: inclusive t1 <= r <= t2) and evaluates
// the polynomial there.  Root VALUES are not cached: a section evaluates few roots
// (most lie outside a short section), and the times alone are 9 N - 36 doubles per lane.  With v_max the search starts at the
// acceleration polynomial, without it at the jerk polynomial, without any of the four limits nothing is searched (:50-81).
//
// The recursion (:133-297) returns the first result that is not feasible, first half before second half.  The walk below is
// that depth-first order without a stack, as roll_pitch_sections of mtg_feasibility_lane.h: a section is (depth, path bits)
// and its ends are recomputed from [0, T] by the reference's own (t1 + t2) / 2.  A section is always bounded in full -- the
// reference returns from inside the section at the first failing test; here the tests are made in its order on the complete
// bounds, which gives the same result and lets the whole-segment bounds be reported whatever the verdict.
// Same code runs on the device (mtg_recursive.hip) and on the host (mtg_recursive_host.cpp).
#pragma once

#include "mtg_feasibility_lane.h"

namespace mtgr {

using mtgf::has;
using mtgf::Limits;
using mtgf::kNumBounds;   // f_lower_bound, f_upper_bound, v_upper_bound, roll/pitch bound of [0, T]; |yaw rate| max, |yaw acc| max

constexpr int kSplit = -1;       // a section whose bounds exceed a limit without proving a violation: look at its halves
constexpr int kMaxDepth = 62;    // our guard (min_section_time_s == 0: the reference recurses without end)

// The lane's two work areas (doubles): the root search's two alternating buffers (the acceleration polynomial's are the
// largest; the yaw searches use them afterwards), and the nine root lists, list (DER, axis) at list_offset.
constexpr int scratch_len(int nc) { return 2 * (nc - 3); }
constexpr int list_len(int nc, int der) { return nc - der - 1; }   // roots of p^(der): its degree
constexpr int list_offset(int nc, int der, int axis) {
  return (der == 2 ? 0 : der == 3 ? 3 * list_len(nc, 2) : 3 * list_len(nc, 2) + 3 * list_len(nc, 3)) + axis * list_len(nc, der);
}
constexpr int store_len(int nc) { return list_offset(nc, 4, 3); }

// p^(DER)(t) (Polynomial::evaluate: Horner over base(DER, i) c_i from the highest power down)
template <int NC, int DER>
MTGX_HD double axis_at(const double (&p)[NC], double t) {
  double r = 0.0;
#pragma unroll
  for (int k = NC - 1; k >= DER; --k) r = fma(r, t, mtgf::ff(k, DER) * p[k]);
  return r;
}

// The root lists of one axis from ONE search.  The derivative chain that isolates the roots of p^(DER) passes, on its way up,
// through the polynomials p^(DER+1), p^(DER+2), ..: level K of the chain of degree M = NC - DER - 1 holds the roots of
// p^(DER + M - K).  So the search of the acceleration polynomial delivers the jerk and snap roots as well, if those levels are
// refined like the last one (TIGHT) -- 3 searches per segment instead of 9.
template <int NC, int DER, class Buf>
struct RootSink {
  Buf& store;
  double T;
  int axis;
  int n[3];   // counts of the lists of p^(2), p^(3), p^(4)
  template <int K>
  MTGX_HD void level(Buf& roots, int src, int cnt) {
    constexpr int der = DER + (NC - DER - 1) - K;
    if constexpr (der <= 4) {
      for (int i = 0; i < cnt; ++i) store[list_offset(NC, der, axis) + i] = roots[src + i] * T;   // as times
      n[der - 2] = cnt;
    }
  }
};

// real roots in [0, T] of p^(DER), .., p^(4) (Polynomial::getRoots, the ones a section can select), ascending, as times
template <int NC, int DER, class Buf>
MTGX_HD void axis_roots(const double (&p)[NC], double T, Buf& scratch, Buf& store, int axis, int (&cnt)[9]) {
  constexpr int L = NC - DER;
  double g[L];
  double tp = 1.0;
#pragma unroll
  for (int j = 0; j < L; ++j) {
    g[j] = p[j + DER] * mtgf::ff(j + DER, DER) * tp;
    tp *= T;
  }
  RootSink<NC, DER, Buf> sink{store, T, axis, {0, 0, 0}};
  int base = 0;
  mtgx::real_roots_unit<L, Buf, false, 5 - DER, RootSink<NC, DER, Buf>>(g, scratch, base, mtgx::Share{0, 1, 1}, &sink);
#pragma unroll
  for (int q = DER - 2; q < 3; ++q) cnt[3 * q + axis] = sink.n[q];
}

// Polynomial::selectMinMaxFromRoots(t1, t2, DER, roots of p^(DER+1)): candidates t1, t2 and the roots inside [t1, t2].  The two
// end values e1, e2 come from the caller, which needs them for the norms at the section's ends as well.
template <int NC, int DER, class Buf>
MTGX_HD void axis_min_max(const double (&p)[NC], double t1, double t2, double e1, double e2, Buf& store, int off, int cnt, double& lo,
                          double& hi) {
  lo = DBL_MAX;
  hi = -DBL_MAX;
  if (e1 < lo) lo = e1;
  if (e1 > hi) hi = e1;
  if (e2 < lo) lo = e2;
  if (e2 > hi) hi = e2;
  for (int i = 0; i < cnt; ++i) {
    const double t = store[off + i];
    if (t < t1 || t > t2) continue;
    const double v = axis_at<NC, DER>(p, t);
    if (v < lo) lo = v;
    if (v > hi) hi = v;
  }
}

MTGX_HD double norm3(double x, double y, double z) { return sqrt(fma(z, z, fma(y, y, x * x))); }

struct Section {
  double f_lower, f_upper, v_upper, omega_xy;   // zero where the quantity is not needed, as in the reference
};

// recursiveFeasibility's body for [t1, t2] (:139-297) without the minimum-section-time test and the recursion: a result
// code, or kSplit.  cnt[3 * (DER - 2) + axis]: root count of list (DER, axis).
template <int NC, class Buf>
MTGX_HD int section_check(const double (&p)[3][NC], double t1, double t2, const Limits& lim, Buf& store, const int (&cnt)[9],
                          Section& s) {
  const bool has_f_min = has(lim.f_min), has_f_max = has(lim.f_max), has_v = has(lim.v_max), has_xy = has(lim.omega_xy_max);
  const double grav[3] = {0.0, 0.0, lim.gravity};
  const bool want_f = has_f_min || has_f_max || has_xy;
  // velocity, acceleration and jerk of every axis at both ends, once: 18 independent Horner chains; the norms at the ends and
  // the per-axis extrema below both start from them
  double v1[3], v2[3], a1[3], a2[3], j1[3], j2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    v1[d] = has_v ? axis_at<NC, 1>(p[d], t1) : 0.0;
    v2[d] = has_v ? axis_at<NC, 1>(p[d], t2) : 0.0;
    a1[d] = want_f ? axis_at<NC, 2>(p[d], t1) : 0.0;
    a2[d] = want_f ? axis_at<NC, 2>(p[d], t2) : 0.0;
    j1[d] = has_xy ? axis_at<NC, 3>(p[d], t1) : 0.0;
    j2[d] = has_xy ? axis_at<NC, 3>(p[d], t2) : 0.0;
  }
  int verdict = mtgf::kFeasible;
  if (has_f_min || has_f_max) {   // thrust at the section's ends, low before high (:140-155)
    const double f1 = norm3(a1[0], a1[1], a1[2] + lim.gravity), f2 = norm3(a2[0], a2[1], a2[2] + lim.gravity);
    if (has_f_min && (f2 < f1 ? f2 : f1) < lim.f_min) verdict = mtgf::kThrustLow;
    else if (has_f_max && (f1 < f2 ? f2 : f1) > lim.f_max) verdict = mtgf::kThrustHigh;
  }
  double v_sqr = 0.0, f_min_sqr = 0.0, f_max_sqr = 0.0, j_sqr = 0.0;
  if (has_v) {
    const double n1 = norm3(v1[0], v1[1], v1[2]), n2 = norm3(v2[0], v2[1], v2[2]);
    if (verdict == mtgf::kFeasible && (n1 < n2 ? n2 : n1) > lim.v_max) verdict = mtgf::kVelocity;   // (:157-168)
#pragma unroll
    for (int d = 0; d < 3; ++d) {   // (:176-193)
      double lo, hi;
      axis_min_max<NC, 1, Buf>(p[d], t1, t2, v1[d], v2[d], store, list_offset(NC, 2, d), cnt[d], lo, hi);
      if (verdict == mtgf::kFeasible && fmax(lo * lo, hi * hi) > lim.v_max * lim.v_max) verdict = mtgf::kVelocity;
      const double m = fmax(fabs(lo), fabs(hi));
      v_sqr = fma(m, m, v_sqr);
    }
  }
  if (want_f) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {   // (:195-228)
      double lo, hi;
      axis_min_max<NC, 2, Buf>(p[d], t1, t2, a1[d], a2[d], store, list_offset(NC, 3, d), cnt[3 + d], lo, hi);
      const double f_i_min = lo + grav[d], f_i_max = hi + grav[d];
      const double m = fmax(fabs(f_i_min), fabs(f_i_max));
      if (verdict == mtgf::kFeasible && has_f_max && m > lim.f_max) verdict = mtgf::kThrustHigh;
      if (!(f_i_min * f_i_max < 0.0)) {   // (a sign change: the minimum squared value is zero)
        const double n = fmin(fabs(f_i_min), fabs(f_i_max));
        f_min_sqr = fma(n, n, f_min_sqr);
      }
      f_max_sqr = fma(m, m, f_max_sqr);
    }
  }
  if (has_xy) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {   // (:230-242)
      double lo, hi;
      axis_min_max<NC, 3, Buf>(p[d], t1, t2, j1[d], j2[d], store, list_offset(NC, 4, d), cnt[6 + d], lo, hi);
      const double m = fmax(fabs(lo), fabs(hi));
      j_sqr = fma(m, m, j_sqr);
    }
  }
  s.f_lower = sqrt(f_min_sqr);
  s.f_upper = sqrt(f_max_sqr);
  s.v_upper = sqrt(v_sqr);
  s.omega_xy = f_min_sqr > 1.0e-6 ? sqrt(j_sqr / f_min_sqr) : DBL_MAX;   // (divide-by-zero protection, :248-253)
  if (verdict != mtgf::kFeasible) return verdict;
  if (has_f_min && s.f_upper < lim.f_min) return mtgf::kThrustLow;    // definitely infeasible (:255-268)
  if (has_f_max && s.f_lower > lim.f_max) return mtgf::kThrustHigh;
  if ((has_f_min && s.f_lower < lim.f_min) || (has_f_max && s.f_upper > lim.f_max) || (has_v && s.v_upper > lim.v_max) ||
      (has_xy && s.omega_xy > lim.omega_xy_max))
    return kSplit;   // (:270-294)
  return mtgf::kFeasible;
}

// One segment.  c = [D][N] coefficients (increasing powers), N <= NC (zero-padded tail), T = segment time.  scratch:
// scratch_len(NC) elements, store: store_len(NC).  bounds[kNumBounds]: NaN where not computed; the first four belong to the
// section [0, T] and are computed even where T is shorter than a section.  sections: the sections examined, i.e. the calls of
// recursiveFeasibility that got past the minimum-section-time test.
template <int NC, class Buf>
MTGX_HD int segment_check(const double* c, int N, int D, double T, const Limits& lim, Buf& scratch, Buf& store,
                          double (&bounds)[kNumBounds], int& sections) {
#pragma unroll
  for (int q = 0; q < kNumBounds; ++q) bounds[q] = NAN;
  sections = 0;
  if (!(D == 3 || D == 4)) return mtgf::kIndeterminable;
  int verdict = mtgf::kFeasible;
  {
    double p[3][NC];
    mtgs::load_padded(c, N, D, p);
    const bool want_f = has(lim.f_min) || has(lim.f_max) || has(lim.omega_xy_max);
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (has(lim.v_max)) {   // (the lists a limit set does not need are filled along the way and never read)
#pragma unroll
      for (int d = 0; d < 3; ++d) axis_roots<NC, 2, Buf>(p[d], T, scratch, store, d, cnt);
    } else if (want_f) {
#pragma unroll
      for (int d = 0; d < 3; ++d) axis_roots<NC, 3, Buf>(p[d], T, scratch, store, d, cnt);
    }
    unsigned long long path = 0;   // bit l (from the top): 0 = first half, 1 = second half
    int depth = 0;
    for (;;) {
      double t1 = 0.0, t2 = T;
      for (int l = depth - 1; l >= 0; --l) {
        const double t_half = (t1 + t2) / 2;
        if ((path >> l) & 1ull) t1 = t_half; else t2 = t_half;
      }
      const bool too_short = t2 - t1 < lim.min_section_time_s;   // (:136-138: before anything else is looked at)
      if (too_short && depth > 0) { verdict = mtgf::kIndeterminable; break; }
      Section s;
      const int r = section_check<NC, Buf>(p, t1, t2, lim, store, cnt, s);
      if (depth == 0) {
        if (want_f) { bounds[0] = s.f_lower; bounds[1] = s.f_upper; }
        if (has(lim.v_max)) bounds[2] = s.v_upper;
        if (has(lim.omega_xy_max)) bounds[3] = s.omega_xy;
      }
      if (too_short) { verdict = mtgf::kIndeterminable; break; }
      ++sections;
      if (r == kSplit) {
        if (depth >= kMaxDepth) { verdict = mtgf::kIndeterminable; break; }
        path <<= 1;
        ++depth;
        continue;
      }
      if (r != mtgf::kFeasible) { verdict = r; break; }
      while (depth > 0 && (path & 1ull)) { path >>= 1; --depth; }   // this section is feasible: on to the next one
      if (depth == 0) break;
      path |= 1ull;
    }
  }
  // yaw over the whole segment, only after the recursion returned feasible (:93-127); the maxima are reported regardless
  if (D == 4 && (has(lim.omega_z_max) || has(lim.omega_z_dot_max))) {
    double y[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) y[i] = i < N ? c[3 * N + i] : 0.0;
    if (has(lim.omega_z_max)) {
      bounds[4] = mtgf::axis_abs_max<NC, 1, Buf>(y, T, scratch);
      if (verdict == mtgf::kFeasible && bounds[4] > lim.omega_z_max) verdict = mtgf::kYawRates;
    }
    if (has(lim.omega_z_dot_max)) {
      bounds[5] = mtgf::axis_abs_max<NC, 2, Buf>(y, T, scratch);
      if (verdict == mtgf::kFeasible && bounds[5] > lim.omega_z_dot_max) verdict = mtgf::kYawAcc;
    }
  }
  return verdict;
}

}  // namespace mtgr
