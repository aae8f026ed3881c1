// mtg_halfplane_lane.h -- per-lane algorithm of the batched half-plane / flight-corridor feasibility check.
//
// What it replaces, per segment: FeasibilityBase::checkHalfPlaneFeasibility(const Segment&)
// (mav_trajectory_generation_ros/src/feasibility_base.cpp:119-154) over a list of HalfPlane (:54-86).  A plane is four doubles
// (nx, ny, nz, offset): unit normal, offset = point . normal.  The signed clearance of the segment at local time t is
//   n . p(t) - offset        over dimensions 0-2 (a 4th, yaw, dimension is ignored: the reference's .head(3)),
// and a plane fails the segment iff a candidate time has clearance <= 0.  Candidates (Polynomial::computeMinMaxCandidates,
// polynomial.cpp:65-83): 0, T and the real roots in [0, T] of the derivative of the PROJECTED polynomial q = sum_dim n_dim p_dim
// (degree N - 2), found in tau = t / T by real_roots_unit of mtg_extrema_lane.h, unchanged.  The clearance itself is
// evaluated on q as well (one Horner chain, not three): it differs from the reference's (p(t) - point) . n by rounding only.
//
// Choices and quirks a caller may meet:
//   * the comparison is the reference's `clearance <= 0.0`: a NaN clearance does NOT fail the plane, and it does not enter the
//     reported minimum either (strict <); a segment all of whose clearances are NaN reports +infinity;
//   * 0 and T are candidates exactly (t = 0 and t = T, not a root times T); T <= 0 has no interior candidates, both ends are
//     still evaluated (the reference, given T < 0, evaluates nothing at all and passes: a negative time is not a segment);
//   * NO early exit: the segment's clearance is the minimum over ALL planes and ALL candidates, where the reference returns at
//     the first failure; the failing plane reported is still the first in list order, as the reference's loop finds it;
//   * a plane whose normal equals the previous plane's, or its negation, component by component (compared by VALUE, so that
//     +0 and -0 agree: HalfPlane::createBoundingBox emits (+1, 0, 0) then (-1, 0, 0), not (-1, -0, -0)) has the same critical
//     points: the root list still in the root buffer is reused and only the evaluation runs -- a box costs three searches,
//     not six.  The roots of q' and of -q' as real_roots_unit finds them can differ only where a derivative level is
//     EXACTLY zero at a partition point.  The condition is a function of the plane data alone: lanes that share a plane
//     set take the same path;
//   * dimension other than 3 or 4: every segment infeasible (the reference returns false before it looks at a plane): plane
//     index kNoPlane, clearance NaN;
//   * N = 1 .. 12 run in the next even instantiation (at least 4) on zero-padded coefficients: identically-zero leading levels
//     of the derivative chain fall through real_roots_unit, N <= 2 has no interior candidates.
// Same code runs on the device (mtg_halfplane.hip) and on the host (mtg_halfplane_host.cpp).
#pragma once

#include "mtg_segment_lane.h"

namespace mtgh {

constexpr int kMinInstance = 4;       // smallest instantiation: q' has 3 coefficients (real_roots_unit needs at least 2)
constexpr int kMaxPlanes = 64;
constexpr int kMaxSegments = 1 << 22; // segment << 8 | plane stays a positive int
constexpr int kNoPlane = 0xff;        // "infeasible before any plane was looked at" (dimension not 3 or 4)

// what both entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         int n_planes, long long ps_b, long long ps_k) {
  return mtgs::shape_ok(n_coeffs, 1, n_segments, dimension, 32, batch, ts_b, ts_k) && n_segments < kMaxSegments &&
         n_planes >= 1 && n_planes <= kMaxPlanes && ps_b >= 0 && ps_k >= 0;
}

constexpr int roots_len(int nc) { return 2 * (nc - 2); }   // the two buffers of real_roots_unit<nc - 1>

// One segment against one plane set.  c = [D][N] coefficients (increasing powers), N <= NC; planes = P x (nx, ny, nz, offset);
// roots: roots_len(NC) elements.  Returns the first failing plane in list order (-1: none, kNoPlane: dimension);
// clearance = minimum over all planes and candidates.
template <int NC, class Roots>
MTGX_HD int segment_check(const double* c, int N, int D, double T, const double* planes, int P, Roots& roots, double& clearance) {
  if (!(D == 3 || D == 4)) {
    clearance = NAN;
    return kNoPlane;
  }
  double p[3][NC];
  mtgs::load_padded(c, N, D, p);
  double tpow[NC - 1];   // T^j
  tpow[0] = 1.0;
#pragma unroll
  for (int j = 1; j < NC - 1; ++j) tpow[j] = tpow[j - 1] * T;

  double best = INFINITY;
  int failing = -1, cnt = 0, base = 0;
  double pnx = NAN, pny = NAN, pnz = NAN;   // (NaN: equal to nothing, the first plane always searches)
  for (int h = 0; h < P; ++h) {
    const double nx = planes[4 * h], ny = planes[4 * h + 1], nz = planes[4 * h + 2], off = planes[4 * h + 3];
    double q[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) q[i] = fma(nz, p[2][i], fma(ny, p[1][i], nx * p[0][i]));
    const bool same = (nx == pnx && ny == pny && nz == pnz) || (nx == -pnx && ny == -pny && nz == -pnz);
    if (!same) {
      cnt = 0;
      if (T > 0.0) {
        double g[NC - 1];   // dq/dt in tau = t / T
#pragma unroll
        for (int j = 0; j < NC - 1; ++j) g[j] = (double)(j + 1) * q[j + 1] * tpow[j];
        cnt = mtgx::real_roots_unit<NC - 1, Roots>(g, roots, base);
      }
      pnx = nx; pny = ny; pnz = nz;
    }
    const double at_start = q[0] - off;                              // t = 0
    const double at_end = mtgx::horner<NC - 1>(q, T) - off;          // t = T
    bool fails = at_start <= 0.0 || at_end <= 0.0;
    double lo = INFINITY;
    if (at_start < lo) lo = at_start;
    if (at_end < lo) lo = at_end;
    for (int i = 0; i < cnt; ++i) {
      const double v = mtgx::horner<NC - 1>(q, roots[base + i] * T) - off;
      fails = fails || v <= 0.0;
      if (v < lo) lo = v;
    }
    if (lo < best) best = lo;
    if (fails && failing < 0) failing = h;
  }
  clearance = best;
  return failing;
}

}  // namespace mtgh
