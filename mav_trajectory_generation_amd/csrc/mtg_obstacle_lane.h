// mtg_obstacle_lane.h -- per-lane algorithm of the batched sphere-obstacle clearance check.
//
// What it replaces, per segment and obstacle: Trajectory::offsetTrajectory(-c) followed by
// Segment::computeMinMaxMagnitudeCandidates(POSITION, 0, T, {0, 1, 2}) / selectMinMaxMagnitudeFromCandidates
// (src/segment.cpp:83-184) and `minimum - r - inflation`.  An obstacle is four doubles (cx, cy, cz, r); the clearance of the
// segment at local time t is
//   || p(t) - c || - r - inflation        over dimensions 0-2 (a 4th, yaw, dimension is never read),
// and an obstacle fails the segment iff a candidate time has !(clearance > 0).  Candidates: t = 0 and t = T exactly, and the
// real roots in [0, T] of g = sum_dim (p_dim - c_dim) p_dim', found in tau = t / T by real_roots_unit of mtg_extrema_lane.h,
// unchanged.
//
// Once per segment (Segment): the convolution g0 = sum_dim p p' in tau (magnitude_derivative, the expensive part:
// 3 NC (NC - 1) FMAs) and the segment's bounding boxes.  Per obstacle only the lowest N - 1 of
// g's 2 N - 2 coefficients change:  g[j] = g0[j] - sum_dim c_dim (j + 1) p_dim[j + 1] T^(j + 1).
//
// Pruning.  The bounding volume is FOUR boxes, one per quarter of tau in [0, 1]: each the hull of the BERNSTEIN coefficients of
// u_dim(tau) = p_dim(tau T) on that quarter (a polynomial lies in the convex hull of its control points; the basis change is
// NC^2 / 2 FMAs per axis, the quarters' control points come from three de Casteljau splits at 1/2; no root search).  One box
// around a whole segment is a poor volume for a long segment -- it reaches most obstacles of a scene -- and the busiest lane
// sets its wave's pace.  lower_bound() is the smallest box distance over the quarters, turned into a bound on every clearance
// the evaluation below can COMPUTE for that obstacle: per axis the box distance is reduced by kBoxUlps ulps of E_dim + |c_dim|,
// E_dim = sum_i |p_dim[i] T^i|, which covers the rounding of the basis change ((NC + 2) ulps of E: weights in [0, 1]), of the
// two nested splits (an average of two control points per level, 2 (NC - 1) ulps of E) and of the Horner chain of the
// evaluation (2 NC ulps of E + |c|) -- 60 at NC = 12 -- with room to spare, and the norm and the two subtractions are reduced by
// kNormUlps ulps of their operands.  An obstacle is skipped only when its bound is > 0 (it cannot
// fail) and strictly greater than the running minimum (it can neither lower the minimum nor tie it, so that neither the value
// nor the index changes).  A NaN bound compares false and skips nothing.
//
// Order.  A lane walks ITS OWN obstacles in ascending (bound, index) order -- the nearest first makes the running minimum
// small early -- and stops at the first one that may be skipped: every later one has a bound at least as large.  The next
// obstacle is SELECTED by a scan of the whole list (about 120 operations per obstacle, against the thousands of a root search),
// not from a stored order: nothing is kept per obstacle, so the list may be long, every lane of a wave reads the same
// obstacle in the same iteration of the scan (scalar loads where the set is shared) and keeps the selected one in registers.
// A wave runs as many searches as its busiest lane.  Since lanes leave list order, the three rules hold for ANY order:
//   * the failing obstacle reported is the smallest index among the failing ones;
//   * the nearest obstacle is the smallest index among those that attain the minimum; a NaN clearance wins the minimum, and
//     the smallest index among the obstacles that produced one is reported;
//   * within one obstacle the candidates are taken in the order 0, T, roots ascending, strict <, first NaN wins.
// N = 1 .. 12 run in the next even instantiation (at least 4) on zero-padded coefficients; T <= 0 has no interior candidates,
// both ends are still evaluated.
// Same code runs on the device (mtg_obstacle.hip) and on the host (mtg_obstacle_host.cpp).
#pragma once

#include "mtg_segment_lane.h"

namespace mtgo {

constexpr int kMinInstance = 4;
constexpr int kMaxObstacles = 4096;
constexpr int kObstacleBits = 12;
constexpr int kMaxSegments = 1 << 19;   // segment << 12 | obstacle stays a positive int
constexpr int kBoxes = 4;               // boxes per segment: the quarters [0, 1/4], .., [3/4, 1] of tau
constexpr double kBoxUlps = 96.0;       // allowance per axis, in ulps of E_dim + |c_dim| (see above)
constexpr double kNormUlps = 8.0;

// the check's own first-failure word: the smallest word over the failing (segment, obstacle) pairs is the first segment in
// SEGMENT order and, within it, the smallest failing obstacle index
MTGX_HD int failure_word(int segment, int obstacle) { return (segment << kObstacleBits) | obstacle; }
MTGX_HD int failure_segment(int word) { return word >> kObstacleBits; }
MTGX_HD int failure_obstacle(int word) { return word & (kMaxObstacles - 1); }

// what both entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         int n_obstacles, long long os_b, double inflation) {
  return mtgs::shape_ok(n_coeffs, 1, n_segments, dimension, 4, batch, ts_b, ts_k) && dimension >= 3 && n_segments < kMaxSegments &&
         n_obstacles >= 1 && n_obstacles <= kMaxObstacles && os_b >= 0 && inflation >= 0.0 && inflation <= DBL_MAX;
}

constexpr int roots_len(int nc) { return 2 * (2 * nc - 3); }   // the two buffers of real_roots_unit<2 nc - 2>
constexpr int buffer_len(int nc) { return roots_len(nc) + 2 * nc - 2; }   // the lane's buffer: the root buffers, then g0

constexpr double binomial(int n, int k) {
  double r = 1.0;
  for (int i = 1; i <= k; ++i) r = r * (double)(n - k + i) / (double)i;
  return r;
}

// The same address, opaque to the device compiler: a load through it is a load.  Without it the compiler recognises the
// segment's coefficients as loaded already and keeps all 3 NC of them in registers from the first read to the last use.
MTGX_HD const double* read_again(const double* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}

// what a lane KEEPS of its segment across the obstacles.  The coefficients themselves are not kept: a search of degree 2 NC - 3
// holds 2 (2 NC - 2) doubles of its own, and 3 NC + 2 NC - 2 more would not fit the register file at NC = 12 without scratch; they are
// read again (36 doubles, from the cache) where g is formed and where the candidates are evaluated.
template <int NC>
struct Segment {
  const double* c;          // [D][N] coefficients, increasing powers
  int N, D;
  double T;
  // (g0 = sum_dim u u' in tau, u_dim[i] = p_dim[i] T^i, is kept behind the root buffers, not here: on the device that is LDS)
  double lo[kBoxes][3], hi[kBoxes][3], e[3];   // bounding boxes of the quarters, and E_dim
};

// de Casteljau at 1/2: the control polygons of the two halves of the polynomial with control points c
template <int NC>
MTGX_HD void split_half(const double (&c)[NC], double (&left)[NC], double (&right)[NC]) {
  double pts[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) pts[i] = c[i];
  left[0] = pts[0];
  right[NC - 1] = pts[NC - 1];
#pragma unroll
  for (int r = 1; r < NC; ++r) {
#pragma unroll
    for (int i = 0; i + r < NC; ++i) pts[i] = 0.5 * (pts[i] + pts[i + 1]);
    left[r] = pts[0];
    right[NC - 1 - r] = pts[NC - 1 - r];
  }
}
template <int NC>
MTGX_HD void hull(const double (&c)[NC], bool nan, double& lo, double& hi) {
  double l = c[0], h = c[0];
#pragma unroll
  for (int i = 1; i < NC; ++i) {
    l = c[i] < l ? c[i] : l;
    h = c[i] > h ? c[i] : h;
  }
  lo = nan ? NAN : l;
  hi = nan ? NAN : h;
}

// the segment's four quarter boxes and E_dim from its padded coefficients p and tpow[i] = T^i (also the keep-out zone check's,
// mtg_keepout_lane.h); c, N, D, T are recorded as they are
template <int NC>
MTGX_HD void segment_boxes(const double* c, int N, int D, double T, const double (&p)[3][NC], const double (&tpow)[NC], Segment<NC>& S) {
  S.c = c;
  S.N = N;
  S.D = D;
  S.T = T;
  constexpr int n = NC - 1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double b[NC], e = fabs(p[d][0]);
    b[0] = p[d][0];   // control point 0 is u[0]
    bool nan = b[0] != b[0];
#pragma unroll
    for (int i = 1; i < NC; ++i) e += fabs(p[d][i] * tpow[i]);
#pragma unroll
    for (int k = 1; k <= n; ++k) {
      double v = p[d][0];   // control point k = sum_{i <= k} C(k, i) / C(n, i) u[i]
#pragma unroll
      for (int i = 1; i <= k; ++i) v = fma(binomial(k, i) / binomial(n, i), p[d][i] * tpow[i], v);
      nan = nan || v != v;
      b[k] = v;
    }
    double left[NC], right[NC], q0[NC], q1[NC];
    split_half<NC>(b, left, right);
    split_half<NC>(left, q0, q1);
    hull<NC>(q0, nan, S.lo[0][d], S.hi[0][d]);
    hull<NC>(q1, nan, S.lo[1][d], S.hi[1][d]);
    split_half<NC>(right, q0, q1);
    hull<NC>(q0, nan, S.lo[2][d], S.hi[2][d]);
    hull<NC>(q1, nan, S.lo[3][d], S.hi[3][d]);
    S.e[d] = e;
  }
}

template <int NC, class Roots>
MTGX_HD void segment_prepare(const double* c, int N, int D, double T, Segment<NC>& S, Roots& roots) {
  double p[3][NC], tpow[NC];
  mtgs::load_padded(c, N, D, p);
  tpow[0] = 1.0;
#pragma unroll
  for (int i = 1; i < NC; ++i) tpow[i] = tpow[i - 1] * T;
  {
    double g0[2 * NC - 2];
    mtgs::magnitude_derivative<NC, 3, 0, false>(p, nullptr, T, g0);
#pragma unroll
    for (int j = 0; j < 2 * NC - 2; ++j) roots[roots_len(NC) + j] = g0[j];
  }
  segment_boxes<NC>(c, N, D, T, p, tpow, S);
}

// a lower bound on every clearance the evaluation computes for this obstacle over the segment (header comment); NaN if
// anything that enters it is
template <int NC>
MTGX_HD double lower_bound(const Segment<NC>& S, double cx, double cy, double cz, double r, double inflation) {
  const double c[3] = {cx, cy, cz};
  double margin[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) margin[d] = kBoxUlps * DBL_EPSILON * (S.e[d] + fabs(c[d]));
  double acc = INFINITY;   // the smallest squared box distance over the quarters
  bool nan = false;
#pragma unroll
  for (int q = 0; q < kBoxes; ++q) {
    double a = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double below = S.lo[q][d] - c[d], above = c[d] - S.hi[q][d];   // (NaN box or centre: NaN)
      double gap = (below > above ? below : above) - margin[d];
      gap = gap < 0.0 ? 0.0 : gap;
      nan = nan || below != below || above != above || margin[d] != margin[d];
      a = fma(gap, gap, a);
    }
    acc = a < acc ? a : acc;
  }
  if (nan) acc = NAN;
  const double dist = sqrt(acc);
  return dist - r - inflation - kNormUlps * DBL_EPSILON * (dist + fabs(r) + inflation);
}

// running result of a segment over its obstacles, in any order
struct Fold {
  double clearance, time;   // minimum so far (NaN wins), and its candidate's local time
  int nearest;              // obstacle that attains it
  int failing;              // smallest failing obstacle index, kMaxObstacles: none
};
MTGX_HD void fold_init(Fold& f) {
  f.clearance = INFINITY;
  f.time = 0.0;
  f.nearest = kMaxObstacles;
  f.failing = kMaxObstacles;
}
// one obstacle's minimum (v at local time t, `fails`: a candidate had !(clearance > 0)) into the running result
MTGX_HD void fold_obstacle(Fold& f, int h, double v, double t, bool fails) {
  const bool v_nan = v != v, f_nan = f.clearance != f.clearance;
  const bool takes = v_nan ? (!f_nan || h < f.nearest) : (!f_nan && (v < f.clearance || (v == f.clearance && h < f.nearest)));
  if (takes) { f.clearance = v; f.time = t; f.nearest = h; }
  if (fails && h < f.failing) f.failing = h;
}

// One segment against one obstacle: the search and the evaluation.  Never pruned.
template <int NC, class Roots>
MTGX_HD void obstacle_clearance(const Segment<NC>& S, double cx, double cy, double cz, double r, double inflation, Roots& roots,
                                double& v_min, double& t_min, bool& fails) {
  constexpr int L = 2 * NC - 2;
  const double off[3] = {-cx, -cy, -cz};   // (joins the constant coefficient: the reference's offset segment)
  int cnt = 0, base = 0;
  if (S.T > 0.0) {
    const double* c = read_again(S.c);
    double g[L];
    double tp = 1.0;   // T^(j + 1)
#pragma unroll
    for (int j = 0; j < L; ++j) {
      g[j] = roots[roots_len(NC) + j];
      if (j < NC - 1) {
        tp *= S.T;
        const double w = (double)(j + 1) * tp;
        const bool in = j + 1 < S.N;
        const double p0 = in ? c[j + 1] : 0.0, p1 = in ? c[S.N + j + 1] : 0.0, p2 = in ? c[2 * S.N + j + 1] : 0.0;
        g[j] = fma(off[2], p2 * w, fma(off[1], p1 * w, fma(off[0], p0 * w, g[j])));
      }
    }
    cnt = mtgx::real_roots_unit<L, Roots>(g, roots, base);
  }
  double p[3][NC];
  mtgs::load_padded(read_again(S.c), S.N, S.D, p);
  double best = INFINITY, best_t = 0.0;
  bool nan = false, bad = false;
  for (int i = -2; i < cnt; ++i) {
    // (a Newton step towards a root AT 0 or 1 can leave [0, 1] by a rounding error: the end itself is a candidate already)
    const double t = i == -2 ? 0.0 : (i == -1 ? S.T : fmin(fmax(roots[base + i], 0.0), 1.0) * S.T);
    const double v = mtgs::magnitude_at<NC, 3, 0, true>(p, off, t) - r - inflation;
    bad = bad || !(v > 0.0);
    if (!nan && (v != v || v < best)) { best = v; best_t = t; nan = v != v; }
  }
  v_min = best;
  t_min = best_t;
  fails = bad;
}

// One segment against its obstacle set (M x (cx, cy, cz, r)); roots: buffer_len(NC) elements.
// searches: if not null, the number of root searches this lane ran (of M without pruning).
template <int NC, class Roots>
MTGX_HD void segment_check(const double* c, int N, int D, double T, const double* obstacles, int M, double inflation, Roots& roots,
                           Fold& out, int* searches = nullptr) {
  Segment<NC> S;
  segment_prepare<NC, Roots>(c, N, D, T, S, roots);
  fold_init(out);
  double last_key = -INFINITY;
  int last_h = -1, n = 0;
  for (;;) {
    // the next obstacle in ascending (key, index) order after (last_key, last_h); key = bound, NaN as -infinity
    double key = INFINITY, cx = 0.0, cy = 0.0, cz = 0.0, r = 0.0;
    int h = -1;
    for (int m = 0; m < M; ++m) {
      const double ox = obstacles[4 * m], oy = obstacles[4 * m + 1], oz = obstacles[4 * m + 2], orad = obstacles[4 * m + 3];
      double k = lower_bound<NC>(S, ox, oy, oz, orad, inflation);
      k = k != k ? -INFINITY : k;
      const bool after = k > last_key || (k == last_key && m > last_h);
      const bool first = h < 0 || k < key;   // (ascending m: an equal key keeps the smaller index)
      if (after && first) { key = k; h = m; cx = ox; cy = oy; cz = oz; r = orad; }
    }
    if (h < 0) break;                                   // every obstacle has been searched
    if (key > 0.0 && key > out.clearance) break;        // this one and every later one can neither fail nor lower the minimum
    double v, t;
    bool fails;
    obstacle_clearance<NC, Roots>(S, cx, cy, cz, r, inflation, roots, v, t, fails);
    fold_obstacle(out, h, v, t, fails);
    last_key = key;
    last_h = h;
    ++n;
  }
  if (searches) *searches = n;
}

}  // namespace mtgo
