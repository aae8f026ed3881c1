// mtg_separation_lane.h -- per-lane algorithm of the batched trajectory-to-trajectory separation check.
//
// What it answers, per PAIR (trajectory a of side A, trajectory b of side B): do the two keep min_separation between their
// centres at every instant both fly, where do they first come too close, and what is the exact minimum distance.  A second
// trajectory is a sphere of radius 0 whose centre is a polynomial, so the numerical tools are the sphere check's
// (mtg_obstacle_lane.h): magnitude_derivative / magnitude_at, real_roots_unit unchanged, Bernstein control-point hulls.  What is
// new: the two sides have their own segment times and start times, their breakpoints do not line up, and the minimum is taken
// PIECE by piece over the merged breakpoints.
//
// Breakpoints (walk()).  ea[0] = start_a, ea[i + 1] = ea[i] + Ta[i]: one rounded float64 addition per step, in segment order;
// eb likewise.  A piece is a pair (i, j) with lo = max(ea[i], eb[j]) < hi = min(ea[i + 1], eb[j + 1]).  Along a pair the pieces
// are ordered in time, i + j increases strictly (it is the piece's rank), there are at most Ka + Kb - 1.
//
// The difference curve of a piece.  sa = lo - ea[i], sb = lo - eb[j], L = hi - lo, d(tau) = pA_i(sa + tau L) - pB_j(sb + tau L),
// tau in [0, 1].  shift_scale() is the Taylor shift and scaling of one axis of one side: u[i] = L^i sum_{k >= i} C(k, i) p[k]
// s^(k - i), a Horner chain in s per coefficient (NC^2 / 2 FMAs).  d[i] = uA[i] - uB[i], one rounded subtraction.  Two sides
// that are the same segment at the same local time give d = 0 exactly.
//
// Candidates and the fold.  tau = 0 and tau = 1 exactly and the real roots in [0, 1] of g = sum_dim d d' (magnitude_derivative
// of d with T = 1, real_roots_unit).  separation = || d(tau) || - min_separation over dimensions 0-2 (a 4th, yaw, dimension is never
// read); a piece fails iff a candidate has !(separation > 0).  Within a piece: 0, 1, roots ascending, strict <, the first NaN
// wins.  Across pieces: the earliest piece wins a tie, a NaN wins every minimum it enters (the earliest NaN stays), the first
// failing piece is the earliest in time.  Times are global: lo + tau L.
//
// Degenerate pairs.  No piece (the two never fly at the same time, or touch at an instant only): feasible, separation +inf,
// time NaN, indices -1, 0 pieces.  A segment time that is negative or not finite, or a start that is not finite, on either
// side: the pair is INVALID -- infeasible, separation NaN, times NaN, indices -1, 0 pieces.  So is a pair whose index is out of range
// (the callers check the index before anything of the pair is read).
//
// Pruning.  A lane is one (pair, segment i of A); it walks the overlapping segments j of B in time order and owns the running
// minimum it prunes against.  Per piece, a lower bound of every separation the evaluation can COMPUTE on the piece: the hulls
// of the two sides' Bernstein control points on the piece (a polynomial on [0, 1] lies in the hull of its control points; the
// basis change is NC^2 / 2 FMAs per axis and side), per axis the gap between the two hulls, less an allowance.  The allowance
// per axis is kHullUlps ulps of E = EA + EB, EA = sum_i |uA[i]| (and EB):
//   * the basis change of each side, weights C(k, i) / C(n, i) in [0, 1]: (NC + 2) ulps of EA and of EB;
//   * the subtraction d[i] = uA[i] - uB[i]: half an ulp of |d[i]|, together below 1 ulp of E;
//   * the Horner chain of the evaluation over d, sum |d[i]| <= E: 2 NC ulps of E;
// 3 NC + 3 = 39 ulps of E at NC = 12, 64 with room to spare.  The norm (three FMAs and a square root) and the subtraction of
// min_separation are covered by kNormUlps ulps of their operands, as in mtg_obstacle_lane.h.  A piece is skipped only when its bound
// is > 0 (it cannot fail) and strictly above the lane's running minimum (it can neither lower the minimum nor tie it).  A NaN
// bound -- any coefficient of the piece not finite -- compares false and skips nothing.  The piece COUNT includes skipped pieces.
//
// N = 1 .. 12 run in the next even instantiation (at least 4) on zero-padded coefficients: the padding adds exact zeros to
// every chain.  Same code runs on the device (mtg_separation.hip) and on the host (mtg_separation_host.cpp).
#pragma once

#include "mtg_obstacle_lane.h"

namespace mtgp {

constexpr int kMinInstance = 4;
constexpr int kMaxSegments = 1024;      // per side: (i + j) << 10 | j orders the pieces of a pair in time and fits an int
constexpr int kSegmentBits = 10;
constexpr long long kMaxLanes = 0x7fffffffll;   // n_pairs * n_segments_a
constexpr double kHullUlps = 64.0;      // allowance per axis, in ulps of EA + EB (see above)
constexpr double kNormUlps = 8.0;
constexpr int kInvalidPair = -1;        // a pair's first-failure word: below every piece's word

// a pair's first-failure word: the smallest over the failing pieces is the earliest in time
MTGX_HD int piece_word(int i, int j) { return ((i + j) << kSegmentBits) | j; }
MTGX_HD int piece_segment_b(int word) { return word & (kMaxSegments - 1); }
MTGX_HD int piece_segment_a(int word) { return (word >> kSegmentBits) - piece_segment_b(word); }

// what both entry points accept of one side (include/mtg_hip.h)
inline bool side_ok(int n_coeffs, int dimension, int n_segments, long long batch, long long ts_b, long long ts_k) {
  return mtgs::shape_ok(n_coeffs, 1, n_segments, dimension, 4, batch, ts_b, ts_k) && dimension >= 3 && n_segments <= kMaxSegments;
}
inline bool arguments_ok(int n_coeffs, int dimension, int ka, long long ba, long long tsa_b, long long tsa_k, int kb, long long bb,
                         long long tsb_b, long long tsb_k, long long n_pairs, double min_separation) {
  return side_ok(n_coeffs, dimension, ka, ba, tsa_b, tsa_k) && side_ok(n_coeffs, dimension, kb, bb, tsb_b, tsb_k) && n_pairs >= 0 &&
         n_pairs <= kMaxLanes / ka && min_separation >= 0.0 && min_separation <= DBL_MAX;
}
// the three pair-closest outputs are found by a scan of the first three per-segment outputs
inline bool outputs_ok(const void* closest_time, const void* closest_a, const void* closest_b, const void* seg_separation,
                       const void* seg_time, const void* seg_b) {
  return !(closest_time || closest_a || closest_b) || (seg_separation && seg_time && seg_b);
}

constexpr int roots_len(int nc) { return 2 * (2 * nc - 3); }          // the two buffers of real_roots_unit<2 nc - 2>
constexpr int buffer_len(int nc) { return roots_len(nc) + 3 * nc; }   // the lane's buffer: the root buffers, then d [3][nc]

// one trajectory of one side: c [K][D][N], its times at t[k * ts_k], its global start time
struct Side {
  const double* c;
  const double* t;
  long long ts_k;
  int K;
  double start;
};

// The breakpoint walk of a lane: [e0, e1] = [ea[i], ea[i + 1]], and whether every time and start of BOTH sides is usable.
MTGX_HD bool walk(const Side& A, const Side& B, int i, double& e0, double& e1) {
  bool ok = A.start >= -DBL_MAX && A.start <= DBL_MAX && B.start >= -DBL_MAX && B.start <= DBL_MAX;
  double e = A.start;
  e0 = e1 = e;
  for (int k = 0; k < A.K; ++k) {
    const double T = A.t[(long long)k * A.ts_k];
    ok = ok && T >= 0.0 && T <= DBL_MAX;
    if (k == i) e0 = e;
    e = e + T;
    if (k == i) e1 = e;
  }
  for (int k = 0; k < B.K; ++k) {
    const double T = B.t[(long long)k * B.ts_k];
    ok = ok && T >= 0.0 && T <= DBL_MAX;
  }
  return ok;
}

// One axis of one segment on a piece: u[i] = L^i sum_{k >= i} C(k, i) p[k] s^(k - i), p = c[0 .. N) zero-padded to NC.
// e = sum |u[i]|; lo, hi = hull of the Bernstein control points of u on [0, 1] (NaN if anything is not finite).
template <int NC>
MTGX_HD void shift_scale(const double* c, int N, double s, const double (&lpow)[NC], double (&u)[NC], double& e, double& lo, double& hi) {
  double p[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) p[k] = k < N ? c[k] : 0.0;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    double r = p[NC - 1] * mtgo::binomial(NC - 1, i);
#pragma unroll
    for (int k = NC - 2; k >= i; --k) r = fma(r, s, mtgo::binomial(k, i) * p[k]);
    u[i] = r * lpow[i];
    sum += fabs(u[i]);
  }
  constexpr int n = NC - 1;
  double b[NC];
  b[0] = u[0];
#pragma unroll
  for (int k = 1; k <= n; ++k) {
    double v = u[0];   // control point k = sum_{i <= k} C(k, i) / C(n, i) u[i]
#pragma unroll
    for (int i = 1; i <= k; ++i) v = fma(mtgo::binomial(k, i) / mtgo::binomial(n, i), u[i], v);
    b[k] = v;
  }
  mtgo::hull<NC>(b, !(sum <= DBL_MAX), lo, hi);
  e = sum;
}

// The piece's difference curve into buf[roots_len .. roots_len + 3 NC) and the lower bound of the header comment.
template <int NC, class Roots>
MTGX_HD double piece_prepare(const double* ca, const double* cb, int N, double sa, double sb, double L, double min_separation, Roots& buf) {
  double lpow[NC];
  lpow[0] = 1.0;
#pragma unroll
  for (int i = 1; i < NC; ++i) lpow[i] = lpow[i - 1] * L;
  double acc = 0.0;
  bool nan = false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double ua[NC], ub[NC], ea, eb, alo, ahi, blo, bhi;
    shift_scale<NC>(ca + d * N, N, sa, lpow, ua, ea, alo, ahi);
    shift_scale<NC>(cb + d * N, N, sb, lpow, ub, eb, blo, bhi);
#pragma unroll
    for (int i = 0; i < NC; ++i) buf[roots_len(NC) + d * NC + i] = ua[i] - ub[i];
    const double below = alo - bhi, above = blo - ahi, margin = kHullUlps * DBL_EPSILON * (ea + eb);
    double gap = (below > above ? below : above) - margin;
    gap = gap < 0.0 ? 0.0 : gap;
    nan = nan || below != below || above != above || margin != margin;
    acc = fma(gap, gap, acc);
  }
  if (nan) acc = NAN;
  const double dist = sqrt(acc);
  return dist - min_separation - kNormUlps * DBL_EPSILON * (dist + min_separation);
}

// The search and the evaluation of the piece whose difference curve piece_prepare left in buf.  Never pruned.
template <int NC, class Roots>
MTGX_HD void piece_separation(double min_separation, Roots& buf, double& v_min, double& tau_min, bool& fails) {
  constexpr int LG = 2 * NC - 2;
  int cnt = 0, base = 0;
  {
    double d[3][NC], g[LG];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < NC; ++i) d[k][i] = buf[roots_len(NC) + k * NC + i];
    mtgs::magnitude_derivative<NC, 3, 0, false>(d, nullptr, 1.0, g);
    cnt = mtgx::real_roots_unit<LG, Roots>(g, buf, base);
  }
  double d[3][NC];   // (read again: nothing of the curve stays in registers across the search)
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < NC; ++i) d[k][i] = buf[roots_len(NC) + k * NC + i];
  double best = INFINITY, best_t = 0.0;
  bool nan = false, bad = false;
  for (int i = -2; i < cnt; ++i) {
    // (a Newton step towards a root AT 0 or 1 can leave [0, 1] by a rounding error: the end itself is a candidate already)
    const double tau = i == -2 ? 0.0 : (i == -1 ? 1.0 : fmin(fmax(buf[base + i], 0.0), 1.0));
    const double v = mtgs::magnitude_at<NC, 3, 0, false>(d, nullptr, tau) - min_separation;
    bad = bad || !(v > 0.0);
    if (!nan && (v != v || v < best)) { best = v; best_t = tau; nan = v != v; }
  }
  v_min = best;
  tau_min = best_t;
  fails = bad;
}

// running result of a lane over its pieces, and of a pair over its lanes: both in time order
struct Fold {
  double separation, time;   // minimum so far (the earliest wins a tie, the earliest NaN wins), and its global time
  int segment_a, segment_b;  // the piece that attains it, -1: none
  int failing_a, failing_b;  // the earliest failing piece, -1: none
  int pieces;
  bool invalid;              // unusable times or start: see the header comment
};
MTGX_HD void fold_init(Fold& f) {
  f.separation = INFINITY;
  f.time = NAN;
  f.segment_a = f.segment_b = f.failing_a = f.failing_b = -1;
  f.pieces = 0;
  f.invalid = false;
}
MTGX_HD void fold_invalid(Fold& f) {
  fold_init(f);
  f.separation = NAN;
  f.invalid = true;
}
// a later minimum (one piece's, or one lane's) into the running result
MTGX_HD void fold_minimum(Fold& f, int i, int j, double v, double t) {
  const bool f_nan = f.separation != f.separation;
  if (!f_nan && (v != v || v < f.separation)) { f.separation = v; f.time = t; f.segment_a = i; f.segment_b = j; }
}

// One lane: segment i of A against the segments of B it overlaps in time; buf: buffer_len(NC) elements.
// searches: if not null, the number of root searches this lane ran (of out.pieces without pruning).
template <int NC, class Roots>
MTGX_HD void lane_check(const Side& A, const Side& B, int i, int N, int D, double min_separation, bool prune, Roots& buf, Fold& out,
                        int* searches = nullptr) {
  if (searches) *searches = 0;
  double e0, e1;
  if (!walk(A, B, i, e0, e1)) { fold_invalid(out); return; }
  fold_init(out);
  const double* ca = A.c + (long long)i * (D * N);
  double eb = B.start;
  int j = 0, n = 0;
  for (;;) {
    // the lane's next piece that has to be searched
    double lo = 0.0, len = 0.0;
    int jp = -1;
    while (j < B.K && jp < 0) {
      const double eb1 = eb + B.t[(long long)j * B.ts_k];
      const double l = e0 > eb ? e0 : eb, h = e1 < eb1 ? e1 : eb1;
      if (l < h) {
        ++out.pieces;
        const double bound = piece_prepare<NC, Roots>(ca, B.c + (long long)j * (D * N), N, l - e0, l - eb, h - l, min_separation, buf);
        if (!(prune && bound > 0.0 && bound > out.separation)) { jp = j; lo = l; len = h - l; }
      }
      eb = eb1;
      ++j;
      if (eb >= e1) j = B.K;   // times are >= 0: every later segment of B starts at or after the end of this one of A
    }
    if (jp < 0) break;
    double v, tau;
    bool fails;
    piece_separation<NC, Roots>(min_separation, buf, v, tau, fails);
    fold_minimum(out, i, jp, v, fma(tau, len, lo));
    if (fails && out.failing_b < 0) { out.failing_a = i; out.failing_b = jp; }
    ++n;
  }
  if (searches) *searches = n;
}

}  // namespace mtgp
