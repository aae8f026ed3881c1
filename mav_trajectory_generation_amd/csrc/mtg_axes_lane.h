// mtg_axes_lane.h -- per-lane algorithm of the batched per-axis extrema (signed minimum and maximum of one axis).
//
// What it replaces, per polynomial: Polynomial::computeMinMax(0, T, q, &min, &max) -> selectMinMaxFromCandidates
// (src/polynomial.cpp:102-143) for a contiguous range of orders q = FIRST .. FIRST + n - 1 within position .. snap.  The
// candidates of order q are 0, T and the real roots in [0, T] of p^(q+1), ascending; the running pair starts at (0, DBL_MAX) /
// (0, -DBL_MAX) and both comparisons are strict, so the first candidate wins a tie.
//
// ONE root search per axis serves every order: the derivative chain that isolates the roots of g = p^(FIRST+1) (degree
// M = NC - 2 - FIRST, real_roots_unit of mtg_extrema_lane.h) passes through p^(FIRST+2), p^(FIRST+3), ..: level K of the chain
// holds the roots of p^(FIRST+1+M-K), the critical points of order FIRST + M - K.  The sink below sees each level's roots before
// the next level overwrites them, evaluates p^(order) there (Polynomial::evaluate's Horner form, mtgr::axis_at) and folds the
// value into that order's running row; no root list is stored.  The levels of the orders that can be asked for are refined to
// kRootTol (TIGHT), the ones above them only partition [0, 1].  Orders >= NC - 2 have a constant or zero derivative: no
// interior candidates; where p^(FIRST+1) has fewer than two coefficients nothing is searched.
//
// One departure from the reference: a (segment, axis, order) with a NaN candidate value reports (0, NaN, 0, NaN) instead of
// the DBL_MAX / lowest sentinels the strict comparisons would leave; in the reduction over segments the first NaN row wins.
// Same code runs on the device (mtg_axes.hip) and on the host (mtg_axes_host.cpp).
#pragma once

#include "mtg_recursive_lane.h"

namespace mtga {

constexpr int kMaxOrder = 4;        // snap
constexpr int kMinCoeffs = 2;
constexpr int kMinInstance = 4;     // N = 2, 3 run in 4
constexpr int kMaxDimension = 8;    // nothing is held per trajectory across axes

using Row = mtgx::MinMax;           // (t_min, v_min, t_max, v_max)

// what both entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         long long derivative_first, long long n_derivatives) {
  if (!mtgs::shape_ok(n_coeffs, kMinCoeffs, n_segments, dimension, kMaxDimension, batch, ts_b, ts_k)) return false;
  if (derivative_first < 0 || derivative_first > kMaxOrder || n_derivatives < 1 || n_derivatives > kMaxOrder + 1) return false;
  const long long last = derivative_first + n_derivatives - 1;
  return last <= kMaxOrder && last <= n_coeffs - 1;   // (polynomial.cpp:70-73: N - derivative - 1 >= 0)
}

constexpr int degree(int nc, int first) { return nc - 2 - first; }                      // M: degree of p^(first+1)
constexpr int roots_len(int nc, int first) { return degree(nc, first) >= 1 ? 2 * degree(nc, first) : 1; }
constexpr int orders(int first) { return kMaxOrder + 1 - first; }                       // rows a lane may be asked for
constexpr int tight(int nc, int first) { return orders(first) < degree(nc, first) ? orders(first) : degree(nc, first); }

MTGX_HD void fold(Row& r, bool& nan, double t, double v) {   // polynomial.cpp:131-141
  if (v < r.v_min) { r.t_min = t; r.v_min = v; }
  if (v > r.v_max) { r.t_max = t; r.v_max = v; }
  nan = nan || v != v;
}

template <int NC, int FIRST, class Buf>
struct FoldSink {
  const double (&p)[NC];
  double T;
  int n;                          // orders asked for
  Row (&row)[orders(FIRST)];
  bool (&nan)[orders(FIRST)];
  template <int K>
  MTGX_HD void level(Buf& roots, int src, int cnt) {
    constexpr int j = degree(NC, FIRST) - K;   // level K <-> order FIRST + j
    if constexpr (j < orders(FIRST)) {
      if (j < n)
        for (int i = 0; i < cnt; ++i) {
          // (a Newton step towards a root AT 0 or 1 -- a rest-to-rest segment's derivatives vanish at its ends -- can leave [0, 1]
          // by a rounding error: seen on the device, whose step takes the reciprocal instruction, as tau = -5e-18.  The reference
          // drops candidates outside [0, T] (polynomial.cpp:56); the end itself is folded already and wins the tie)
          const double t = fmin(fmax(roots[src + i], 0.0), 1.0) * T;
          fold(row[j], nan[j], t, mtgr::axis_at<NC, FIRST + j>(p, t));
        }
    }
  }
};

template <int NC, int FIRST, int J = 0>
MTGX_HD void fold_ends(const double (&p)[NC], double T, int n, Row (&row)[orders(FIRST)], bool (&nan)[orders(FIRST)]) {
  if constexpr (J < orders(FIRST)) {
    row[J] = Row{0.0, DBL_MAX, 0.0, -DBL_MAX};
    nan[J] = false;
    if (J < n) {
      fold(row[J], nan[J], 0.0, mtgr::axis_at<NC, FIRST + J>(p, 0.0));
      fold(row[J], nan[J], T, mtgr::axis_at<NC, FIRST + J>(p, T));
    }
    fold_ends<NC, FIRST, J + 1>(p, T, n, row, nan);
  }
}

// One axis of one segment.  c = N coefficients (increasing powers), N <= NC (zero-padded tail), T = segment time, n orders
// FIRST .. FIRST + n - 1 into row[0 .. n).  roots: roots_len(NC, FIRST) elements.
template <int NC, int FIRST, class Buf>
MTGX_HD void axis_minmax(const double* c, int N, double T, int n, Buf& roots, Row (&row)[orders(FIRST)]) {
  double p[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) p[i] = i < N ? c[i] : 0.0;
  bool nan[orders(FIRST)];
  fold_ends<NC, FIRST>(p, T, n, row, nan);
  constexpr int M = degree(NC, FIRST);
  if constexpr (M >= 1) {
    constexpr int L = M + 1;   // coefficient count of g = p^(FIRST+1) in tau = t / T (as mtgr::axis_roots builds it)
    double g[L];
    double tp = 1.0;
#pragma unroll
    for (int j = 0; j < L; ++j) {
      g[j] = p[j + FIRST + 1] * mtgf::ff(j + FIRST + 1, FIRST + 1) * tp;
      tp *= T;
    }
    FoldSink<NC, FIRST, Buf> sink{p, T, n, row, nan};
    int base = 0;
    mtgx::real_roots_unit<L, Buf, false, tight(NC, FIRST), FoldSink<NC, FIRST, Buf>>(g, roots, base, mtgx::Share{0, 1, 1}, &sink);
  }
#pragma unroll
  for (int j = 0; j < orders(FIRST); ++j)
    if (nan[j]) row[j] = Row{0.0, NAN, 0.0, NAN};
}

// Reduction over the K segments of one (trajectory, axis, order): rows at seg[k * stride .. + 4), in segment order.  The first
// segment with the strictly smallest / largest value, and that segment's time and value; the first NaN row wins both.
MTGX_HD void reduce_rows(const double* seg, long long stride, int K, Row& out, int& k_min, int& k_max) {
  out = Row{seg[0], seg[1], seg[2], seg[3]};
  k_min = 0;
  k_max = 0;
  bool nan = out.v_min != out.v_min || out.v_max != out.v_max;
  for (int k = 1; k < K && !nan; ++k) {
    const double* r = seg + (long long)k * stride;
    if (r[1] != r[1] || r[3] != r[3]) {
      out = Row{r[0], r[1], r[2], r[3]};
      k_min = k;
      k_max = k;
      nan = true;
    } else {
      if (r[1] < out.v_min) { out.t_min = r[0]; out.v_min = r[1]; k_min = k; }
      if (r[3] > out.v_max) { out.t_max = r[2]; out.v_max = r[3]; k_max = k; }
    }
  }
}

// f(std::integral_constant<int, FIRST>) for FIRST = derivative_first in 0 .. 4
template <int FIRST = 0, class F>
inline void with_first(int derivative_first, F&& f) {
  if constexpr (FIRST == kMaxOrder) f(std::integral_constant<int, FIRST>{});
  else if (derivative_first == FIRST) f(std::integral_constant<int, FIRST>{});
  else with_first<FIRST + 1>(derivative_first, f);
}

}  // namespace mtga
