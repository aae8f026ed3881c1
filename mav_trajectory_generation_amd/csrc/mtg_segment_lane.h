// mtg_segment_lane.h -- what the per-segment root-search checks share around their lane algorithms (mtg_feasibility_lane.h,
// mtg_objective_lane.h, mtg_halfplane_lane.h): the shape rules of a [B][K][D][N] batch with strided times, the zero-padded
// coefficient load, the squared magnitude's derivative and the magnitude itself, the even-instantiation dispatch and the
// first-failure word.  Host + device, plain C++17; the device-only half of the frame is mtg_segment_kernel.h.
#pragma once

#include <type_traits>

#include "mtg_extrema_lane.h"

namespace mtgs {

// the shape every check accepts: N in [min_coeffs, 12], K >= 1, D in [1, max_dimension], batch >= 0, times at b*ts_b + k*ts_k
inline bool shape_ok(int n_coeffs, int min_coeffs, int n_segments, int dimension, int max_dimension, long long batch,
                     long long ts_b, long long ts_k) {
  if (n_coeffs < min_coeffs || n_coeffs > mtgx::kMaxCoeffs || n_segments < 1 || dimension < 1 || dimension > max_dimension || batch < 0)
    return false;
  if (ts_b < 1 || ts_k < 1) return false;
  // [B][K] with rows at least K apart, or [K][B] with rows at least B apart: anything else aliases two segments' times
  return ts_b >= (long long)n_segments * ts_k || ts_k >= batch * ts_b;
}

// c = [D][N] coefficients (increasing powers) into p[DC][NC], N <= NC; the tails are zero: identically-zero leading levels of
// the derivative chains fall through real_roots_unit, a dimension of zeros adds nothing to a magnitude or to its derivative
template <int NC, int DC>
MTGX_HD void load_padded(const double* c, int N, int D, double (&p)[DC][NC]) {
#pragma unroll
  for (int d = 0; d < DC; ++d)
#pragma unroll
    for (int i = 0; i < NC; ++i) p[d][i] = (d < D && i < N) ? c[d * N + i] : 0.0;
}

// || p^(DER)(t) [+ off] || over DC dimensions (Polynomial::evaluate: Horner over base(DER, i) c_i from the highest power down;
// OFFSET: off joins the constant term, as in the thrust segment's coefficients, feasibility_analytic.cpp:138-144)
template <int NC, int DC, int DER, bool OFFSET>
MTGX_HD double magnitude_at(const double (&p)[DC][NC], const double* off, double t) {
  double acc = 0.0;
#pragma unroll
  for (int d = 0; d < DC; ++d) {
    double r = 0.0;
#pragma unroll
    for (int i = NC - 1; i >= DER; --i) {
      double a = mtgx::falling_factorial(i, DER) * p[d][i];
      if constexpr (OFFSET) { if (i == DER) a += off[d]; }
      r = fma(r, t, a);
    }
    acc = fma(r, r, acc);
  }
  return sqrt(acc);
}

// g = d/dtau || p^(DER) [+ off] ||^2 / 2 in tau = t / T: sum over the dimensions of u u' (the convolved polynomial of
// segment.cpp:96-115); its real roots in [0, 1] are the magnitude's interior critical points
template <int NC, int DC, int DER, bool OFFSET>
MTGX_HD void magnitude_derivative(const double (&p)[DC][NC], const double* off, double T, double (&g)[2 * (NC - DER) - 2]) {
  constexpr int NQ = NC - DER;
#pragma unroll
  for (int j = 0; j < 2 * NQ - 2; ++j) g[j] = 0.0;
#pragma unroll
  for (int d = 0; d < DC; ++d) {
    double u[NQ];
    double tp = 1.0;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      if constexpr (OFFSET) u[i] = (p[d][i + DER] * mtgx::falling_factorial(i + DER, DER) + (i == 0 ? off[d] : 0.0)) * tp;
      else u[i] = p[d][i + DER] * mtgx::falling_factorial(i + DER, DER) * tp;
      tp *= T;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int j = 0; j + 1 < NQ; ++j) g[i + j] = fma(u[i], (double)(j + 1) * u[j + 1], g[i + j]);
  }
}

// An odd N, and one below the smallest instantiation, runs in the next even one on zero-padded coefficients.
constexpr int even_instance(int n_coeffs, int min_instance) { return n_coeffs <= min_instance ? min_instance : (n_coeffs + 1) & ~1; }

// f(std::integral_constant<int, NC>) for NC = even_instance(n_coeffs, MIN) in {MIN, MIN + 2, .., 12}
template <int MIN, int NC = MIN, class F>
inline void with_instance(int n_coeffs, F&& f) {
  static_assert(MIN >= 2 && MIN % 2 == 0 && NC <= mtgx::kMaxCoeffs, "instantiations are (2,) 4, 6, 8, 10, 12");
  if constexpr (NC == mtgx::kMaxCoeffs) f(std::integral_constant<int, NC>{});
  else if (even_instance(n_coeffs, MIN) == NC) f(std::integral_constant<int, NC>{});
  else with_instance<MIN, NC + 2>(n_coeffs, f);
}

// First failure of a trajectory as one int: the smallest word over the failing segments is the first in SEGMENT order and,
// within it, the smallest code (a result code, or a plane's index in list order)
constexpr int kNoFailure = 0x7fffffff;
MTGX_HD int failure_word(int segment, int code) { return (segment << 8) | code; }
MTGX_HD int failure_segment(int word) { return word >> 8; }
MTGX_HD int failure_code(int word) { return word & 0xff; }

}  // namespace mtgs
