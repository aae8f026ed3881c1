// mtg_collision_lane.h -- lane code of the batched distance-field collision cost and its gradient (mtg_collision_cost,
// include/mtg_hip.h): per segment  sum_i w_i c(d(p(t_i)) - inflation) s(t_i)  on the sample grid of the distance-field check, a
// trapezoid rule of the CHOMP objective  int c(d(p(t))) ||v(t)|| dt,  and the exact derivative of that sum with respect to the
// polynomial coefficients.  Here: the weights, one sample's terms, the 64 partial sums and their butterfly.  Host + device, plain
// C++17; the kernel is mtg_collision.hip, the serial loop over the same functions mtg_collision_host.cpp.
//
// Every rounding is fixed so that a host loop reproduces each choice (the specification is the comment block in mtg_hip.h); fl()
// is one float64 rounding, every fma a fused multiply-add, nothing else is fused:
//   samples    mtgf::sample_count and mtgf::sample_time: t_0 = 0, t_i = fl(i dt) < T, then T; S of them.  S > max_samples: the
//              segment is not sampled: cost NaN, gradient NaN, sample count -1
//   weights    trapezoid on that grid: w_0 = fl(fl(t_1 - t_0) 0.5), w_i = fl(fl(t_{i+1} - t_{i-1}) 0.5),
//              w_{S-1} = fl(fl(t_{S-1} - t_{S-2}) 0.5); T <= 0: every weight is 0; T NaN: the weights are NaN by the same formula
//   p, v       per axis 0-2, from the highest coefficient down: v = fma(v, t, p); p = fma(p, t, c_j), both from 0
//   d          mtgf::voxel_coordinates and mtgf::lookup_voxel, operation for operation
//   G          inside the grid, from the lookup's own eight voxels, f_a, x**, y*, and r, with lerp_a(lo, hi) = fma(f_a, hi - lo, lo)
//              and e** = the four (hi - lo) x-differences:  G_x = fl(r lerp_z(lerp_y(e00, e10), lerp_y(e01, e11))),
//              G_y = fl(r lerp_z(x10 - x00, x11 - x01)),  G_z = fl(r fl(y1 - y0)).  Outside: d = outside_distance, G = 0.
//              A NaN u_a: d and G are NaN.
//   potential  x = fl(d - inflation).  x < 0: c = fl(fl(epsilon 0.5) - x), c' = -1.  x <= epsilon: q = fl(x - epsilon),
//              c = fl(fl(q q) / fl(2 epsilon)), c' = fl(q / epsilon).  x > epsilon: c = c' = 0 and the sample adds NOTHING to any
//              sum (it is skipped, whatever s and G are).  x NaN: c = c' = NaN.
//   speed      s = sqrt(fma(v_z, v_z, fma(v_y, v_y, fma(v_x, v_x, fl(speed_epsilon speed_epsilon)))))
//   cost term  fl(fl(w c) s)
//   gradient   k1 = fl(fl(w c') s), A_a = fl(k1 G_a);  k2 = fl(fl(w c) / s), 0 if s == 0, B_a = fl(k2 v_a);
//              q_0 = 1, q_j = fl(q_{j-1} t);  entry (a, j): acc = fma(A_a, q_j, acc), then for j >= 1
//              acc = fma(B_a, fl(j q_{j-1}), acc)
//   sums       64 partial sums per output, each from +0: partial g takes samples g, g + 64, .. in ascending order (cost: plain
//              additions); then P[l] = fl(P[l] + P[l xor off]) for off = 32, 16, 8, 4, 2, 1.  IEEE addition commutes, so after
//              the last step all 64 hold the same total.
//   yaw        a 4th dimension is never read; its N gradient entries are 0 in every segment, also one that is not sampled
//   trajectory the sum of segment_cost over the segments in ascending order, from +0
// Contraction is OFF for this header: fusing w c s or the weights changes results between host and device.
#pragma once

#include "mtg_field_lane.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace mtgc {

constexpr int kMinInstance = mtgf::kMinInstance;
constexpr int kPartials = 64;   // partial sums per output: the lanes of a wavefront

struct Potential {
  double inflation, epsilon, half_epsilon, two_epsilon, speed_epsilon2;   // fl(epsilon 0.5), fl(2 epsilon), fl(speed_epsilon^2)
};

// what both entry points accept on top of mtgf::arguments_ok; fills g and q
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         const mtg_distance_field* f, double dt, int max_samples, double inflation, double epsilon, double speed_epsilon,
                         mtgf::Grid* g, Potential* q) {
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, ts_b, ts_k, f, dt, max_samples, inflation, g)) return false;
  if (f->interpolation != MTG_FIELD_TRILINEAR) return false;
  if (!(epsilon > 0.0) || !(epsilon <= DBL_MAX) || !(speed_epsilon >= 0.0) || !(speed_epsilon <= DBL_MAX)) return false;
  q->inflation = inflation; q->epsilon = epsilon; q->half_epsilon = epsilon * 0.5; q->two_epsilon = 2.0 * epsilon;
  q->speed_epsilon2 = speed_epsilon * speed_epsilon;
  return true;
}

// trapezoid weight of sample i of S
MTGX_HD double sample_weight(int i, int S, double T, double dt) {
  if (T <= 0.0) return 0.0;
  const double lo = mtgf::sample_time(i > 0 ? i - 1 : 0, S, T, dt), hi = mtgf::sample_time(i < S - 1 ? i + 1 : S - 1, S, T, dt);
  return (hi - lo) * 0.5;
}

// d and G at voxel coordinates u of a trilinear grid: d is mtgf::lookup_voxel's value, operation for operation
MTGX_HD double lookup_gradient(const mtgf::Grid& g, const double (&u)[3], double (&G)[3]) {
  if (u[0] != u[0] || u[1] != u[1] || u[2] != u[2]) { G[0] = G[1] = G[2] = NAN; return NAN; }
  const int n[3] = {g.nx, g.ny, g.nz};
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) inside = inside && u[a] >= 0.0 && u[a] <= (double)(n[a] - 1);
  if (!inside) { G[0] = G[1] = G[2] = 0.0; return g.outside; }
  int i[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int fl = (int)floor(u[a]);
    i[a] = fl < n[a] - 2 ? fl : n[a] - 2;
    f[a] = u[a] - (double)i[a];
  }
  const float* base = g.d + ((long long)i[2] * g.ny + i[1]) * (long long)g.nx + i[0];
  const long long sy = g.nx, sz = (long long)g.nx * g.ny;
  float v00[2], v10[2], v01[2], v11[2];
  mtgf::load2(base, v00);
  mtgf::load2(base + sy, v10);
  mtgf::load2(base + sz, v01);
  mtgf::load2(base + sz + sy, v11);
  const double e00 = (double)v00[1] - (double)v00[0], e10 = (double)v10[1] - (double)v10[0];
  const double e01 = (double)v01[1] - (double)v01[0], e11 = (double)v11[1] - (double)v11[0];
  const double x00 = fma(f[0], e00, (double)v00[0]);
  const double x10 = fma(f[0], e10, (double)v10[0]);
  const double x01 = fma(f[0], e01, (double)v01[0]);
  const double x11 = fma(f[0], e11, (double)v11[0]);
  const double dy0 = x10 - x00, dy1 = x11 - x01;
  const double y0 = fma(f[1], dy0, x00);
  const double y1 = fma(f[1], dy1, x01);
  const double dz = y1 - y0;
  const double ex0 = fma(f[1], e10 - e00, e00), ex1 = fma(f[1], e11 - e01, e01);
  G[0] = g.r * fma(f[2], ex1 - ex0, ex0);
  G[1] = g.r * fma(f[2], dy1 - dy0, dy0);
  G[2] = g.r * dz;
  return fma(f[2], dz, y0);
}

// One lane's sums: the cost and, with GRAD, the 3 NC gradient entries [axis][power]
template <int NC, bool GRAD>
struct Sums {
  double cost;
  double grad[GRAD ? 3 : 1][GRAD ? NC : 1];
};
template <int NC, bool GRAD>
MTGX_HD void clear(Sums<NC, GRAD>& s) {
  s.cost = 0.0;
#pragma unroll
  for (int a = 0; a < (GRAD ? 3 : 1); ++a)
#pragma unroll
    for (int j = 0; j < (GRAD ? NC : 1); ++j) s.grad[a][j] = 0.0;
}
// P = P + Q, entry by entry (one step of the butterfly)
template <int NC, bool GRAD>
MTGX_HD void add(Sums<NC, GRAD>& p, const Sums<NC, GRAD>& q) {
  p.cost = p.cost + q.cost;
  if constexpr (GRAD) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < NC; ++j) p.grad[a][j] = p.grad[a][j] + q.grad[a][j];
  }
}

// samples first, first + step, .. < S of one segment into s; p: the segment's position polynomials, zero-padded to NC
template <int NC, bool GRAD>
MTGX_HD void sum_samples(const double (&p)[3][NC], double T, double dt, int S, int first, int step, const mtgf::Grid& g,
                         const Potential& q, Sums<NC, GRAD>& s) {
  for (int i = first; i < S; i += step) {
    const double t = mtgf::sample_time(i, S, T, dt);
    const double w = sample_weight(i, S, T, dt);
    double x[3], v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double r = 0.0, dr = 0.0;
#pragma unroll
      for (int j = NC - 1; j >= 0; --j) { dr = fma(dr, t, r); r = fma(r, t, p[a][j]); }
      x[a] = r; v[a] = dr;
    }
    double u[3], G[3];
    mtgf::voxel_coordinates(g, x, u);
    const double d = lookup_gradient(g, u, G);
    const double e = d - q.inflation;
    double c, dc;
    if (e < 0.0) { c = q.half_epsilon - e; dc = -1.0; }
    else if (e <= q.epsilon) { const double h = e - q.epsilon; c = (h * h) / q.two_epsilon; dc = h / q.epsilon; }
    else if (e > q.epsilon) continue;
    else { c = NAN; dc = NAN; }
    const double speed = sqrt(fma(v[2], v[2], fma(v[1], v[1], fma(v[0], v[0], q.speed_epsilon2))));
    const double wc = w * c;
    s.cost = s.cost + wc * speed;
    if constexpr (GRAD) {
      const double k1 = (w * dc) * speed;
      const double k2 = speed == 0.0 ? 0.0 : wc / speed;
      double A[3], B[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) { A[a] = k1 * G[a]; B[a] = k2 * v[a]; }
      double pw = 1.0, below = 0.0;   // t^j and j t^(j-1)
#pragma unroll
      for (int j = 0; j < NC; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          s.grad[a][j] = fma(A[a], pw, s.grad[a][j]);
          if (j >= 1) s.grad[a][j] = fma(B[a], below, s.grad[a][j]);
        }
        below = (double)(j + 1) * pw;
        pw = pw * t;
      }
    }
  }
}

}  // namespace mtgc
