// mtg_certify_lane.h -- lane code of the CERTIFIED distance-field check (mtg_certify_distance_field, include/mtg_hip.h): a solved
// segment is covered by a binary tree of time intervals; a node is one sample at its midpoint plus a Lipschitz bound of the field
// over the Taylor reach of the position around that midpoint.  Here: the node rule, the fold over a segment's nodes, the serial
// walk of one segment and the Lipschitz helper's cell rule.  Host + device, plain C++17; the kernel is mtg_certify.hip (a
// wavefront per segment, the frontier in LDS), the serial loop over the same functions mtg_certify_host.cpp.
//
// Every rule is fixed so that a host loop reproduces each choice (the specification is the comment block in mtg_hip.h):
//   node (d, j)  half-width w = T 2^-(d+1) (exact), midpoint m = fl((2 j + 1) w); !(T > 0): one node, w = 0, m = 0 (NaN T: m = T)
//   shift        q = p re-centred at m, for i = 0 .. NC-2: for j = NC-2 down to i: q[j] = fma(m, q[j+1], q[j]); q[0] = p(m) is
//                the sampled check's Horner value bit for bit
//   reach        R_a = fl(w horner_w(|q_a,NC-1| .. |q_a,1|)),  A_a = horner_|m|(|c_a,NC-1| .. |c_a,0|) + |origin_a|,
//                Rh_a = fma(s, A_a, fl(R_a (1 + s))),  Rh = fl(sqrt(fma(Rh_z, Rh_z, fma(Rh_y, Rh_y, Rh_x Rh_x))) (1 + s)),  s = 2^-36
//   sample       c = fl(lookup(p(m)) - inflation); fails iff !(c > 0)
//   box          rho_a = fl(fl(Rh_a r) (1 + s)); inside iff 0 <= u_a - rho_a and u_a + rho_a <= n_a - 1 on every axis, touches iff
//                u_a + rho_a >= 0 and u_a - rho_a <= n_a - 1 on every axis; a NaN u_a - rho_a or u_a + rho_a: the bound is NaN
//   bound        touches: Dc - inflation - L Rh - s (|Dc| + inflation + 2 L / r), Dc = lookup at u clamped to [0, n_a - 1], one
//                rounding per operation from left to right; else +infinity.  Not inside: min with outside_distance - inflation.
//                A NaN wins.
// Contraction is OFF for this header, as for mtg_field_lane.h (the explicit fma calls stay fused multiply-adds).
#pragma once

#include "mtg_field_lane.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace mtgc {

constexpr double kSlack = 0x1p-36;        // s
constexpr int kFrontier = 1024;           // the largest max_frontier: what one frontier buffer holds
constexpr int kMaxMinDepth = 10;          // 2^10 = kFrontier
constexpr int kMaxDepth = 24;             // 2 j + 1 < 2^25 is exact as an int and as a double
constexpr unsigned long long kKeyNone = ~0ull;   // above every key of a double: "nothing yet"

struct Rule {
  double lipschitz, inflation;
  int min_depth, max_depth, max_frontier;
};

// what both entry points accept beyond the sampled check's rules (dt and max_samples do not exist here); fills g
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         const mtg_distance_field* f, double lipschitz, int min_depth, int max_depth, int max_frontier, double inflation,
                         mtgf::Grid* g) {
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, ts_b, ts_k, f, 1.0, 2, inflation, g)) return false;
  if (f->interpolation != MTG_FIELD_TRILINEAR) return false;   // a piecewise-constant field has no Lipschitz constant
  if (!(lipschitz > 0.0) || !(lipschitz <= DBL_MAX)) return false;
  if (min_depth < 0 || min_depth > kMaxMinDepth || max_depth < min_depth || max_depth > kMaxDepth) return false;
  const int least = (1 << min_depth) > 2 ? (1 << min_depth) : 2;
  return max_frontier >= least && max_frontier <= kFrontier;
}

// 2^-e, 1 <= e <= 1022, without a library call
MTGX_HD double pow2_neg(int e) {
  const unsigned long long bits = (unsigned long long)(1023 - e) << 52;
  double x;
  __builtin_memcpy(&x, &bits, sizeof x);
  return x;
}

// the nodes of a segment: lone iff !(T > 0)
MTGX_HD bool lone_node(double T) { return !(T > 0.0); }
MTGX_HD double half_width(double T, int depth) { return lone_node(T) ? 0.0 : T * pow2_neg(depth + 1); }
MTGX_HD double midpoint(double T, int j, double w) { return lone_node(T) ? (T != T ? T : 0.0) : (double)(2 * j + 1) * w; }

struct Node {
  double c;       // the sample's clearance
  double bound;   // lower bound of the clearance over the node's interval
};

// one node; p: the segment's position polynomials, zero-padded to NC
template <int NC>
MTGX_HD Node evaluate_node(const double (&p)[3][NC], double m, double w, const mtgf::Grid& g, const Rule& P) {
  constexpr double s1 = 1.0 + kSlack;
  const double am = fabs(m);
  double x[3], rh[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double q[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) q[j] = p[a][j];
#pragma unroll
    for (int i = 0; i < NC - 1; ++i)
#pragma unroll
      for (int j = NC - 2; j >= i; --j) q[j] = fma(m, q[j + 1], q[j]);
    x[a] = q[0];
    double r = fabs(q[NC - 1]);
#pragma unroll
    for (int k = NC - 2; k >= 1; --k) r = fma(r, w, fabs(q[k]));
    r = r * w;
    double A = 0.0;
#pragma unroll
    for (int j = NC - 1; j >= 0; --j) A = fma(A, am, fabs(p[a][j]));
    A = A + fabs(g.o[a]);
    rh[a] = fma(kSlack, A, r * s1);
  }
  const double reach = sqrt(fma(rh[2], rh[2], fma(rh[1], rh[1], rh[0] * rh[0]))) * s1;
  double u[3];
  mtgf::voxel_coordinates(g, x, u);
  const double d = mtgf::lookup_voxel(g, u);
  Node nd;
  nd.c = d - P.inflation;
  const int n[3] = {g.nx, g.ny, g.nz};
  bool inside = true, touches = true, at = true, nan_box = false;
  double uc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double rho = (rh[a] * g.r) * s1, top = (double)(n[a] - 1);
    nan_box = nan_box || u[a] - rho != u[a] - rho || u[a] + rho != u[a] + rho;
    inside = inside && 0.0 <= u[a] - rho && u[a] + rho <= top;
    touches = touches && u[a] + rho >= 0.0 && u[a] - rho <= top;
    uc[a] = u[a] < 0.0 ? 0.0 : (u[a] > top ? top : u[a]);
    at = at && uc[a] == u[a];
  }
  unsigned long long key = mtgf::order_key(INFINITY);
  if (touches) {
    const double dc = at ? d : mtgf::lookup_voxel(g, uc);
    const double b = dc - P.inflation - P.lipschitz * reach - kSlack * (fabs(dc) + P.inflation + 2.0 * P.lipschitz / g.r);
    key = mtgf::order_key(b);
  }
  if (!inside) {
    const unsigned long long out = mtgf::order_key(g.outside - P.inflation);
    if (out < key) key = out;
  }
  nd.bound = nan_box ? NAN : mtgf::order_value(key);
  return nd;
}

// The fold over a set of nodes: minima of order keys, a sum and flags -- associative and commutative, so any split of a
// segment's nodes over lanes gives the same result.
struct Fold {
  unsigned long long c_key = kKeyNone, c_time = kKeyNone;   // smallest (key of c, key of m), smaller key first, then smaller m
  unsigned long long failing_time = kKeyNone;               // smallest key of m over the failing samples
  unsigned long long bound_key = kKeyNone;                  // smallest key of bound over the terminal nodes
  int undecided = 0;                                        // a terminal node at max_depth that is neither failing nor certified
};
MTGX_HD void combine(Fold& a, unsigned long long c_key, unsigned long long c_time, unsigned long long failing_time,
                     unsigned long long bound_key, int undecided) {
  if (c_key < a.c_key || (c_key == a.c_key && c_time < a.c_time)) { a.c_key = c_key; a.c_time = c_time; }
  if (failing_time < a.failing_time) a.failing_time = failing_time;
  if (bound_key < a.bound_key) a.bound_key = bound_key;
  a.undecided |= undecided;
}

// node (m, nd) of a level into f; last: the level is max_depth (or the node is the lone one).  True: the node is replaced by
// its two children.
MTGX_HD bool fold_node(Fold& f, double m, const Node& nd, bool last) {
  const bool fails = !(nd.c > 0.0), certified = nd.bound > 0.0;
  const bool terminal = fails || certified || last;
  combine(f, mtgf::order_key(nd.c), mtgf::order_key(m), fails ? mtgf::order_key(m) : kKeyNone,
          terminal ? mtgf::order_key(nd.bound) : kKeyNone, terminal && !fails && !certified);
  return !terminal;
}

// a segment's outputs from its complete fold
struct SegmentResult {
  double lower_bound, sampled, closest_time, first_failing_time;
  int result, nodes, depth;
};
MTGX_HD SegmentResult segment_result(const Fold& f, bool budget, int nodes, int depth) {
  SegmentResult r;
  const bool fails = f.failing_time != kKeyNone;
  r.result = fails ? MTG_FIELD_COLLIDES : budget ? MTG_FIELD_UNDECIDED_BUDGET : f.undecided ? MTG_FIELD_UNDECIDED_DEPTH : MTG_FIELD_FREE;
  r.lower_bound = budget ? -INFINITY : mtgf::order_value(f.bound_key);
  r.sampled = mtgf::order_value(f.c_key);
  r.closest_time = mtgf::order_value(f.c_time);
  r.first_failing_time = fails ? mtgf::order_value(f.failing_time) : NAN;
  r.nodes = nodes;
  r.depth = depth;
  return r;
}

// The serial walk of one segment, level by level; cur, nxt: two buffers of kFrontier ints.
template <int NC>
inline SegmentResult walk_segment(const double (&p)[3][NC], double T, const mtgf::Grid& g, const Rule& P, int* cur, int* nxt) {
  const bool lone = lone_node(T);
  int count = lone ? 1 : 1 << P.min_depth, nodes = 0, depth = lone ? 0 : P.min_depth;
  for (int j = 0; j < count; ++j) cur[j] = j;
  Fold f;
  bool budget = false;
  for (;; ++depth) {
    const double w = half_width(T, depth);
    const bool last = lone || depth == P.max_depth;
    int survivors = 0;
    for (int i = 0; i < count; ++i) {
      const int j = cur[i];
      const double m = midpoint(T, j, w);
      if (fold_node(f, m, evaluate_node<NC>(p, m, w, g, P), last)) {
        if (2 * survivors + 1 < kFrontier) { nxt[2 * survivors] = 2 * j; nxt[2 * survivors + 1] = 2 * j + 1; }
        ++survivors;
      }
    }
    nodes += count;
    if (survivors == 0) break;
    if (2 * survivors > P.max_frontier) { budget = true; break; }
    count = 2 * survivors;
    int* t = cur; cur = nxt; nxt = t;
  }
  return segment_result(f, budget, nodes, depth);
}

// The Lipschitz helper's cell rule: the largest absolute difference over the four x-, y- and z-edges of the cell whose lowest
// corner is v (sy, sz: the strides of y and z), then sqrt(gx^2 + gy^2 + gz^2).  A NaN difference wins its maximum.
inline double cell_gradient(const float* v, long long sy, long long sz) {
  double gm[3] = {0.0, 0.0, 0.0};
  const long long step[3] = {1, sy, sz};
  for (int a = 0; a < 3; ++a) {
    const long long s1 = step[(a + 1) % 3], s2 = step[(a + 2) % 3];
    for (int e = 0; e < 4; ++e) {
      const float* lo = v + (e & 1) * s1 + (e >> 1) * s2;
      const double d = fabs((double)lo[step[a]] - (double)lo[0]);
      if (d > gm[a] || d != d) gm[a] = d;
      if (gm[a] != gm[a]) break;
    }
  }
  return sqrt(gm[0] * gm[0] + gm[1] * gm[1] + gm[2] * gm[2]);
}

}  // namespace mtgc
