// mtg_keepout_lane.h -- per-lane algorithm of the batched keep-out zone check: convex obstacles (boxes, prisms) given as the
// intersection of half spaces.
//
// A zone is P planes of four doubles (nx, ny, nz, offset) in the convention of the half-plane check (mtg_halfplane_lane.h):
// unit normal pointing INTO the zone, offset = point . normal; the zone is the set where every n_j . x - offset_j > 0, so the
// six planes of mtg_half_planes_bounding_box are a box zone as they stand.  Where the half-plane check asks whether a segment is
// inside for ALL t, this one asks whether it is inside at ANY t.  For a segment at local time t, over dimensions 0-2 (a 4th,
// yaw, dimension is never read):
//   h_j(t)    = offset_j - n_j . p(t)                  (> 0: outside plane j)
//   c(t)      = max_j h_j(t) - inflation
//   clearance = min over t in [0, T] of c(t)
// and a zone fails the segment iff !(clearance > 0): a safety check like the sphere check, a NaN fails and wins every minimum
// it enters.  What the number means:
//   * clearance > 0: outside.  It is a LOWER bound of the Euclidean distance to the zone whose planes are pushed out by
//     `inflation`: exact where the nearest point of the zone lies in a face, up to sqrt(3) low at a box corner (the distance to
//     the corner is the norm of the positive h_j, the clearance their maximum);
//   * clearance < 0: minus the exact penetration depth, i.e. the distance to the nearest (pushed-out) face;
//   * pushing the planes out by `inflation` is a superset of the Minkowski sum of the zone with a ball of that radius (the sum
//     has rounded edges and corners), so a vehicle of that radius that passes is clear.
//
// Candidates.  c(t) is the upper envelope of P polynomials; on [0, T] its minimum is attained at t = 0 or t = T, at an interior
// stationary point of the active h_j (a root of h_j', degree N - 2) or where the active polynomial changes (a root of
// h_i - h_j, i < j, degree N - 1).  Every search is "project p onto a vector -- n_j, or n_j - n_i -- and find the real roots in
// tau = t / T with real_roots_unit of mtg_extrema_lane.h, unchanged"; h_j' runs in the same instantiation as the differences
// with a zero leading coefficient (a zero leading level falls through), so a kernel holds ONE body of the root search.  Every
// candidate is evaluated as max_j h_j(t) from one evaluation of p(t): a surplus candidate is a value of the same function and
// cannot lower the minimum, so nothing records which plane is active where.  As in the half-plane lane, normals are compared
// by VALUE (+0 equals -0): a plane whose normal equals an earlier plane's or its negation shares that plane's stationary
// points and is not searched again, a pair with equal normals has a constant difference and is not searched.  A box costs
// at most 3 + 15 searches; a zone padded to P planes by repeating one gives bit-identical results (the repeats add only
// candidates that are there already).  A plane that is nowhere the maximum over the segment's quarter boxes (active_planes())
// is neither searched nor paired: of a box beside the segment the far faces drop out.
//
// Pruning and order are the sphere check's (mtg_obstacle_lane.h, whose Segment, four Bernstein-hull quarter boxes, Fold and
// first-failure word are used as they are).  lower_bound(): over a box with corners lo, hi every point has
// n_j . x <= sum_d max(n_jd lo_d, n_jd hi_d), so
//   min over the quarters of  max_j (offset_j - sum_d max(n_jd lo_d, n_jd hi_d))  - inflation
// bounds c(t) from below; it is reduced, per plane, by kBoxUlps ulps of sum_d |n_jd| E_d (E_d = sum_i |p_d[i] T^i|: the basis
// change, the two splits and the Horner chain as in the sphere check, plus the three products and sums of the projection, here
// and in the evaluation) and by kNormUlps ulps of |offset_j| and of the result and the inflation (the subtractions), so that it
// bounds every clearance the evaluation can COMPUTE.  A lane walks ITS OWN zones in ascending (bound,
// index) order, the next one selected by a scan of the whole list and never stored, and stops at the first zone whose bound is
// > 0 and strictly above the running minimum.  No result depends on the pruning or on list order:
//   * the failing zone reported is the smallest index among the failing ones;
//   * the nearest zone is the smallest index among those that attain the minimum; a NaN clearance wins the minimum, and the
//     smallest index among the zones that produced one is reported;
//   * within one zone the candidates are taken in the order 0, T, then the roots in search order ((0,0), (0,1), .., (0,P-1),
//     (1,1), ..; (j,j) is h_j', (i,j) is h_i - h_j), strict <, first NaN wins.
// N = 1 .. 12 run in the next even instantiation (at least 4) on zero-padded coefficients; T <= 0 has no interior candidates,
// both ends are still evaluated.
// Same code runs on the device (mtg_keepout.hip) and on the host (mtg_keepout_host.cpp).
#pragma once

#include "mtg_obstacle_lane.h"

namespace mtgk {

constexpr int kMinInstance = 4;
constexpr int kMaxZones = mtgo::kMaxObstacles;   // 4096: the first-failure word is segment << 12 | zone
constexpr int kMaxPlanes = 8;
constexpr int kMaxSegments = mtgo::kMaxSegments;
using mtgo::kBoxUlps;    // per plane, in ulps of sum_d |n_d| E_d
using mtgo::kNormUlps;
using mtgo::Fold;
using mtgo::Segment;

// what both entry points accept (include/mtg_hip.h)
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k, int n_zones,
                         int n_planes, long long zs_b, double inflation) {
  return mtgs::shape_ok(n_coeffs, 1, n_segments, dimension, 4, batch, ts_b, ts_k) && dimension >= 3 && n_segments < kMaxSegments &&
         n_zones >= 1 && n_zones <= kMaxZones && n_planes >= 1 && n_planes <= kMaxPlanes && zs_b >= 0 && inflation >= 0.0 &&
         inflation <= DBL_MAX;
}

constexpr int roots_len(int nc) { return 2 * (nc - 1); }   // the two buffers of real_roots_unit<nc>: the lane's whole buffer

template <int NC>
MTGX_HD void segment_prepare(const double* c, int N, int D, double T, Segment<NC>& S) {
  double p[3][NC], tpow[NC];
  mtgs::load_padded(c, N, D, p);
  tpow[0] = 1.0;
#pragma unroll
  for (int i = 1; i < NC; ++i) tpow[i] = tpow[i - 1] * T;
  mtgo::segment_boxes<NC>(c, N, D, T, p, tpow, S);
}

// a lower bound on every clearance the evaluation computes for the zone z (P planes) over the segment (header comment); NaN if
// anything that enters it is
template <int NC>
MTGX_HD double lower_bound(const Segment<NC>& S, const double* z, int P, double inflation) {
  double low[mtgo::kBoxes];   // per quarter: max_j of plane j's bound
#pragma unroll
  for (int q = 0; q < mtgo::kBoxes; ++q) low[q] = -INFINITY;
  bool nan = false;
  for (int j = 0; j < P; ++j) {
    const double n[3] = {z[4 * j], z[4 * j + 1], z[4 * j + 2]}, off = z[4 * j + 3];
    const double allowance = DBL_EPSILON * fma(kBoxUlps, fma(fabs(n[2]), S.e[2], fma(fabs(n[1]), S.e[1], fabs(n[0]) * S.e[0])),
                                               kNormUlps * fabs(off));
    nan = nan || off != off || allowance != allowance;
#pragma unroll
    for (int q = 0; q < mtgo::kBoxes; ++q) {
      double reach = 0.0;   // the largest n . x over the box
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double a = n[d] * S.lo[q][d], b = n[d] * S.hi[q][d];   // (0 x infinity: NaN)
        nan = nan || a != a || b != b;
        reach += a > b ? a : b;
      }
      const double h = off - reach - allowance;
      low[q] = h > low[q] ? h : low[q];
    }
  }
  double acc = low[0];
#pragma unroll
  for (int q = 1; q < mtgo::kBoxes; ++q) acc = low[q] < acc ? low[q] : acc;
  if (nan) acc = NAN;
  return acc - inflation - kNormUlps * DBL_EPSILON * (fabs(acc) + inflation);
}

// The planes that can be the maximum somewhere on the segment, as a bit mask: plane j is left out if, on every quarter box, the
// most it reaches (offset_j - the smallest n_j . x over the box, plus its allowance) is below what some plane never falls under
// there (lower_bound()'s per-plane term).  Such a plane is nowhere the active one, so its stationary points and its crossings
// are no candidates of the envelope's minimum; it still enters every evaluation.  A function of the segment and the zone alone.
// A NaN compares false and leaves the plane in.
template <int NC>
MTGX_HD unsigned active_planes(const Segment<NC>& S, const double* z, int P) {
  double floor[mtgo::kBoxes];
#pragma unroll
  for (int q = 0; q < mtgo::kBoxes; ++q) floor[q] = -INFINITY;
  unsigned active = 0u;
  for (int pass = 0; pass < 2; ++pass)
    for (int j = 0; j < P; ++j) {
      const double n[3] = {z[4 * j], z[4 * j + 1], z[4 * j + 2]}, off = z[4 * j + 3];
      const double allowance = DBL_EPSILON * fma(kBoxUlps, fma(fabs(n[2]), S.e[2], fma(fabs(n[1]), S.e[1], fabs(n[0]) * S.e[0])),
                                                 kNormUlps * fabs(off));
#pragma unroll
      for (int q = 0; q < mtgo::kBoxes; ++q) {
        double most = 0.0, least = 0.0;   // the largest and the smallest n . x over the box
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const double a = n[d] * S.lo[q][d], b = n[d] * S.hi[q][d];
          most += a > b ? a : b;
          least += a > b ? b : a;
        }
        const double low = off - most - allowance, top = off - least + allowance;
        if (pass == 0) floor[q] = low > floor[q] ? low : floor[q];
        else if (!(top < floor[q])) active |= 1u << j;
      }
    }
  return active;
}

// c(t) = max_j h_j(t) - inflation from one evaluation of p(t); NaN if any h_j is
template <int NC>
MTGX_HD double envelope_at(const double (&p)[3][NC], const double* z, int P, double inflation, double t) {
  const double x0 = mtgx::horner<NC - 1>(p[0], t), x1 = mtgx::horner<NC - 1>(p[1], t), x2 = mtgx::horner<NC - 1>(p[2], t);
  double top = -INFINITY;
  bool nan = false;
  for (int j = 0; j < P; ++j) {
    const double h = z[4 * j + 3] - fma(z[4 * j + 2], x2, fma(z[4 * j + 1], x1, z[4 * j] * x0));
    nan = nan || h != h;
    top = h > top ? h : top;
  }
  return nan ? NAN : top - inflation;
}

// running minimum over one zone's candidates: strict <, first NaN wins
struct Candidates {
  double best, best_t;
  bool nan, bad;
};
MTGX_HD void candidate(Candidates& k, double v, double t) {
  k.bad = k.bad || !(v > 0.0);
  if (!k.nan && (v != v || v < k.best)) { k.best = v; k.best_t = t; k.nan = v != v; }
}

// One segment against one zone: the searches and the evaluation.  Never pruned.
template <int NC, class Roots>
MTGX_HD void zone_clearance(const Segment<NC>& S, const double* z, int P, double inflation, Roots& roots, double& v_min, double& t_min,
                            bool& fails) {
  Candidates k{INFINITY, 0.0, false, false};
  {
    double p[3][NC];
    mtgs::load_padded(mtgo::read_again(S.c), S.N, S.D, p);
    candidate(k, envelope_at<NC>(p, z, P, inflation, 0.0), 0.0);
    candidate(k, envelope_at<NC>(p, z, P, inflation, S.T), S.T);
  }
  if (S.T > 0.0) {
    const unsigned active = active_planes<NC>(S, z, P);
    for (int i = 0; i < P; ++i) {
      if (!((active >> i) & 1u)) continue;
      const double ix = z[4 * i], iy = z[4 * i + 1], iz = z[4 * i + 2], ioff = z[4 * i + 3];
      for (int j = i; j < P; ++j) {
        const double jx = z[4 * j], jy = z[4 * j + 1], jz = z[4 * j + 2], joff = z[4 * j + 3];
        const bool own = i == j;   // h_j' (own) or h_i - h_j
        bool skip = !((active >> j) & 1u) || (!own && ix == jx && iy == jy && iz == jz);   // (equal normals: a constant difference)
        if (own)
          for (int e = 0; e < j; ++e) {   // an earlier SEARCHED plane with this normal or its negation: its stationary points
            const double ex = z[4 * e], ey = z[4 * e + 1], ez = z[4 * e + 2];
            skip = skip || (((active >> e) & 1u) && ((ex == jx && ey == jy && ez == jz) || (ex == -jx && ey == -jy && ez == -jz)));
          }
        if (skip) continue;
        // the projection onto v, in tau: own -> d/dtau (v . u), else (offset_i - offset_j) + v . u, u[m] = p[m] T^m
        // v is oriented so that its first non-zero component is positive: (i, j) and (j, i) then search the SAME polynomial, bit
        // for bit (the search of g and of -g may differ in the last place of a bisection step), which is what makes a repeated
        // plane add nothing whichever plane it repeats
        double vx = own ? jx : jx - ix, vy = own ? jy : jy - iy, vz = own ? jz : jz - iz, v0 = own ? 0.0 : ioff - joff;
        if (vx < 0.0 || (vx == 0.0 && (vy < 0.0 || (vy == 0.0 && vz < 0.0)))) { vx = -vx; vy = -vy; vz = -vz; v0 = -v0; }
        int cnt, base = 0;
        {
          const double* c = mtgo::read_again(S.c);
          double w[NC], g[NC];
          double tp = 1.0;
#pragma unroll
          for (int m = 0; m < NC; ++m) {
            const bool in = m < S.N;
            const double p0 = in ? c[m] : 0.0, p1 = in ? c[S.N + m] : 0.0, p2 = in ? c[2 * S.N + m] : 0.0;
            w[m] = fma(vz, p2, fma(vy, p1, vx * p0)) * tp;
            tp *= S.T;
          }
#pragma unroll
          for (int m = 0; m < NC; ++m) g[m] = own ? (m + 1 < NC ? (double)(m + 1) * w[m + 1] : 0.0) : (m == 0 ? w[0] + v0 : w[m]);
          cnt = mtgx::real_roots_unit<NC, Roots>(g, roots, base);
        }
        double p[3][NC];
        mtgs::load_padded(mtgo::read_again(S.c), S.N, S.D, p);
        for (int r = 0; r < cnt; ++r) {
          // (a Newton step towards a root AT 0 or 1 can leave [0, 1] by a rounding error: the end itself is a candidate already)
          const double t = fmin(fmax(roots[base + r], 0.0), 1.0) * S.T;
          candidate(k, envelope_at<NC>(p, z, P, inflation, t), t);
        }
      }
    }
  }
  v_min = k.best;
  t_min = k.best_t;
  fails = k.bad;
}

// One segment against its zone set (M zones x P planes x (nx, ny, nz, offset)); roots: roots_len(NC) elements.
// searches: if not null, the number of zones this lane searched (of M without pruning).
template <int NC, class Roots>
MTGX_HD void segment_check(const double* c, int N, int D, double T, const double* zones, int M, int P, double inflation, Roots& roots,
                           Fold& out, int* searches = nullptr) {
  Segment<NC> S;
  segment_prepare<NC>(c, N, D, T, S);
  mtgo::fold_init(out);
  double last_key = -INFINITY;
  int last_h = -1, n = 0;
  for (;;) {
    // the next zone in ascending (key, index) order after (last_key, last_h); key = bound, NaN as -infinity
    double key = INFINITY;
    int h = -1;
    for (int m = 0; m < M; ++m) {
      double b = lower_bound<NC>(S, zones + (long long)m * (4 * P), P, inflation);
      b = b != b ? -INFINITY : b;
      const bool after = b > last_key || (b == last_key && m > last_h);
      const bool first = h < 0 || b < key;   // (ascending m: an equal key keeps the smaller index)
      if (after && first) { key = b; h = m; }
    }
    if (h < 0) break;                                   // every zone has been searched
    if (key > 0.0 && key > out.clearance) break;        // this one and every later one can neither fail nor lower the minimum
    double v, t;
    bool fails;
    zone_clearance<NC, Roots>(S, zones + (long long)h * (4 * P), P, inflation, roots, v, t, fails);
    mtgo::fold_obstacle(out, h, v, t, fails);
    last_key = key;
    last_h = h;
    ++n;
  }
  if (searches) *searches = n;
}

}  // namespace mtgk
