// mtg_field_lane.h -- lane code of the batched distance-field clearance check (mtg_check_distance_field, include/mtg_hip.h): a
// solved segment is SAMPLED at local times 0, fl(i dt) < T, T and every sample's position is looked up in a voxel grid of
// float distances (an ESDF, an inflated occupancy map).  Here: the sample rule, the lookup, and the fold over a segment's
// samples.  Host + device, plain C++17; the kernel is mtg_field.hip, the serial loop over the same functions mtg_field_host.cpp.
//
// Every rule is fixed so that a host loop reproduces each choice (the specification is the comment block in mtg_hip.h):
//   samples    t_0 = 0, t_i = fl(i dt) for i >= 1 with fl(i dt) < T, then T itself; S of them (>= 2); T <= 0 or NaN: 0 and T
//   position   Horner with one fma per coefficient, dimensions 0-2
//   u_a        fl(fl(p_a - origin_a) r),  r = fl(1 / voxel_size) formed once by the entry
//   trilinear  inside iff 0 <= u_a <= n_a - 1; i_a = min((int)floor(u_a), n_a - 2), f_a = fl(u_a - i_a); the eight floats as
//              doubles, combined along x, then y, then z, each step fma(f, hi - lo, lo)
//   nearest    i_a = floor(fl(u_a + 0.5)), inside iff 0 <= i_a <= n_a - 1
//   outside    outside_distance; a NaN u_a on any axis: NaN
//   clearance  fl(d - inflation); a sample fails iff !(clearance > 0)
// Nothing here may be fused by the compiler: u_a + 0.5 as fma(p_a - origin_a, r, 0.5) moves a sample across a voxel boundary,
// i dt - T < 0 changes S.  Contraction is therefore OFF for this header (the explicit fma calls stay fused multiply-adds).
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/mtg_hip.h"
#include "mtg_segment_lane.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace mtgf {

constexpr int kMinInstance = 4;
constexpr int kMaxSegments = 1 << 19;      // failure_word(segment, 0) stays a positive int
constexpr int kMaxSamplesLimit = 1 << 20;  // the largest max_samples
constexpr long long kMaxVoxels = 0x7fffffffll;
constexpr int kNoSample = 0x7fffffff;      // "no failing sample yet"

// what the kernel and the host loop read of an mtg_distance_field
struct Grid {
  const float* d;   // [nz][ny][nx]
  int nx, ny, nz;
  double o[3];      // centre of voxel (0, 0, 0)
  double r;         // fl(1 / voxel_size)
  double outside;
  int trilinear;
};

// what both entry points accept (include/mtg_hip.h); fills g
inline bool arguments_ok(int n_coeffs, int n_segments, int dimension, long long batch, long long ts_b, long long ts_k,
                         const mtg_distance_field* f, double dt, int max_samples, double inflation, Grid* g) {
  if (!mtgs::shape_ok(n_coeffs, 1, n_segments, dimension, 4, batch, ts_b, ts_k) || dimension < 3 || n_segments >= kMaxSegments)
    return false;
  if (!f || !f->distances) return false;
  if (f->interpolation != MTG_FIELD_NEAREST && f->interpolation != MTG_FIELD_TRILINEAR) return false;
  const int least = f->interpolation == MTG_FIELD_TRILINEAR ? 2 : 1;
  if (f->nx < least || f->ny < least || f->nz < least) return false;
  if ((long long)f->nx * f->ny > kMaxVoxels || (long long)f->nx * f->ny * f->nz > kMaxVoxels) return false;
  if (!(f->voxel_size > 0.0) || !(f->voxel_size <= DBL_MAX) || !(1.0 / f->voxel_size <= DBL_MAX)) return false;
  for (int a = 0; a < 3; ++a)
    if (!(std::fabs(f->origin[a]) <= DBL_MAX)) return false;
  if (f->outside_distance != f->outside_distance) return false;
  if (!(inflation >= 0.0) || !(inflation <= DBL_MAX)) return false;
  if (!(dt > 0.0) || !(dt <= DBL_MAX)) return false;
  if (max_samples < 2 || max_samples > kMaxSamplesLimit) return false;
  g->d = f->distances; g->nx = f->nx; g->ny = f->ny; g->nz = f->nz;
  for (int a = 0; a < 3; ++a) g->o[a] = f->origin[a];
  g->r = 1.0 / f->voxel_size; g->outside = f->outside_distance; g->trilinear = f->interpolation == MTG_FIELD_TRILINEAR;
  return true;
}

// S, or -1 if S > max_samples.  Not a walk: T / dt is compared with the cap as a double, then the integer guess is corrected by
// one either way with the sample rule's own test (fl(i dt) and fl(T / dt) carry one rounding each: with T / dt < 2^20 + 2 the
// guess is off by at most one).
MTGX_HD int sample_count(double T, double dt, int max_samples) {
  if (!(T > 0.0)) return 2;
  const double q = T / dt;
  if (!(q < (double)max_samples + 2.0)) return -1;   // (also q = +infinity)
  int m = (int)q;                                    // interior samples: the i >= 1 with fl(i dt) < T
  if (m >= 1 && !((double)m * dt < T)) --m;
  else if ((double)(m + 1) * dt < T) ++m;
  return m + 2 > max_samples ? -1 : m + 2;
}

// local time of sample i of S
MTGX_HD double sample_time(int i, int S, double T, double dt) { return i == S - 1 ? T : (double)i * dt; }

MTGX_HD void load2(const float* p, float (&v)[2]) { __builtin_memcpy(v, p, 2 * sizeof(float)); }   // the two x-neighbours at once

// voxel coordinates of position p (dimensions 0-2)
MTGX_HD void voxel_coordinates(const Grid& g, const double (&p)[3], double (&u)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) u[a] = (p[a] - g.o[a]) * g.r;
}

// the field's value at voxel coordinates u (the certified check, mtg_certify_lane.h, looks up clamped coordinates too)
MTGX_HD double lookup_voxel(const Grid& g, const double (&u)[3]) {
  if (u[0] != u[0] || u[1] != u[1] || u[2] != u[2]) return NAN;
  const int n[3] = {g.nx, g.ny, g.nz};
  if (g.trilinear) {
    int i[3];
    double f[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) inside = inside && u[a] >= 0.0 && u[a] <= (double)(n[a] - 1);
    if (!inside) return g.outside;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int fl = (int)floor(u[a]);
      i[a] = fl < n[a] - 2 ? fl : n[a] - 2;
      f[a] = u[a] - (double)i[a];
    }
    const float* base = g.d + ((long long)i[2] * g.ny + i[1]) * (long long)g.nx + i[0];
    const long long sy = g.nx, sz = (long long)g.nx * g.ny;
    float v00[2], v10[2], v01[2], v11[2];
    load2(base, v00);
    load2(base + sy, v10);
    load2(base + sz, v01);
    load2(base + sz + sy, v11);
    const double x00 = fma(f[0], (double)v00[1] - (double)v00[0], (double)v00[0]);
    const double x10 = fma(f[0], (double)v10[1] - (double)v10[0], (double)v10[0]);
    const double x01 = fma(f[0], (double)v01[1] - (double)v01[0], (double)v01[0]);
    const double x11 = fma(f[0], (double)v11[1] - (double)v11[0], (double)v11[0]);
    const double y0 = fma(f[1], x10 - x00, x00);
    const double y1 = fma(f[1], x11 - x01, x01);
    return fma(f[2], y1 - y0, y0);
  }
  double v[3];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v[a] = floor(u[a] + 0.5);
    inside = inside && v[a] >= 0.0 && v[a] <= (double)(n[a] - 1);   // (compared as doubles: u may be infinite)
  }
  if (!inside) return g.outside;
  return (double)g.d[((long long)(int)v[2] * g.ny + (int)v[1]) * (long long)g.nx + (int)v[0]];
}

// the field's value at position p (dimensions 0-2)
MTGX_HD double lookup(const Grid& g, const double (&p)[3]) {
  double u[3];
  voxel_coordinates(g, p, u);
  return lookup_voxel(g, u);
}

// order_key of mtg_segment_kernel.h for host and device: unsigned order = numeric order, NaN below every number
MTGX_HD unsigned long long order_key(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, sizeof u);
  if (x != x) return 0ull;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
MTGX_HD double order_value(unsigned long long k) {
  if (k == 0ull) return NAN;
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  __builtin_memcpy(&x, &u, sizeof x);
  return x;
}

// The fold over a set of samples: the minimum of (order_key(clearance), sample index), smaller key first, then smaller index --
// associative and commutative, so any split of a segment's samples over lanes gives the same result -- and the smallest
// failing index.
struct Fold {
  unsigned long long key = ~0ull;   // above every key of a double
  int sample = kNoSample;
  int failing = kNoSample;
};
MTGX_HD void combine(Fold& a, unsigned long long key, int sample, int failing) {
  if (key < a.key || (key == a.key && sample < a.sample)) { a.key = key; a.sample = sample; }
  if (failing < a.failing) a.failing = failing;
}

// samples first, first + step, .. < S of one segment into f; p: the segment's position polynomials, zero-padded to NC
template <int NC>
MTGX_HD void fold_samples(const double (&p)[3][NC], double T, double dt, int S, int first, int step, const Grid& g, double inflation,
                          Fold& f) {
  for (int i = first; i < S; i += step) {
    const double t = sample_time(i, S, T, dt);
    double x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double r = 0.0;
#pragma unroll
      for (int j = NC - 1; j >= 0; --j) r = fma(r, t, p[a][j]);
      x[a] = r;
    }
    const double c = lookup(g, x) - inflation;
    combine(f, order_key(c), i, c > 0.0 ? kNoSample : i);
  }
}

// a segment's outputs from its complete fold (S = -1: not sampled)
struct SegmentResult {
  double clearance;
  int closest, first_failing, samples;
  bool fails;
};
MTGX_HD SegmentResult segment_result(const Fold& f, int S) {
  SegmentResult r;
  if (S < 0) { r.clearance = NAN; r.closest = -1; r.first_failing = -1; r.samples = -1; r.fails = true; return r; }
  r.clearance = order_value(f.key);
  r.closest = f.sample;
  r.fails = f.failing != kNoSample;
  r.first_failing = r.fails ? f.failing : -1;
  r.samples = S;
  return r;
}

}  // namespace mtgf
