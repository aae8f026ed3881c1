// mtg_pullback_lane.h -- lane code of the batched gradient with respect to the free derivatives (mtg_free_gradient,
// include/mtg_hip.h): the exact TRANSPOSE of the map mtg_update_segments_from_free applies (mtg_recover in mtg_lane.h),
//   c_p = x_S,p / p!  (p < h),   c_(h+j) = T^-(h+j) sum_k ai[j][k] dl_k,   dl = [T^p x_S,p ; T^p x_E,p],
// applied to a coefficient-space gradient G [B][K][D][N], optionally with the derivative cost's gradient w Q(T) c added on the
// fly.  One lane owns one (trajectory, vertex, dimension): it forms the END half of segment v - 1 and the START half of segment
// v, adds them and writes its h numbers to the free or the fixed column of (v, p).  Host + device, plain C++17; the kernel is
// mtg_pullback.hip, the serial loop over the same function mtg_pullback_host.cpp.
//
// Every rounding is fixed so that a host loop reproduces each bit (the specification is the comment block in mtg_hip.h); fl()
// is one float64 rounding, every fma a fused multiply-add, nothing else is fused, nothing depends on the launch geometry:
//   powers     tp_0 = 1, tp_m = fl(tp_(m-1) T);  ti = fl(1 / T), tn_1 = ti, tn_m = fl(tn_(m-1) ti)        (repeated multiplication)
//   input      G_i = grad_coeffs entry i of the segment's row, +0 without grad_coeffs.  With coeffs, for i >= d:
//              y_j = fl(c_j tp_(j-d)) (j >= d),  S_i = sum over j = d .. N-1 ascending, one fma(Q1[i][j], y_j, S) per term from +0,
//              q_i = fl(tp_(i-d+1) S_i)  [= (Q(T) c)_i: T^(1-2d) T^i T^j = T T^(i-d) T^(j-d)],  G_i = fma(w, q_i, G_i);
//              rows i < d of Q are zero: G_i stays as it is (also for a non-finite w)
//   u          u_j = fl(tn_(h+j) G_(h+j)),  j < h
//   z          z_k = sum over j = 0 .. h-1 ascending, one fma(ai[j][k], u_j, z) per term from +0
//   halves     g_S,p = fma(tp_p, z_p, fl(G_p rf_p)) with rf_p = fl(1 / p!);   g_E,p = fl(tp_p z_(h+p))
//   vertex     0 < v < K: fl(g_E,p of segment v - 1  +  g_S,p of segment v), the left segment's end first, one rounded addition;
//              v = 0: g_S,p of segment 0;  v = K: g_E,p of segment K - 1 (no addition)
//   routing    fixed_mask[v] bit p set: grad_fixed column offF[v] + popcount(mask below p); else grad_free column
//              offP[v] + (p - popcount(mask below p)).  Every output element is written exactly once, by the lane that owns it.
// Times are not validated: T <= 0 or NaN gives what this arithmetic gives.  Contraction is OFF for this header.
#pragma once

#include <stdint.h>

#include "mtg_segment_lane.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#if defined(__HIPCC__)
#define MTGP_HD __device__ inline __attribute__((always_inline))
#ifndef MTG_TABLE_QUAL
#define MTG_TABLE_QUAL __constant__ const
#endif
#else
#define MTGP_HD inline
#ifndef MTG_TABLE_QUAL
#define MTG_TABLE_QUAL static const
#endif
#endif

namespace mtgp {

#include "mtg_tables.inc"

constexpr int kMinInstance = 2;

constexpr int ainv_offset(int n) {   // kAinvLoOff[n / 2]
  int off = 0;
  for (int m = 2; m < n; m += 2) off += (m / 2) * m;
  return off;
}
constexpr int q1_offset(int n, int d) {   // kH1Off[n / 2][d]: Q(1) shares H(1)'s layout
  int off = 0;
  for (int m = 2; m < n; m += 2) off += (m / 2) * m * m;
  return off + d * n * n;
}

struct Params {
  const double* times;  long long ts_b, ts_k;
  const double* grad;      // [B][K][D][N] or null (+0)
  const double* coeffs;    // [B][K][D][N] or null (no derivative-cost term)
  double w;                // smoothness weight
  double* gfree;        long long ps_b, ps_d, ps_c;   // or null
  double* gfixed;       long long fs_b, fs_d, fs_c;   // or null
  const int* mask;         // [K + 1]
  const int* offF;         // [K + 2] prefix of the fixed slots
  const int* offP;         // [K + 2] prefix of the free slots
  long long B;
  int K, D, deriv, q1off;
};

// What both entry points check besides their plan or plan description
inline bool arguments_ok(long long batch, const void* layout, const void* times, const void* grad, const void* coeffs,
                         const void* gfree, const void* gfixed) {
  return batch >= 0 && layout && times && (grad || coeffs) && (gfree || gfixed);
}

MTGP_HD double fma_(double a, double b, double c) {
#if defined(__HIPCC__)
  return __builtin_fma(a, b, c);
#else
  return std::fma(a, b, c);
#endif
}

// One half of one segment's pull-back for one dimension: END = false: g_S (start vertex), END = true: g_E (end vertex).
// row: element offset of the segment's [N] row in grad / coeffs.
template <int N, bool END>
MTGP_HD void segment_half(const Params& P, long long row, double T, double (&g)[N / 2]) {
  constexpr int H = N / 2;
  constexpr int LO = END ? H : 0;   // the end half reads only the high half of G
  double tp[N];
  tp[0] = 1.0;
#pragma unroll
  for (int m = 1; m < N; ++m) tp[m] = tp[m - 1] * T;
  double G[N];
#pragma unroll
  for (int i = 0; i < N; ++i) G[i] = (P.grad && i >= LO) ? P.grad[row + i] : 0.0;
  if (P.coeffs) {
    const int d = P.deriv;
    const double* q1 = kQ1 + P.q1off;
    double y[N];
    {
      double pw = 1.0;   // tp_(j-d)
#pragma unroll
      for (int j = 0; j < N; ++j) {
        y[j] = 0.0;
        if (j >= d) { y[j] = P.coeffs[row + j] * pw; pw = pw * T; }
      }
    }
    double rs = T;       // tp_(i-d+1)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= d) {
        if (i >= LO) {
          double S = 0.0;
#pragma unroll
          for (int j = 0; j < N; ++j)
            if (j >= d) S = fma_(q1[i * N + j], y[j], S);
          G[i] = fma_(P.w, rs * S, G[i]);
        }
        rs = rs * T;
      }
    }
  }
  const double ti = 1.0 / T;
  double tn = ti;        // tn_m
#pragma unroll
  for (int m = 2; m <= H; ++m) tn = tn * ti;
  double u[H];
#pragma unroll
  for (int j = 0; j < H; ++j) {
    u[j] = tn * G[H + j];
    tn = tn * ti;
  }
  const double* ai = kAinvLo + ainv_offset(N);   // [H][N]
#pragma unroll
  for (int p = 0; p < H; ++p) {
    const int k = END ? H + p : p;
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < H; ++j) z = fma_(ai[j * N + k], u[j], z);
    if constexpr (END) {
      g[p] = tp[p] * z;
    } else {
      double f = 1.0;
#pragma unroll
      for (int q = 2; q <= p; ++q) f *= (double)q;   // p! (exact: p <= 5)
      const double rf = 1.0 / f;                     // compile-time constant after unrolling
      g[p] = fma_(tp[p], z, G[p] * rf);
    }
  }
}

// The lane of (trajectory b, vertex v, dimension dim)
template <int N>
MTGP_HD void vertex_lane(const Params& P, long long b, int v, int dim) {
  constexpr int H = N / 2;
  double g[H];
#pragma unroll
  for (int p = 0; p < H; ++p) g[p] = 0.0;
  if (v > 0) {
    const double T = P.times[b * P.ts_b + (long long)(v - 1) * P.ts_k];
    segment_half<N, true>(P, ((b * P.K + (v - 1)) * P.D + dim) * (long long)N, T, g);
  }
  if (v < P.K) {
    const double T = P.times[b * P.ts_b + (long long)v * P.ts_k];
    double gs[H];
    segment_half<N, false>(P, ((b * P.K + v) * P.D + dim) * (long long)N, T, gs);
#pragma unroll
    for (int p = 0; p < H; ++p) g[p] = v > 0 ? g[p] + gs[p] : gs[p];
  }
  const int mask = P.mask[v], of = P.offF[v], op = P.offP[v];
#pragma unroll
  for (int p = 0; p < H; ++p) {
    const int below = __builtin_popcount((unsigned)(mask & ((1 << p) - 1)));
    if ((mask >> p) & 1) {
      if (P.gfixed) P.gfixed[b * P.fs_b + dim * P.fs_d + (long long)(of + below) * P.fs_c] = g[p];
    } else {
      if (P.gfree) P.gfree[b * P.ps_b + dim * P.ps_d + (long long)(op + p - below) * P.ps_c] = g[p];
    }
  }
}

}  // namespace mtgp
