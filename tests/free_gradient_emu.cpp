// free_gradient_emu.cpp -- stand-alone program (its own main) around the host form of the gradient with respect to the free
// derivatives, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_free_gradient_arguments.py together with
// csrc/mtg_pullback_host.cpp.  For every N, D in {1, 3, 4} and every combination of the optional pointers it calls
// mtg_free_gradient_host on seeded inputs with guard words around both outputs and compares every written number, bit for bit,
// with a serial restatement of the rule of include/mtg_hip.h that is written segment by segment (scatter into a per-vertex
// array) instead of vertex by vertex.  Prints "<n> mismatches".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mtg_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma GCC optimize("fp-contract=off")
#endif

#define MTG_TABLE_QUAL static const
#include "../mav_trajectory_generation_amd/csrc/mtg_tables.inc"

namespace {

uint64_t g_state = 0x243F6A8885A308D3ull;
double uniform(double lo, double hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// The rule, restated: one segment and dimension at a time, both halves; gS / gE [h]
void segment_rule(int N, int d, double T, const double* G_in, const double* c, double w, double* gS, double* gE) {
  const int h = N / 2;
  double tp[13], tn[13], G[12];
  tp[0] = 1.0;
  for (int m = 1; m <= N; ++m) tp[m] = tp[m - 1] * T;
  const double ti = 1.0 / T;
  tn[1] = ti;
  for (int m = 2; m <= N; ++m) tn[m] = tn[m - 1] * ti;
  for (int i = 0; i < N; ++i) G[i] = G_in ? G_in[i] : 0.0;
  if (c) {
    const double* Q1 = kQ1 + kH1Off[h][d];
    for (int i = d; i < N; ++i) {
      double S = 0.0;
      for (int j = d; j < N; ++j) S = std::fma(Q1[i * N + j], c[j] * tp[j - d], S);
      G[i] = std::fma(w, tp[i - d + 1] * S, G[i]);
    }
  }
  const double* ai = kAinvLo + kAinvLoOff[h];
  double rf = 1.0, fact = 1.0;
  for (int p = 0; p < h; ++p) {
    if (p > 0) fact *= p;
    rf = 1.0 / fact;
    double zS = 0.0, zE = 0.0;
    for (int j = 0; j < h; ++j) {
      const double u = tn[h + j] * G[h + j];
      zS = std::fma(ai[j * N + p], u, zS);
      zE = std::fma(ai[j * N + h + p], u, zE);
    }
    gS[p] = std::fma(tp[p], zS, G[p] * rf);
    gE[p] = tp[p] * zE;
  }
}

int run_case(int N, int D, int K, int d, int64_t B, const std::vector<uint32_t>& mask, bool with_grad, bool with_coeffs, bool want_free,
             bool want_fixed, bool soa) {
  const int h = N / 2, guard = 4;
  int n_fixed = 0;
  for (int v = 0; v <= K; ++v) n_fixed += __builtin_popcount(mask[v] & ((1u << h) - 1));
  const int n_free = h * (K + 1) - n_fixed;
  std::vector<double> times(B * K), grad(B * K * D * N), coeffs(B * K * D * N);
  for (auto& t : times) t = uniform(0.3, 4.0);
  for (auto& x : grad) x = uniform(-2.0, 2.0);
  for (auto& x : coeffs) x = uniform(-2.0, 2.0);
  mtg_layout L;
  if (!soa) {
    L.times_stride_b = K; L.times_stride_k = 1;
    L.fixed_stride_b = (int64_t)D * n_fixed; L.fixed_stride_d = n_fixed; L.fixed_stride_c = 1;
    L.free_stride_b = (int64_t)D * n_free; L.free_stride_d = n_free; L.free_stride_c = 1;
  } else {
    L.times_stride_b = 1; L.times_stride_k = B;
    L.fixed_stride_b = 1; L.fixed_stride_d = (int64_t)n_fixed * B; L.fixed_stride_c = B;
    L.free_stride_b = 1; L.free_stride_d = (int64_t)n_free * B; L.free_stride_c = B;
  }
  const double kGuard = -12345.678;
  std::vector<double> out_free(guard + B * D * n_free + guard, kGuard), out_fixed(guard + B * D * n_fixed + guard, kGuard);
  const double w = 0.625;
  const mtg_plan_desc desc = {N, D, K, d, mask.data()};
  const int rc = mtg_free_gradient_host(&desc, B, &L, times.data(), with_grad ? grad.data() : nullptr, with_coeffs ? coeffs.data() : nullptr,
                                        w, want_free ? out_free.data() + guard : nullptr, want_fixed ? out_fixed.data() + guard : nullptr);
  if (rc != MTG_OK) return 1000;
  int bad = 0;
  std::vector<char> seen_free(out_free.size(), 0), seen_fixed(out_fixed.size(), 0);
  for (int64_t b = 0; b < B; ++b)
    for (int dim = 0; dim < D; ++dim) {
      std::vector<double> gS(K * h), gE(K * h);
      for (int k = 0; k < K; ++k) {
        const int64_t row = ((b * K + k) * D + dim) * N;
        segment_rule(N, d, times[b * L.times_stride_b + k * L.times_stride_k], with_grad ? &grad[row] : nullptr,
                     with_coeffs ? &coeffs[row] : nullptr, w, &gS[k * h], &gE[k * h]);
      }
      int cf = 0, cp = 0;
      for (int v = 0; v <= K; ++v)
        for (int p = 0; p < h; ++p) {
          const double want = v == 0 ? gS[p] : (v == K ? gE[(K - 1) * h + p] : gE[(v - 1) * h + p] + gS[v * h + p]);
          if ((mask[v] >> p) & 1) {
            const int64_t at = guard + b * L.fixed_stride_b + dim * L.fixed_stride_d + cf++ * L.fixed_stride_c;
            seen_fixed[at] = 1;
            if (want_fixed && !same_bits(out_fixed[at], want)) ++bad;
          } else {
            const int64_t at = guard + b * L.free_stride_b + dim * L.free_stride_d + cp++ * L.free_stride_c;
            seen_free[at] = 1;
            if (want_free && !same_bits(out_free[at], want)) ++bad;
          }
        }
    }
  // everything the rule does not name, and everything of an output that was not asked for, still holds the guard value
  for (size_t i = 0; i < out_free.size(); ++i)
    if ((!want_free || !seen_free[i]) && !same_bits(out_free[i], kGuard)) ++bad;
  for (size_t i = 0; i < out_fixed.size(); ++i)
    if ((!want_fixed || !seen_fixed[i]) && !same_bits(out_fixed[i], kGuard)) ++bad;
  return bad;
}

}  // namespace

int main() {
  int mismatches = 0, cases = 0;
  for (int N = 2; N <= 12; N += 2) {
    const int h = N / 2;
    const uint32_t full = (1u << h) - 1;
    for (int D : {1, 3, 4})
      for (int K : {1, 3}) {
        std::vector<std::vector<uint32_t>> plans;
        std::vector<uint32_t> standard(K + 1, 1u);
        standard[0] = standard[K] = full;
        plans.push_back(standard);
        plans.push_back(std::vector<uint32_t>(K + 1, 0u));
        plans.push_back(std::vector<uint32_t>(K + 1, full));
        std::vector<uint32_t> mixed(K + 1);
        for (int v = 0; v <= K; ++v) mixed[v] = (0x2Du >> v) & full;
        plans.push_back(mixed);
        for (const auto& mask : plans)
          for (int inputs = 1; inputs <= 3; ++inputs)
            for (int outputs = 1; outputs <= 3; ++outputs) {
              const int d = (N + D + K + inputs) % h;
              mismatches += run_case(N, D, K, d, 3, mask, inputs & 1, inputs & 2, outputs & 1, outputs & 2, (cases & 1) != 0);
              ++cases;
            }
      }
  }
  // the argument rules that need no buffers
  const uint32_t m2[2] = {1, 1};
  const mtg_plan_desc ok = {2, 1, 1, 0, m2};
  mtg_layout L = {1, 1, 1, 1, 1, 1, 1, 1};
  double x[4] = {1, 2, 3, 4}, t[1] = {1.0}, o[2];
  if (mtg_free_gradient_host(&ok, 1, &L, t, nullptr, nullptr, 1.0, o, o) != MTG_ERR_INVALID_ARGUMENT) ++mismatches;
  if (mtg_free_gradient_host(&ok, 1, &L, t, x, nullptr, 1.0, nullptr, nullptr) != MTG_ERR_INVALID_ARGUMENT) ++mismatches;
  if (mtg_free_gradient_host(nullptr, 1, &L, t, x, nullptr, 1.0, o, o) != MTG_ERR_INVALID_ARGUMENT) ++mismatches;
  std::printf("%d cases, %d mismatches\n", cases, mismatches);
  return mismatches == 0 ? 0 : 1;
}
