// mtg_collision_host.cpp -- host build (plain g++, no HIP) of the distance-field collision cost and gradient: the lane code of
// mtg_collision_lane.h run one segment after the other, with the device's 64 partial sums and its butterfly, so that both forms
// add in the same order.  For one-trajectory-at-a-time callers and as the reproducible form of every rule in include/mtg_hip.h.
// Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_collision_lane.h"

namespace {

template <int NC, bool GRAD>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const mtgf::Grid& g,
         const mtgc::Potential& q, double dt, int max_samples, double* seg_cost, double* traj_cost, double* grad, int32_t* seg_samples) {
  mtgc::Sums<NC, GRAD> P[mtgc::kPartials];   // (19 KB at NC = 12)
  for (int64_t b = 0; b < B; ++b) {
    double total = 0.0;
    for (int k = 0; k < K; ++k) {
      const int64_t idx = b * K + k;
      const double T = times[b * ts_b + k * ts_k];
      double p[3][NC];
      mtgs::load_padded<NC, 3>(coeffs + idx * (int64_t)(D * N), N, D, p);
      const int S = mtgf::sample_count(T, dt, max_samples);
      for (int l = 0; l < mtgc::kPartials; ++l) {
        mtgc::clear(P[l]);
        mtgc::sum_samples<NC, GRAD>(p, T, dt, S, l, mtgc::kPartials, g, q, P[l]);
      }
      for (int off = mtgc::kPartials / 2; off > 0; off >>= 1) {
        for (int l = 0; l < mtgc::kPartials; ++l)   // (IEEE addition commutes: both partners get the same sum)
          if (!(l & off)) { mtgc::add(P[l], P[l ^ off]); P[l ^ off] = P[l]; }
      }
      const double cost = S < 0 ? NAN : P[0].cost;
      seg_cost[idx] = cost;
      total = total + cost;
      if (seg_samples) seg_samples[idx] = S;
      if constexpr (GRAD) {
        double* out = grad + idx * (int64_t)(D * N);
        for (int a = 0; a < D; ++a)
          for (int j = 0; j < N; ++j) out[a * N + j] = a >= 3 ? 0.0 : (S < 0 ? NAN : P[0].grad[a][j]);
      }
    }
    if (traj_cost) traj_cost[b] = total;
  }
}

}  // namespace

extern "C" int mtg_collision_cost_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                       const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                       const mtg_distance_field* field, double dt, int32_t max_samples, double inflation, double epsilon,
                                       double speed_epsilon, double* segment_cost, double* trajectory_cost, double* coeff_gradient,
                                       int32_t* segment_samples) {
  if (!coeffs || !times || !segment_cost) return MTG_ERR_INVALID_ARGUMENT;
  mtgf::Grid g;
  mtgc::Potential q;
  if (!mtgc::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, dt, max_samples, inflation,
                          epsilon, speed_epsilon, &g, &q))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<mtgc::kMinInstance>(n_coeffs, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    if (coeff_gradient)
      run<NC, true>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, g, q, dt, max_samples,
                    segment_cost, trajectory_cost, coeff_gradient, segment_samples);
    else
      run<NC, false>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, g, q, dt, max_samples,
                     segment_cost, trajectory_cost, nullptr, segment_samples);
  });
  return MTG_OK;
}
