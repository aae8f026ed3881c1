// mtg_separation_host.cpp -- host build (plain g++, no HIP) of the trajectory-to-trajectory separation check: the lane code of
// mtg_separation_lane.h run one (pair, segment of A) after the other, folded in time order.  For the replanner that checks one
// candidate against a few committed plans.  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_separation_lane.h"

namespace {

struct HostSide {
  const double* coeffs;
  const double* times;
  const double* start;
  int64_t ts_b, ts_k, B;
  int K;
};

mtgp::Side side_of(const HostSide& S, int index, int N, int D) {
  return {S.coeffs + (int64_t)index * S.K * (int64_t)(D * N), S.times + (int64_t)index * S.ts_b, S.ts_k, S.K, S.start ? S.start[index] : 0.0};
}

template <int NC>
void run(int N, int D, const HostSide& a, const HostSide& b, int64_t P, const int32_t* pairs, double min_separation, int32_t* feasible,
         int32_t* first_a, int32_t* first_b, double* pair_separation, double* pair_time, int32_t* pair_a, int32_t* pair_b,
         double* seg_separation, double* seg_time, int32_t* seg_b, int32_t* seg_pieces) {
  double buf[mtgp::buffer_len(NC)];
  double* r = buf;
  for (int64_t p = 0; p < P; ++p) {
    const mtgp::Side A = side_of(a, pairs[2 * p], N, D), B = side_of(b, pairs[2 * p + 1], N, D);
    mtgp::Fold pair;
    mtgp::fold_init(pair);
    for (int i = 0; i < a.K; ++i) {   // (every segment is checked, as on the device: the separations are complete whatever fails first)
      const int64_t idx = p * a.K + i;
      mtgp::Fold f;
      mtgp::lane_check<NC, double*>(A, B, i, N, D, min_separation, true, r, f);
      if (seg_separation) seg_separation[idx] = f.separation;
      if (seg_time) seg_time[idx] = f.time;
      if (seg_b) seg_b[idx] = f.segment_b;
      if (seg_pieces) seg_pieces[idx] = f.pieces;
      if (f.invalid) {   // (every lane of the pair finds the same)
        mtgp::fold_invalid(pair);
        continue;
      }
      mtgp::fold_minimum(pair, i, f.segment_b, f.separation, f.time);
      if (f.failing_b >= 0 && pair.failing_b < 0) { pair.failing_a = f.failing_a; pair.failing_b = f.failing_b; }
    }
    feasible[p] = !pair.invalid && pair.failing_b < 0 ? 1 : 0;
    if (first_a) first_a[p] = pair.failing_a;
    if (first_b) first_b[p] = pair.failing_b;
    if (pair_separation) pair_separation[p] = pair.separation;
    if (pair_time) pair_time[p] = pair.time;
    if (pair_a) pair_a[p] = pair.segment_a;
    if (pair_b) pair_b[p] = pair.segment_b;
  }
}

}  // namespace

extern "C" int mtg_check_trajectory_separation_host(int32_t n_coeffs, int32_t dimension, int32_t n_segments_a, int64_t batch_a,
                                                    const double* coeffs_a, const double* times_a, int64_t times_a_stride_b,
                                                    int64_t times_a_stride_k, const double* start_a, int32_t n_segments_b,
                                                    int64_t batch_b, const double* coeffs_b, const double* times_b,
                                                    int64_t times_b_stride_b, int64_t times_b_stride_k, const double* start_b,
                                                    int64_t n_pairs, const int32_t* pairs, double min_separation, int32_t* pair_feasible,
                                                    int32_t* first_failing_segment_a, int32_t* first_failing_segment_b,
                                                    double* pair_separation, double* pair_closest_time, int32_t* pair_closest_segment_a,
                                                    int32_t* pair_closest_segment_b, double* segment_separation,
                                                    double* segment_closest_time, int32_t* segment_closest_segment_b,
                                                    int32_t* segment_pieces) {
  if (!coeffs_a || !times_a || !coeffs_b || !times_b || !pairs || !pair_feasible) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgp::arguments_ok(n_coeffs, dimension, n_segments_a, batch_a, times_a_stride_b, times_a_stride_k, n_segments_b, batch_b,
                          times_b_stride_b, times_b_stride_k, n_pairs, min_separation))
    return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgp::outputs_ok(pair_closest_time, pair_closest_segment_a, pair_closest_segment_b, segment_separation, segment_closest_time,
                        segment_closest_segment_b))
    return MTG_ERR_INVALID_ARGUMENT;
  // the host can read the pair list: every index must name a trajectory of its side
  for (int64_t p = 0; p < n_pairs; ++p)
    if (pairs[2 * p] < 0 || pairs[2 * p] >= batch_a || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= batch_b) return MTG_ERR_INVALID_ARGUMENT;
  const HostSide a{coeffs_a, times_a, start_a, times_a_stride_b, times_a_stride_k, batch_a, n_segments_a};
  const HostSide b{coeffs_b, times_b, start_b, times_b_stride_b, times_b_stride_k, batch_b, n_segments_b};
  mtgs::with_instance<mtgp::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, dimension, a, b, n_pairs, pairs, min_separation, pair_feasible, first_failing_segment_a,
                             first_failing_segment_b, pair_separation, pair_closest_time, pair_closest_segment_a, pair_closest_segment_b,
                             segment_separation, segment_closest_time, segment_closest_segment_b, segment_pieces);
  });
  return MTG_OK;
}
