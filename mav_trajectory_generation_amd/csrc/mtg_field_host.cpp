// mtg_field_host.cpp -- host build (plain g++, no HIP) of the distance-field clearance check: the lane code of mtg_field_lane.h
// run one segment after the other, every sample in index order.  For one-trajectory-at-a-time callers and as the reproducible
// form of every rule in include/mtg_hip.h.  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_field_lane.h"

extern "C" void mtg_distance_field_init(mtg_distance_field* field) {
  if (!field) return;
  *field = mtg_distance_field{};
  field->interpolation = MTG_FIELD_TRILINEAR;
}

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const mtgf::Grid& g,
         double dt, int max_samples, double inflation, int32_t* feasible, int32_t* first_seg, double* seg_clearance,
         int32_t* seg_closest, int32_t* seg_first_failing, int32_t* seg_samples, double* traj_clearance) {
  for (int64_t b = 0; b < B; ++b) {
    int fseg = -1;
    unsigned long long lowest = ~0ull;
    for (int k = 0; k < K; ++k) {   // (every segment is checked, as on the device: the clearances are complete whatever fails first)
      const int64_t idx = b * K + k;
      const double T = times[b * ts_b + k * ts_k];
      double p[3][NC];
      mtgs::load_padded<NC, 3>(coeffs + idx * (int64_t)(D * N), N, D, p);
      const int S = mtgf::sample_count(T, dt, max_samples);
      mtgf::Fold f;
      mtgf::fold_samples<NC>(p, T, dt, S, 0, 1, g, inflation, f);
      const mtgf::SegmentResult r = mtgf::segment_result(f, S);
      if (seg_clearance) seg_clearance[idx] = r.clearance;
      if (seg_closest) seg_closest[idx] = r.closest;
      if (seg_first_failing) seg_first_failing[idx] = r.first_failing;
      if (seg_samples) seg_samples[idx] = r.samples;
      const unsigned long long key = mtgf::order_key(r.clearance);
      if (key < lowest) lowest = key;
      if (r.fails && fseg < 0) fseg = k;
    }
    feasible[b] = fseg < 0 ? 1 : 0;
    if (first_seg) first_seg[b] = fseg;
    if (traj_clearance) traj_clearance[b] = mtgf::order_value(lowest);
  }
}

}  // namespace

extern "C" int mtg_check_distance_field_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                             const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                             const mtg_distance_field* field, double dt, int32_t max_samples, double inflation,
                                             int32_t* trajectory_feasible, int32_t* first_failing_segment, double* segment_clearance,
                                             int32_t* segment_closest_sample, int32_t* segment_first_failing_sample,
                                             int32_t* segment_samples, double* trajectory_clearance) {
  if (!coeffs || !times || !trajectory_feasible) return MTG_ERR_INVALID_ARGUMENT;
  mtgf::Grid g;
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, dt, max_samples, inflation, &g))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<mtgf::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, g, dt, max_samples,
                             inflation, trajectory_feasible, first_failing_segment, segment_clearance, segment_closest_sample,
                             segment_first_failing_sample, segment_samples, trajectory_clearance);
  });
  return MTG_OK;
}
