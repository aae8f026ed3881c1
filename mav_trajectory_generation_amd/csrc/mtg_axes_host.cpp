// mtg_axes_host.cpp -- host build (plain g++, no HIP) of the per-axis extrema: the lane code of mtg_axes_lane.h run one
// (segment, axis) after the other, then the reduction over segments.  For the reference's one-polynomial-at-a-time callers
// (Polynomial::computeMinMax), as mtg_recursive_host.cpp is for the recursive check.  Touches no device: works in a process
// without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_axes_lane.h"

namespace {

template <int NC, int FIRST>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, int n, double* seg) {
  double buf[mtga::roots_len(NC, FIRST)];
  double* roots = buf;
  for (int64_t b = 0; b < B; ++b)
    for (int k = 0; k < K; ++k) {
      const int64_t idx = b * K + k;
      const double T = times[b * ts_b + k * ts_k];
      for (int d = 0; d < D; ++d) {
        mtga::Row row[mtga::orders(FIRST)];
        mtga::axis_minmax<NC, FIRST, double*>(coeffs + (idx * D + d) * (int64_t)N, N, T, n, roots, row);
        double* o = seg + (idx * D + d) * (int64_t)(4 * n);
        for (int j = 0; j < n; ++j) {
          o[4 * j] = row[j].t_min; o[4 * j + 1] = row[j].v_min; o[4 * j + 2] = row[j].t_max; o[4 * j + 3] = row[j].v_max;
        }
      }
    }
}

}  // namespace

extern "C" int mtg_minmax_axes_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                    const double* times, int64_t times_stride_b, int64_t times_stride_k, int32_t derivative_first,
                                    int32_t n_derivatives, double* segment_minmax, double* trajectory_minmax,
                                    int32_t* trajectory_segment_idx) {
  if (!coeffs || !times || !segment_minmax) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtga::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, derivative_first, n_derivatives))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<mtga::kMinInstance>(n_coeffs, [&](auto nc) {
    mtga::with_first(derivative_first, [&](auto first) {
      run<decltype(nc)::value, decltype(first)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b,
                                                       times_stride_k, n_derivatives, segment_minmax);
    });
  });
  if (trajectory_minmax) {
    const int64_t per_traj = (int64_t)dimension * n_derivatives;
    for (int64_t i = 0; i < batch * per_traj; ++i) {
      const int64_t b = i / per_traj;
      mtga::Row r;
      int k_min, k_max;
      mtga::reduce_rows(segment_minmax + (b * n_segments * per_traj + (i - b * per_traj)) * 4, per_traj * 4, n_segments, r, k_min, k_max);
      double* o = trajectory_minmax + i * 4;
      o[0] = r.t_min; o[1] = r.v_min; o[2] = r.t_max; o[3] = r.v_max;
      if (trajectory_segment_idx) {
        trajectory_segment_idx[2 * i] = k_min;
        trajectory_segment_idx[2 * i + 1] = k_max;
      }
    }
  }
  return MTG_OK;
}
