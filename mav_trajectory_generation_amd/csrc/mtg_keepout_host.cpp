// mtg_keepout_host.cpp -- host build (plain g++, no HIP) of the keep-out zone check: the lane code of mtg_keepout_lane.h run one
// segment after the other, and the helper that turns boxes into zones.  For one-trajectory-at-a-time callers.  Touches no
// device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_keepout_lane.h"

extern "C" int mtg_keep_out_boxes(int32_t n, const double* centers, const double* sizes, double* out) {
  if (n < 0 || (n > 0 && (!centers || !sizes || !out))) return MTG_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < 3 * (int64_t)n; ++i)
    if (!(sizes[i] > 0.0) || !std::isfinite(sizes[i])) return MTG_ERR_INVALID_ARGUMENT;
  for (int32_t i = 0; i < n; ++i) {
    const int rc = mtg_half_planes_bounding_box(centers + 3 * (int64_t)i, sizes + 3 * (int64_t)i, out + 24 * (int64_t)i);
    if (rc != MTG_OK) return rc;
  }
  return MTG_OK;
}

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const double* zones,
         int M, int P, int64_t zs_b, double inflation, int32_t* feasible, int32_t* first_seg, int32_t* first_zone, double* seg_clearance,
         int32_t* seg_nearest, double* seg_time, double* traj_clearance) {
  double roots[mtgk::roots_len(NC)];
  double* r = roots;
  for (int64_t b = 0; b < B; ++b) {
    int fseg = -1, fzone = -1;
    double lowest = INFINITY;
    for (int k = 0; k < K; ++k) {   // (every segment is checked, as on the device: the clearances are complete whatever fails first)
      const int64_t idx = b * K + k;
      mtgk::Fold f;
      mtgk::segment_check<NC, double*>(coeffs + idx * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k], zones + b * zs_b, M, P,
                                       inflation, r, f);
      if (seg_clearance) seg_clearance[idx] = f.clearance;
      if (seg_nearest) seg_nearest[idx] = f.nearest;
      if (seg_time) seg_time[idx] = f.time;
      if (lowest == lowest && (f.clearance != f.clearance || f.clearance < lowest)) lowest = f.clearance;   // (a NaN wins)
      if (f.failing < mtgk::kMaxZones && fseg < 0) { fseg = k; fzone = f.failing; }
    }
    feasible[b] = fseg < 0 ? 1 : 0;
    if (first_seg) first_seg[b] = fseg;
    if (first_zone) first_zone[b] = fzone;
    if (traj_clearance) traj_clearance[b] = lowest;
  }
}

}  // namespace

extern "C" int mtg_check_keep_out_zones_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                             const double* times, int64_t times_stride_b, int64_t times_stride_k, const double* zones,
                                             int32_t n_zones, int32_t n_planes, int64_t zones_stride_b, double inflation,
                                             int32_t* trajectory_feasible, int32_t* first_failing_segment, int32_t* first_failing_zone,
                                             double* segment_clearance, int32_t* segment_nearest_zone, double* segment_closest_time,
                                             double* trajectory_clearance) {
  if (!coeffs || !times || !zones || !trajectory_feasible) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgk::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_zones, n_planes, zones_stride_b,
                          inflation))
    return MTG_ERR_INVALID_ARGUMENT;
  // the host can read the zones: every normal of every set in use must have unit length (|n|^2 within 1e-9 of 1) and every
  // offset must be finite
  const int64_t nb = zones_stride_b ? batch : (batch > 0 ? 1 : 0);
  for (int64_t b = 0; b < nb; ++b)
    for (int64_t h = 0; h < (int64_t)n_zones * n_planes; ++h) {
      const double* v = zones + b * zones_stride_b + 4 * h;
      if (!(std::fabs(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] - 1.0) <= 1e-9) || !std::isfinite(v[3])) return MTG_ERR_INVALID_ARGUMENT;
    }
  mtgs::with_instance<mtgk::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, zones, n_zones,
                             n_planes, zones_stride_b, inflation, trajectory_feasible, first_failing_segment, first_failing_zone,
                             segment_clearance, segment_nearest_zone, segment_closest_time, trajectory_clearance);
  });
  return MTG_OK;
}
