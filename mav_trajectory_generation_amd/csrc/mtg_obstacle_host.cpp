// mtg_obstacle_host.cpp -- host build (plain g++, no HIP) of the sphere-obstacle clearance check: the lane code of
// mtg_obstacle_lane.h run one segment after the other.  For the reference's one-trajectory-at-a-time callers
// (Trajectory::offsetTrajectory + computeMinMaxMagnitude per obstacle).  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_obstacle_lane.h"

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const double* obstacles,
         int M, int64_t os_b, double inflation, int32_t* feasible, int32_t* first_seg, int32_t* first_obstacle, double* seg_clearance,
         int32_t* seg_nearest, double* seg_time, double* traj_clearance) {
  double roots[mtgo::buffer_len(NC)];
  double* r = roots;
  for (int64_t b = 0; b < B; ++b) {
    int fseg = -1, fobstacle = -1;
    double lowest = INFINITY;
    for (int k = 0; k < K; ++k) {   // (every segment is checked, as on the device: the clearances are complete whatever fails first)
      const int64_t idx = b * K + k;
      mtgo::Fold f;
      mtgo::segment_check<NC, double*>(coeffs + idx * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k], obstacles + b * os_b, M,
                                       inflation, r, f);
      if (seg_clearance) seg_clearance[idx] = f.clearance;
      if (seg_nearest) seg_nearest[idx] = f.nearest;
      if (seg_time) seg_time[idx] = f.time;
      if (lowest == lowest && (f.clearance != f.clearance || f.clearance < lowest)) lowest = f.clearance;   // (a NaN wins)
      if (f.failing < mtgo::kMaxObstacles && fseg < 0) { fseg = k; fobstacle = f.failing; }
    }
    feasible[b] = fseg < 0 ? 1 : 0;
    if (first_seg) first_seg[b] = fseg;
    if (first_obstacle) first_obstacle[b] = fobstacle;
    if (traj_clearance) traj_clearance[b] = lowest;
  }
}

}  // namespace

extern "C" int mtg_check_obstacle_clearance_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                                 const double* coeffs, const double* times, int64_t times_stride_b,
                                                 int64_t times_stride_k, const double* obstacles, int32_t n_obstacles,
                                                 int64_t obstacles_stride_b, double inflation, int32_t* trajectory_feasible,
                                                 int32_t* first_failing_segment, int32_t* first_failing_obstacle,
                                                 double* segment_clearance, int32_t* segment_nearest_obstacle,
                                                 double* segment_closest_time, double* trajectory_clearance) {
  if (!coeffs || !times || !obstacles || !trajectory_feasible) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgo::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_obstacles, obstacles_stride_b,
                          inflation))
    return MTG_ERR_INVALID_ARGUMENT;
  // the host can read the obstacles: every radius of every set in use must be >= 0 and finite
  const int64_t nb = obstacles_stride_b ? batch : (batch > 0 ? 1 : 0);
  for (int64_t b = 0; b < nb; ++b)
    for (int h = 0; h < n_obstacles; ++h) {
      const double radius = obstacles[b * obstacles_stride_b + 4 * h + 3];
      if (!(radius >= 0.0) || !std::isfinite(radius)) return MTG_ERR_INVALID_ARGUMENT;
    }
  mtgs::with_instance<mtgo::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, obstacles,
                             n_obstacles, obstacles_stride_b, inflation, trajectory_feasible, first_failing_segment,
                             first_failing_obstacle, segment_clearance, segment_nearest_obstacle, segment_closest_time,
                             trajectory_clearance);
  });
  return MTG_OK;
}
