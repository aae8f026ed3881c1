// mtg_feasibility_host.cpp -- host build (plain g++, no HIP) of the analytic input-feasibility check: the lane code of
// mtg_feasibility_lane.h run one segment after the other.  For the reference's one-trajectory-at-a-time callers
// (FeasibilityAnalytic::checkInputFeasibility(Segment) / ...Trajectory): the project's design for single calls, as
// MTG_FLAG_HOST_BACKEND is for single solves.  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_feasibility_lane.h"

// mtg_input_constraints -> lane limits: magnitudes (InputConstraints::addConstraint and Settings::setMinSectionTimeS store
// |value|), NaN stays "absent".  Shared with the device entry (mtg_feasibility.hip).
extern "C" int mtg_feasibility_limits(const mtg_input_constraints* in, mtgf::Limits* out) {
  if (!in || !out) return MTG_ERR_INVALID_ARGUMENT;
  out->f_min = std::fabs(in->f_min);
  out->f_max = std::fabs(in->f_max);
  out->v_max = std::fabs(in->v_max);
  out->omega_xy_max = std::fabs(in->omega_xy_max);
  out->omega_z_max = std::fabs(in->omega_z_max);
  out->omega_z_dot_max = std::fabs(in->omega_z_dot_max);
  out->min_section_time_s = std::fabs(in->min_section_time_s);
  out->gravity = in->gravity;
  return MTG_OK;
}

extern "C" void mtg_input_constraints_init(mtg_input_constraints* c) {
  if (!c) return;
  c->f_min = c->f_max = c->v_max = c->omega_xy_max = c->omega_z_max = c->omega_z_dot_max = NAN;
  c->min_section_time_s = 0.05;   // FeasibilityAnalytic::Settings::Settings()
  c->gravity = 9.81;              // mav_msgs::kGravity
}

extern "C" void mtg_input_constraints_set_defaults(mtg_input_constraints* c) {   // InputConstraints::setDefaultValues
  if (!c) return;
  const double g = c->gravity == c->gravity ? c->gravity : 9.81;
  c->f_min = 0.5 * g;
  c->f_max = 1.5 * g;
  c->v_max = 3.0;
  c->omega_xy_max = M_PI / 2.0;
  c->omega_z_max = M_PI / 2.0;
  c->omega_z_dot_max = 2.0 * M_PI;
}

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k,
         const mtgf::Limits& lim, int32_t* traj, int32_t* first, int32_t* seg_result, double* seg_bounds) {
  double roots[mtgf::roots_len(NC)], cand[mtgf::cand_thrust_len(NC)], cand_jerk[mtgf::cand_jerk_len(NC)];
  double* r = roots;
  double* ct = cand;
  double* cj = cand_jerk;
  for (int64_t b = 0; b < B; ++b) {
    int result = mtgf::kFeasible, failing = -1;
    for (int k = 0; k < K; ++k) {
      // (every segment is checked, as on the device: the per-segment tables are complete whatever fails first)
      if (result != mtgf::kFeasible && !seg_result && !seg_bounds) break;
      double bounds[mtgf::kNumBounds];
      const int64_t idx = b * K + k;
      const int v = mtgf::segment_check<NC, double*, double*>(coeffs + idx * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k], lim,
                                                              r, ct, cj, bounds);
      if (seg_result) seg_result[idx] = v;
      if (seg_bounds)
        for (int q = 0; q < mtgf::kNumBounds; ++q) seg_bounds[idx * mtgf::kNumBounds + q] = bounds[q];
      if (v != mtgf::kFeasible && result == mtgf::kFeasible) { result = v; failing = k; }
    }
    traj[b] = result;
    if (first) first[b] = failing;
  }
}

}  // namespace

extern "C" int mtg_check_input_feasibility_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                                const double* coeffs, const double* times, int64_t times_stride_b,
                                                int64_t times_stride_k, const mtg_input_constraints* constraints,
                                                int32_t* trajectory_result, int32_t* first_failing_segment,
                                                int32_t* segment_result, double* segment_bounds) {
  if (!coeffs || !times || !constraints || !trajectory_result) return MTG_ERR_INVALID_ARGUMENT;
  mtgf::Limits lim;
  if (mtg_feasibility_limits(constraints, &lim) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, lim))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<6>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, lim,
                             trajectory_result, first_failing_segment, segment_result, segment_bounds);
  });
  return MTG_OK;
}
