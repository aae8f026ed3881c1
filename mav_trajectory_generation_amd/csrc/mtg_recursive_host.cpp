// mtg_recursive_host.cpp -- host build (plain g++, no HIP) of the recursive input-feasibility check: the lane code of
// mtg_recursive_lane.h run one segment after the other.  For the reference's one-trajectory-at-a-time callers
// (FeasibilityRecursive::checkInputFeasibility(Segment) / ...Trajectory), as mtg_feasibility_host.cpp is for the analytic
// check.  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_recursive_lane.h"

extern "C" int mtg_feasibility_limits(const mtg_input_constraints* in, mtgf::Limits* out);   // mtg_feasibility_host.cpp

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k,
         const mtgf::Limits& lim, int32_t* traj, int32_t* first, int32_t* seg_result, double* seg_bounds, int32_t* seg_sections) {
  double scratch[mtgr::scratch_len(NC)], store[mtgr::store_len(NC)];
  double* sc = scratch;
  double* st = store;
  for (int64_t b = 0; b < B; ++b) {
    int result = mtgf::kFeasible, failing = -1;
    for (int k = 0; k < K; ++k) {
      // (every segment is checked, as on the device: the per-segment tables are complete whatever fails first)
      if (result != mtgf::kFeasible && !seg_result && !seg_bounds && !seg_sections) break;
      double bounds[mtgr::kNumBounds];
      int sections = 0;
      const int64_t idx = b * K + k;
      const int v = mtgr::segment_check<NC, double*>(coeffs + idx * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k], lim, sc, st,
                                                     bounds, sections);
      if (seg_result) seg_result[idx] = v;
      if (seg_sections) seg_sections[idx] = sections;
      if (seg_bounds)
        for (int q = 0; q < mtgr::kNumBounds; ++q) seg_bounds[idx * mtgr::kNumBounds + q] = bounds[q];
      if (v != mtgf::kFeasible && result == mtgf::kFeasible) { result = v; failing = k; }
    }
    traj[b] = result;
    if (first) first[b] = failing;
  }
}

}  // namespace

extern "C" int mtg_check_input_feasibility_recursive_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                                          const double* coeffs, const double* times, int64_t times_stride_b,
                                                          int64_t times_stride_k, const mtg_input_constraints* constraints,
                                                          int32_t* trajectory_result, int32_t* first_failing_segment,
                                                          int32_t* segment_result, double* segment_bounds,
                                                          int32_t* segment_sections) {
  if (!coeffs || !times || !constraints || !trajectory_result) return MTG_ERR_INVALID_ARGUMENT;
  mtgf::Limits lim;
  if (mtg_feasibility_limits(constraints, &lim) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, lim))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<6>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, lim,
                             trajectory_result, first_failing_segment, segment_result, segment_bounds, segment_sections);
  });
  return MTG_OK;
}
