// mtg_objective_host.cpp -- host build (plain g++, no HIP) of the time objective's maxima + soft-cost stage: the lane code of
// mtg_objective_lane.h run one segment after the other.  For callers that evaluate one trajectory at a time on the host
// (getTotalCostWithSoftConstraints' third term), and the CPU anchor of the device kernels.  Touches no device.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/mtg_hip.h"
#include "mtg_objective_lane.h"

extern "C" void mtg_time_objective_params_init(mtg_time_objective_params* p) {   // NonlinearOptimizationParameters' defaults
  if (!p) return;
  p->time_cost_kind = MTG_TIME_SQUARED_AND_CONSTRAINTS;
  p->use_soft_constraints = 1;
  p->time_penalty = 500.0;
  p->soft_constraint_weight = 100.0;
  p->maximum_cost = 1.0e12;
  p->n_constraints = 0;
  for (int q = 0; q < MTG_MAX_MAGNITUDE_CONSTRAINTS; ++q) { p->derivative[q] = 0; p->value[q] = 0.0; }
}

// mtg_time_objective_params -> the lane code's constraint list; shared with the device entries (mtg_objective.hip).
// Checks what does not depend on the shape; mtgo::arguments_ok checks the derivatives against N.
extern "C" int mtg_objective_constraints(const mtg_time_objective_params* in, mtgo::Constraints* out) {
  if (!in || !out) return MTG_ERR_INVALID_ARGUMENT;
  if (in->n_constraints < 0 || in->n_constraints > MTG_MAX_MAGNITUDE_CONSTRAINTS) return MTG_ERR_INVALID_ARGUMENT;
  if (in->time_cost_kind != MTG_TIME_SQUARED && in->time_cost_kind != MTG_TIME_RICHTER &&
      in->time_cost_kind != MTG_TIME_SQUARED_AND_CONSTRAINTS && in->time_cost_kind != MTG_TIME_RICHTER_AND_CONSTRAINTS)
    return MTG_ERR_INVALID_ARGUMENT;
  if (in->time_penalty != in->time_penalty || in->soft_constraint_weight != in->soft_constraint_weight ||
      in->maximum_cost != in->maximum_cost)
    return MTG_ERR_INVALID_ARGUMENT;
  out->n = in->n_constraints;
  for (int q = 0; q < mtgo::kMaxConstraints; ++q) {
    out->derivative[q] = q < in->n_constraints ? in->derivative[q] : 0;
    out->value[q] = q < in->n_constraints ? in->value[q] : 0.0;
  }
  return MTG_OK;
}

namespace {

// The device's fold (atomicMax on the bit pattern, mtg_objective.hip): magnitudes are >= +0, so unsigned order is numeric order,
// and a NaN segment maximum -- whatever its sign bit -- is above every number and stays.  (std::fmax dropped it: a trajectory
// of NaN coefficients reported maximum 0 and the best possible soft cost.)
double fold_max(double best, double m) {
  uint64_t a, b;
  std::memcpy(&a, &best, sizeof a);
  std::memcpy(&b, &m, sizeof b);
  return b > a ? m : best;
}

template <int NC, int DC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k,
         const mtgo::Constraints& con, const mtg_time_objective_params& par, double* cost_soft, double* maxima, double* violations) {
  double roots[mtgo::roots_len(NC)];
  double* r = roots;
  for (int64_t b = 0; b < B; ++b) {
    double best[mtgo::kMaxConstraints] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) {
      mtgo::segment_maxima<NC, DC, double*>(coeffs + (b * K + k) * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k], con, r,
                                            [&best](int q, double m) { best[q] = fold_max(best[q], m); });
    }
    double soft = 0.0;
    for (int q = 0; q < con.n; ++q) {
      if (par.use_soft_constraints) soft += mtgo::soft_term(best[q], con.value[q], par.soft_constraint_weight, par.maximum_cost);
      if (maxima) maxima[b * con.n + q] = best[q];
      if (violations) violations[b * con.n + q] = best[q] - con.value[q];
    }
    cost_soft[b] = soft;
  }
}

}  // namespace

extern "C" int mtg_magnitude_soft_cost_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                            const double* coeffs, const double* times, int64_t times_stride_b,
                                            int64_t times_stride_k, const mtg_time_objective_params* params, double* cost_soft,
                                            double* maxima, double* violations) {
  if (!coeffs || !times || !params || !cost_soft) return MTG_ERR_INVALID_ARGUMENT;
  mtgo::Constraints con;
  if (mtg_objective_constraints(params, &con) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgo::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, con))
    return MTG_ERR_INVALID_ARGUMENT;
  mtgs::with_instance<4>(n_coeffs, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    if (dimension <= 3) run<NC, 3>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k,
                                   con, *params, cost_soft, maxima, violations);
    else run<NC, 4>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, con, *params,
                    cost_soft, maxima, violations);
  });
  return MTG_OK;
}

extern "C" int mtg_time_cost_host(const mtg_time_objective_params* params, int32_t n_segments, int64_t batch, const double* times,
                                  int64_t times_stride_b, int64_t times_stride_k, double* cost_time) {
  mtgo::Constraints con;
  if (!times || !cost_time || n_segments < 1 || batch < 0 || times_stride_b < 1 || times_stride_k < 1) return MTG_ERR_INVALID_ARGUMENT;
  if (mtg_objective_constraints(params, &con) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < batch; ++b) {
    double total_time = 0.0;
    for (int k = 0; k < n_segments; ++k) total_time += times[b * times_stride_b + k * times_stride_k];
    cost_time[b] = mtgo::time_cost(params->time_cost_kind, params->time_penalty, total_time);
  }
  return MTG_OK;
}
