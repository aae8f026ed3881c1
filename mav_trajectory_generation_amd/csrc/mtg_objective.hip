// mtg_objective.hip -- batched nonlinear time objective with soft constraints (the callbacks of PolynomialOptimizationNonLinear<N>).
//
// objective = cost_trajectory + cost_time + cost_soft for a batch of segment-time vectors -> mtg_time_objective; the maxima +
// soft-cost stage alone on existing coefficients -> mtg_magnitude_soft_cost.  The per-lane algorithm lives in
// mtg_objective_lane.h on top of the root isolation of mtg_extrema_lane.h.  Mapping of the search: one lane per (trajectory,
// segment), 64-lane workgroups; the lane reads its D x N coefficients once into registers and searches every constrained
// derivative on them one after the other, so the searches share the two LDS root buffers ([slot][lane] layout, as in
// mtg_extrema.hip).  Only the largest candidate value is kept; the lane folds it into its trajectory's slot with a 64-bit
// atomic maximum on the BIT PATTERN -- magnitudes are non-negative, so unsigned order is numeric order, and the result does not
// depend on which lane arrives first; a NaN maximum (non-finite coefficients: mtg_objective_lane.h) is above every number in that
// order and stays, whichever segment it comes from.  A lane per trajectory then forms the components (cost arithmetic: mtg_objective_lane.h).
#include <cmath>

#include "mtg_objective_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // roots per lane: 30 doubles at N = 10 (15 KB per workgroup), 38 at N = 12 (19 KB)

struct ObjParams {
  mtgs::SegShape s;
  unsigned long long* slots;   // [B][slot_stride]: bit patterns of the maxima so far; zero-filled before the search
  int slot_stride;
  const double* cost_trajectory;   // [B] or null (soft cost alone)
  const int* tstatus;              // [B] or null: per-trajectory status of the solve
  double* objective;      // [B] or null
  double* components;     // [B][3] or null
  double* cost_soft;      // [B] or null
  double* maxima;         // [B][n] or null (may alias slots when slot_stride == n)
  double* violations;     // [B][n] or null
  int time_cost_kind, use_soft;
  double time_penalty, weight, maximum_cost;
  mtgo::Constraints con;
};

template <int NC, int DC>
__global__ __launch_bounds__(kThreads) void mtg_objective_seg_kernel(ObjParams P) {
  extern __shared__ double lds[];
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x * kThreads + threadIdx.x);
  if (!L.in_range) return;
  mtgs::LdsColumn<kThreads> roots{lds + threadIdx.x};
  unsigned long long* slot = P.slots + L.b * P.slot_stride;
  mtgo::segment_maxima<NC, DC, mtgs::LdsColumn<kThreads>>(L.c, P.s.N, P.s.D, L.T, P.con, roots, [slot](int q, double m) {
    atomicMax(slot + q, (unsigned long long)__double_as_longlong(m));
  });
}

// objectiveFunctionTime / ...AndConstraints after the solve (polynomial_optimization_nonlinear_impl.h:572-614, :698-741)
__global__ void mtg_objective_finish_kernel(ObjParams P) {
  // every product and sum rounded on its own, as in the reference's host code: the total IS the sum of the components written
  // next to it (contracted, cost_trajectory + T * T * penalty became one fused operation and differed from it in the last bit)
#pragma clang fp contract(off)
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  double total_time = 0.0;
  bool bad = P.tstatus && P.tstatus[b] != 0;
  for (int k = 0; k < P.s.K; ++k) {   // computeTotalTrajectoryTime: in segment order
    const double T = P.s.times[b * P.s.ts_b + (long long)k * P.s.ts_k];
    bad = bad || !(T > 0.0);
    total_time += T;
  }
  double mx[mtgo::kMaxConstraints];
#pragma unroll
  for (int q = 0; q < mtgo::kMaxConstraints; ++q)
    mx[q] = q < P.con.n ? __longlong_as_double((long long)P.slots[b * P.slot_stride + q]) : 0.0;
  double soft = 0.0;
#pragma unroll
  for (int q = 0; q < mtgo::kMaxConstraints; ++q) {
    if (q < P.con.n) {
      if (P.use_soft) soft += mtgo::soft_term(mx[q], P.con.value[q], P.weight, P.maximum_cost);
      if (P.maxima) P.maxima[b * P.con.n + q] = mx[q];
      if (P.violations) P.violations[b * P.con.n + q] = mx[q] - P.con.value[q];
    }
  }
  if (P.cost_soft) P.cost_soft[b] = soft;
  if (P.objective) {
    const double cost_trajectory = P.cost_trajectory[b];
    const double cost_time = mtgo::time_cost(P.time_cost_kind, P.time_penalty, total_time);
    P.objective[b] = bad ? INFINITY : cost_trajectory + cost_time + soft;
    if (P.components) {
      P.components[3 * b] = cost_trajectory;
      P.components[3 * b + 1] = cost_time;
      P.components[3 * b + 2] = soft;
    }
  }
}

template <int NC, int DC>
void launch_seg(const ObjParams& P, hipStream_t stream) {
  const size_t lds = (size_t)kThreads * mtgo::roots_len(NC) * sizeof(double);
  hipLaunchKernelGGL((mtg_objective_seg_kernel<NC, DC>), mtgs::grid_for(P.s.B * P.s.K, kThreads), dim3(kThreads), lds, stream, P);
}

// zero the slots, search, finish.  P.slots / P.slot_stride set by the caller.
int run_stages(const ObjParams& P, hipStream_t stream) {
  if (P.con.n > 0) {
    if (hipMemsetAsync(P.slots, 0, (size_t)P.s.B * P.slot_stride * sizeof(double), stream) != hipSuccess) return MTG_ERR_DEVICE;
    mtgs::with_instance<4>(P.s.N, [&](auto nc) {
      if (P.s.D <= 3) launch_seg<decltype(nc)::value, 3>(P, stream);
      else launch_seg<decltype(nc)::value, 4>(P, stream);
    });
  }
  hipLaunchKernelGGL(mtg_objective_finish_kernel, mtgs::grid_for(P.s.B, 256), dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}

void fill_params(ObjParams& P, const mtg_time_objective_params& par) {
  P.time_cost_kind = par.time_cost_kind; P.use_soft = par.use_soft_constraints;
  P.time_penalty = par.time_penalty; P.weight = par.soft_constraint_weight; P.maximum_cost = par.maximum_cost;
}

}  // namespace

extern "C" int mtg_plan_objective_solve(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                        const double* d_fixed, const double* d_free_in, double* coeffs, double** cost, double** slots,
                                        int32_t** tstatus);   // mtg_dispatch.hip
extern "C" int mtg_objective_constraints(const mtg_time_objective_params* in, mtgo::Constraints* out);   // mtg_objective_host.cpp

extern "C" int mtg_time_objective(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                  const double* d_fixed, const double* d_free_in, const mtg_time_objective_params* params,
                                  double* coeffs, double* objective, double* components, double* maxima, double* violations) {
  if (!plan) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = mtg_plan_context(plan);
  if (!layout || !times || !params || !coeffs || !objective)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "time objective: layout, times, params, coeffs and objective are required");
  ObjParams P{};
  if (mtg_objective_constraints(params, &P.con) != MTG_OK)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "time objective: n_constraints in [0,4], a time-cost kind with a time term, parameters not NaN");
  int32_t n = 0, dim = 0, k = 0;
  mtg_plan_get_shape(plan, &n, &dim, &k, nullptr);
  if (!mtgo::arguments_ok(n, k, dim, batch, layout->times_stride_b, layout->times_stride_k, P.con))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "time objective: n_coeffs in [4,12], dimension <= 4, batch >= 0, times strides >= 1 that do not overlap, "
                                      "constraint derivatives in [1, N/2-1] with values > 0");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  double* cost = nullptr;
  double* slots = nullptr;
  int32_t* tstatus = nullptr;
  rc = mtg_plan_objective_solve(plan, batch, layout, times, d_fixed, d_free_in, coeffs, &cost, &slots, &tstatus);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, layout->times_stride_b, layout->times_stride_k, batch, n, k, dim};
  P.slots = reinterpret_cast<unsigned long long*>(slots); P.slot_stride = mtgo::kMaxConstraints;
  P.cost_trajectory = cost; P.tstatus = tstatus;
  P.objective = objective; P.components = components; P.cost_soft = nullptr; P.maxima = maxima; P.violations = violations;
  fill_params(P, *params);
  return run_stages(P, stream);
}

extern "C" int mtg_magnitude_soft_cost(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                       const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                       const mtg_time_objective_params* params, double* cost_soft, double* maxima,
                                       double* violations) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !params || !cost_soft)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "magnitude soft cost: coeffs, times, params and cost_soft are required");
  ObjParams P{};
  if (mtg_objective_constraints(params, &P.con) != MTG_OK)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "magnitude soft cost: n_constraints in [0,4], a time-cost kind with a time term, parameters not NaN");
  if (!mtgo::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, P.con))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "magnitude soft cost: n_coeffs in [4,12], dimension <= 4, batch >= 0, times strides >= 1 that do not overlap, "
                                      "constraint derivatives in [1, N/2-1] with values > 0");
  if (P.con.n > 0 && !maxima)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "magnitude soft cost: maxima is required (the search reduces into it)");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.slots = reinterpret_cast<unsigned long long*>(maxima); P.slot_stride = P.con.n;   // finished in place: the bits ARE the doubles
  P.cost_trajectory = nullptr; P.tstatus = nullptr;
  P.objective = nullptr; P.components = nullptr; P.cost_soft = cost_soft; P.maxima = nullptr; P.violations = violations;
  fill_params(P, *params);
  return run_stages(P, stream);
}
