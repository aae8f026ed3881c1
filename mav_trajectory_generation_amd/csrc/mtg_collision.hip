// mtg_collision.hip -- batched distance-field collision cost and its gradient with respect to the polynomial coefficients: for a
// batch of solved trajectories (coeffs [B][K][D][N]) and a trilinear voxel grid of float distances (an ESDF), per segment
// sum_i w_i c(d(p(t_i)) - inflation) s(t_i) and its exact derivative -> mtg_collision_cost.  The rules (weights, a sample's terms,
// the order of every sum) live in mtg_collision_lane.h.  Mapping: one wavefront per (trajectory, segment) of the frame of
// mtg_segment_kernel.h, as in mtg_field.hip; lane g keeps the three position polynomials in registers, takes samples g, g + 64, ..
// and accumulates 1 + 3 NC partial sums; the 64 partials are joined by the xor butterfly (32, 16, .. 1), after which every lane
// holds every total and lane l stores gradient entry l: one coalesced store per segment.  Two instantiations per NC, with and
// without the gradient.  A lane per trajectory then adds the written segment costs in segment order.  No LDS, no workspace, no
// floating-point atomics; the grid is read with plain global loads.
#include "mtg_collision_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // one wavefront per workgroup = per segment

struct CollisionParams {
  mtgs::SegShape s;
  mtgf::Grid g;
  mtgc::Potential q;
  double dt;
  int max_samples;
  double* seg_cost;      // [B][K]
  double* traj_cost;     // [B] or null
  double* grad;          // [B][K][D][N] or null
  int* seg_samples;      // [B][K] or null
};

template <int NC, bool GRAD>
__global__ __launch_bounds__(kThreads) void mtg_collision_seg_kernel(CollisionParams P) {
  static_assert(kThreads == mtgc::kPartials, "one partial sum per lane");
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x);   // (the grid has exactly B K workgroups)
  if (!L.in_range) return;
  const int lane = (int)threadIdx.x;
  double p[3][NC];
  mtgs::load_padded<NC, 3>(L.c, P.s.N, P.s.D, p);
  const int S = mtgf::sample_count(L.T, P.dt, P.max_samples);
  mtgc::Sums<NC, GRAD> sum;
  mtgc::clear(sum);
  mtgc::sum_samples<NC, GRAD>(p, L.T, P.dt, S, lane, kThreads, P.g, P.q, sum);
#pragma unroll
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    sum.cost = sum.cost + __shfl_xor(sum.cost, off);
    if constexpr (GRAD) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int j = 0; j < NC; ++j) sum.grad[a][j] = sum.grad[a][j] + __shfl_xor(sum.grad[a][j], off);
    }
  }
  if (lane == 0) {
    P.seg_cost[L.idx] = S < 0 ? NAN : sum.cost;
    if (P.seg_samples) P.seg_samples[L.idx] = S;
  }
  if constexpr (GRAD) {
    const int N = P.s.N, DN = P.s.D * N;   // DN <= 48: one store per lane
    if (lane < DN) {
      double value = 0.0;                 // (the yaw rows stay 0)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int j = 0; j < NC; ++j)
          if (j < N && lane == a * N + j) value = sum.grad[a][j];
      if (S < 0 && lane < 3 * N) value = NAN;
      P.grad[L.idx * (long long)DN + lane] = value;
    }
  }
}

__global__ void mtg_collision_traj_kernel(CollisionParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  double total = 0.0;
  for (int k = 0; k < P.s.K; ++k) total = total + P.seg_cost[b * P.s.K + k];
  P.traj_cost[b] = total;
}

}  // namespace

extern "C" int mtg_collision_cost(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                  const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                  const mtg_distance_field* field, double dt, int32_t max_samples, double inflation, double epsilon,
                                  double speed_epsilon, double* segment_cost, double* trajectory_cost, double* coeff_gradient,
                                  int32_t* segment_samples) {
  // (the argument checks come first and need no context: mtg_context_set_last_error records nothing without one)
  if (!coeffs || !times || !field || !field->distances || !segment_cost)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "collision cost: coeffs, times, field, field->distances and segment_cost are required");
  CollisionParams P;
  if (!mtgc::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, dt, max_samples, inflation,
                          epsilon, speed_epsilon, &P.g, &P.q))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "collision cost: the arguments of the distance-field check with a trilinear field; epsilon > 0 and "
                                      "speed_epsilon >= 0, both finite");
  if ((long long)batch * n_segments > 0x7fffffffll)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "collision cost: batch x n_segments is beyond one launch");
  if (batch == 0) return MTG_OK;
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.dt = dt; P.max_samples = max_samples;
  P.seg_cost = segment_cost; P.traj_cost = trajectory_cost; P.grad = coeff_gradient; P.seg_samples = segment_samples;
  const dim3 per_segment((unsigned)(batch * n_segments));
  mtgs::with_instance<mtgc::kMinInstance>(n_coeffs, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    if (coeff_gradient) hipLaunchKernelGGL((mtg_collision_seg_kernel<NC, true>), per_segment, dim3(kThreads), 0, stream, P);
    else hipLaunchKernelGGL((mtg_collision_seg_kernel<NC, false>), per_segment, dim3(kThreads), 0, stream, P);
  });
  if (trajectory_cost) hipLaunchKernelGGL(mtg_collision_traj_kernel, mtgs::grid_for(batch, 256), dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
