// mtg_pullback.hip -- batched gradient with respect to the free derivatives: a coefficient-space gradient G [B][K][D][N]
// (mtg_collision_cost's output, and / or the derivative cost's gradient w Q(T) c formed on the fly from coeffs) pulled back
// through the transpose of the map mtg_update_segments_from_free applies -> mtg_free_gradient.  The rule (every rounding, the
// order of every sum) lives in mtg_pullback_lane.h.  Mapping: one lane per (trajectory, vertex, dimension), the dimension
// fastest, so that neighbouring lanes read neighbouring 8 N-byte coefficient rows; a lane forms the end half of segment v - 1
// and the start half of segment v (N h FMAs without coeffs) and writes its h outputs to the free or the fixed column its
// vertex's mask names.  No LDS, no workspace, no floating-point atomics: every output element has exactly one writer.
// One instantiation per N = 2, 4, .. 12; d, the masks and the column offsets are run-time values from the plan's device tables.
#include "mtg_pullback_lane.h"
#include "mtg_segment_kernel.h"

extern "C" int mtg_plan_context_tables(const mtg_plan* plan, mtg_context** ctx, int* n_coeffs, int* dimension, int* n_segments,
                                       const int** device_masks);   // mtg_plan.hip

namespace {

constexpr int kThreads = 256;

template <int N>
__global__ __launch_bounds__(kThreads) void mtg_free_gradient_kernel(mtgp::Params P) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  const long long per_traj = (long long)(P.K + 1) * P.D;
  if (idx >= P.B * per_traj) return;
  const long long b = idx / per_traj;
  const int r = (int)(idx - b * per_traj);
  const int v = r / P.D;
  mtgp::vertex_lane<N>(P, b, v, r - v * P.D);
}

}  // namespace

extern "C" int mtg_free_gradient(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                 const double* grad_coeffs, const double* coeffs, double smoothness_weight, double* grad_free,
                                 double* grad_fixed) {
  // (the argument checks come first and need no context)
  if (!plan || !mtgp::arguments_ok(batch, layout, times, grad_coeffs, coeffs, grad_free, grad_fixed)) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = nullptr;
  int N = 0, D = 0, K = 0, d = 0;
  const int* tables = nullptr;
  int rc = mtg_plan_context_tables(plan, &ctx, &N, &D, &K, &tables);
  if (rc != MTG_OK) return rc;
  rc = mtg_plan_get_shape(plan, nullptr, nullptr, nullptr, &d);
  if (rc != MTG_OK) return rc;
  const long long lanes_per_traj = (long long)(K + 1) * D;
  if (batch > 0x7fffffffll / lanes_per_traj)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "free gradient: batch x (n_segments + 1) x dimension is beyond one launch");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  mtgp::Params P;
  P.times = times; P.ts_b = layout->times_stride_b; P.ts_k = layout->times_stride_k;
  P.grad = grad_coeffs; P.coeffs = coeffs; P.w = smoothness_weight;
  P.gfree = grad_free; P.ps_b = layout->free_stride_b; P.ps_d = layout->free_stride_d; P.ps_c = layout->free_stride_c;
  P.gfixed = grad_fixed; P.fs_b = layout->fixed_stride_b; P.fs_d = layout->fixed_stride_d; P.fs_c = layout->fixed_stride_c;
  P.mask = tables; P.offF = tables + (K + 1); P.offP = tables + (K + 1) + (K + 2);
  P.B = batch; P.K = K; P.D = D; P.deriv = d; P.q1off = mtgp::q1_offset(N, d);
  const dim3 grid = mtgs::grid_for(batch * lanes_per_traj, kThreads);
  mtgs::with_instance<mtgp::kMinInstance>(N, [&](auto nc) {
    hipLaunchKernelGGL((mtg_free_gradient_kernel<decltype(nc)::value>), grid, dim3(kThreads), 0, stream, P);
  });
  const hipError_t launched = hipGetLastError();
  if (launched != hipSuccess) return mtg_context_set_last_error(ctx, MTG_ERR_DEVICE, hipGetErrorString(launched));
  return MTG_OK;
}
