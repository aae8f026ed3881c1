// mtg_axes.hip -- batched per-axis extrema: the signed minimum and maximum of single axes (Polynomial::computeMinMax).
//
// For a batch of solved trajectories (coeffs [B][K][D][N] as written by mtg_solve_linear): per (trajectory, segment, axis) the
// extrema over [0, T] of a contiguous range of derivative orders within position .. snap -> mtg_minmax_axes.  The per-lane
// algorithm lives in mtg_axes_lane.h on top of the root isolation of mtg_extrema_lane.h.  Mapping, on the frame of
// mtg_segment_kernel.h: one lane per (trajectory, segment, AXIS) -- seg_lane(S, lane / D), axis = lane % D -- so a lane holds NC
// coefficients, not D x NC: the searches of a segment's axes share nothing, and the launch has D times the lanes to hide the
// dependent FP64 chains.  One search of degree NC - 2 - FIRST per lane into two LDS root buffers ([slot][lane] layout); the
// rows of the orders asked for stay in registers and leave as one contiguous run per lane.  An optional second kernel, one lane
// per (trajectory, axis, order), scans the K rows of the segment table in segment order: deterministic whatever the first
// kernel's finishing order, no atomics.
#include "mtg_axes_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // root buffers: 2 (NC - 2 - FIRST) doubles per lane, 10 KB per workgroup at NC = 12, FIRST = 0

struct AxesParams {
  mtgs::SegShape s;
  int n;                 // orders asked for
  double* seg_minmax;    // [B][K][D][n][4]
  double* traj_minmax;   // [B][D][n][4] or null
  int* traj_idx;         // [B][D][n][2] or null
};

template <int NC, int FIRST>
__global__ __launch_bounds__(kThreads) void mtg_axes_seg_kernel(AxesParams P) {
  __shared__ double lds[mtga::roots_len(NC, FIRST) * kThreads];
  const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
  const mtgs::SegLane L = mtgs::seg_lane(P.s, lane / P.s.D);
  if (!L.in_range) return;
  const int axis = (int)(lane - L.idx * P.s.D);
  mtgs::LdsColumn<kThreads> roots{lds + threadIdx.x};
  mtga::Row row[mtga::orders(FIRST)];
  mtga::axis_minmax<NC, FIRST, mtgs::LdsColumn<kThreads>>(L.c + axis * P.s.N, P.s.N, L.T, P.n, roots, row);
  double2* o = reinterpret_cast<double2*>(P.seg_minmax + lane * (long long)(4 * P.n));   // (32 B per row: 16-byte aligned)
#pragma unroll
  for (int j = 0; j < mtga::orders(FIRST); ++j)
    if (j < P.n) {
      o[2 * j] = make_double2(row[j].t_min, row[j].v_min);
      o[2 * j + 1] = make_double2(row[j].t_max, row[j].v_max);
    }
}

__global__ void mtg_axes_traj_kernel(AxesParams P) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (trajectory, axis, order)
  const long long per_traj = (long long)P.s.D * P.n;
  if (i >= P.s.B * per_traj) return;
  const long long b = i / per_traj;
  mtga::Row r;
  int k_min, k_max;
  mtga::reduce_rows(P.seg_minmax + (b * P.s.K * per_traj + (i - b * per_traj)) * 4, per_traj * 4, P.s.K, r, k_min, k_max);
  double* o = P.traj_minmax + i * 4;
  o[0] = r.t_min; o[1] = r.v_min; o[2] = r.t_max; o[3] = r.v_max;
  if (P.traj_idx) {
    P.traj_idx[2 * i] = k_min;
    P.traj_idx[2 * i + 1] = k_max;
  }
}

}  // namespace

extern "C" int mtg_minmax_axes(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                               const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                               int32_t derivative_first, int32_t n_derivatives, double* segment_minmax, double* trajectory_minmax,
                               int32_t* trajectory_segment_idx) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !segment_minmax)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "per-axis extrema: coeffs, times and segment_minmax are required");
  if (!mtga::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, derivative_first, n_derivatives))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "per-axis extrema: n_coeffs in [2,12], n_segments >= 1, dimension in [1,8], batch >= 0, times strides "
                                      ">= 1 that do not overlap ([B][K] or [K][B]), derivative_first >= 0, n_derivatives >= 1, last order "
                                      "<= min(4, n_coeffs - 1)");
  if (reinterpret_cast<uintptr_t>(segment_minmax) & 15)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "per-axis extrema: segment_minmax must be 16-byte aligned");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  AxesParams P;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.n = n_derivatives;
  P.seg_minmax = segment_minmax; P.traj_minmax = trajectory_minmax; P.traj_idx = trajectory_segment_idx;
  mtgs::with_instance<mtga::kMinInstance>(n_coeffs, [&](auto nc) {
    mtga::with_first(derivative_first, [&](auto first) {
      hipLaunchKernelGGL((mtg_axes_seg_kernel<decltype(nc)::value, decltype(first)::value>),
                         mtgs::grid_for(P.s.B * P.s.K * P.s.D, kThreads), dim3(kThreads), 0, stream, P);
    });
  });
  if (P.traj_minmax)
    hipLaunchKernelGGL(mtg_axes_traj_kernel, mtgs::grid_for(P.s.B * P.s.D * P.n, 256), dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
