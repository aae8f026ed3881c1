// mtg_recursive.hip -- batched recursive input-feasibility check (FeasibilityRecursive of mav_trajectory_generation_ros).
//
// The cheap, conservative sibling of mtg_feasibility.hip -> mtg_check_input_feasibility_recursive.  The per-lane algorithm
// lives in mtg_recursive_lane.h on top of the root isolation of mtg_extrema_lane.h.  Mapping, on the frame of
// mtg_segment_kernel.h: one lane per (trajectory, segment); the lane reads its D x N coefficients once, finds the single-axis
// roots the present limits need (one search of degree N - 3 per axis, which delivers the jerk and snap roots on its way) into
// LDS columns ([slot][lane] layout) and then walks the reference's recursion over them without a stack.  Lanes of a wave leave the walk at different times: that
// divergence is the nature of the check.  A failing lane reports (segment << 8 | code) with an atomic minimum on its
// trajectory's word; a lane per trajectory then decodes the words.
#include "mtg_recursive_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // search buffers + root lists per lane: 68 doubles at N = 10 (34 KB per workgroup), 90 at N = 12 (45 KB)
using Column = mtgs::LdsColumn<kThreads>;

struct RecParams {
  mtgs::SegShape s;
  int* traj_word;         // [B]: mtgs::kNoFailure, or min over failing segments of (segment << 8 | code); decoded in place
  int* first_failing;     // [B] or null
  int* seg_result;        // [B][K] or null
  double* seg_bounds;     // [B][K][6] or null
  int* seg_sections;      // [B][K] or null
  mtgf::Limits lim;
};

template <int NC>
__global__ __launch_bounds__(kThreads) void mtg_recursive_seg_kernel(RecParams P) {
  extern __shared__ double lds[];
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x * kThreads + threadIdx.x);
  if (!L.in_range) return;
  Column scratch{lds + threadIdx.x};
  Column store{lds + (size_t)mtgr::scratch_len(NC) * kThreads + threadIdx.x};
  double bounds[mtgr::kNumBounds];
  int sections;
  const int verdict = mtgr::segment_check<NC, Column>(L.c, P.s.N, P.s.D, L.T, P.lim, scratch, store, bounds, sections);
  if (P.seg_result) P.seg_result[L.idx] = verdict;
  if (P.seg_sections) P.seg_sections[L.idx] = sections;
  if (P.seg_bounds) {
    double2* o = reinterpret_cast<double2*>(P.seg_bounds + L.idx * mtgr::kNumBounds);   // (48 B per segment: 16-byte aligned rows)
    o[0] = make_double2(bounds[0], bounds[1]);
    o[1] = make_double2(bounds[2], bounds[3]);
    o[2] = make_double2(bounds[4], bounds[5]);
  }
  if (verdict != mtgf::kFeasible) mtgs::report_failure(P.traj_word + L.b, L.seg, verdict);
}

// FeasibilityBase::checkInputFeasibilityTrajectory (feasibility_base.cpp:97-107): the first segment that is not feasible
__global__ void mtg_recursive_traj_kernel(RecParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == mtgs::kNoFailure ? mtgf::kFeasible : mtgs::failure_code(w);
  if (P.first_failing) P.first_failing[b] = w == mtgs::kNoFailure ? -1 : mtgs::failure_segment(w);
}

}  // namespace

extern "C" int mtg_feasibility_limits(const mtg_input_constraints* in, mtgf::Limits* out);   // mtg_feasibility_host.cpp

extern "C" int mtg_check_input_feasibility_recursive(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension,
                                                     int64_t batch, const double* coeffs, const double* times,
                                                     int64_t times_stride_b, int64_t times_stride_k,
                                                     const mtg_input_constraints* constraints, int32_t* trajectory_result,
                                                     int32_t* first_failing_segment, int32_t* segment_result,
                                                     double* segment_bounds, int32_t* segment_sections) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !constraints || !trajectory_result)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "recursive input feasibility: coeffs, times, constraints and trajectory_result are required");
  RecParams P;
  if (mtg_feasibility_limits(constraints, &P.lim) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  if (n_coeffs < mtgf::kMinCoeffs || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "recursive input feasibility: n_coeffs must be in [5,12]");
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, P.lim) || n_segments >= (1 << 22))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "recursive input feasibility: n_segments, dimension >= 1, batch >= 0, times strides >= 1 that do not "
                                      "overlap ([B][K] or [K][B]), min_section_time_s and gravity not NaN");
  if (reinterpret_cast<uintptr_t>(segment_bounds) & 15)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "recursive input feasibility: segment_bounds must be 16-byte aligned");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.traj_word = trajectory_result; P.first_failing = first_failing_segment; P.seg_result = segment_result; P.seg_bounds = segment_bounds;
  P.seg_sections = segment_sections;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<int>, per_traj, dim3(256), 0, stream, P.traj_word, nullptr, 0, P.s.B);   // (no second word)
  mtgs::with_instance<6>(n_coeffs, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    const size_t lds = (size_t)kThreads * (mtgr::scratch_len(NC) + mtgr::store_len(NC)) * sizeof(double);
    hipLaunchKernelGGL(mtg_recursive_seg_kernel<NC>, mtgs::grid_for(P.s.B * P.s.K, kThreads), dim3(kThreads), lds, stream, P);
  });
  hipLaunchKernelGGL(mtg_recursive_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
