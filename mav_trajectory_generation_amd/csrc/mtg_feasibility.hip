// mtg_feasibility.hip -- batched analytic input-feasibility check (FeasibilityAnalytic of mav_trajectory_generation_ros).
//
// For a batch of solved trajectories (coeffs [B][K][D][N] as written by mtg_solve_linear): which of them can the vehicle fly
// under up to six input limits -> mtg_check_input_feasibility.  The per-lane algorithm lives in mtg_feasibility_lane.h on top
// of the root isolation of mtg_extrema_lane.h.  Mapping: one lane per (trajectory, segment); the lane reads its D x N
// coefficients once and runs the thrust, velocity, yaw and jerk searches on them one after the other, so the searches share
// the two LDS root buffers ([slot][lane] layout, as in mtg_extrema.hip); the thrust and jerk candidate lists stay in LDS next
// to them for the roll/pitch sections.  A failing lane reports (segment << 8 | code) with an atomic minimum on its
// trajectory's word: the smallest word is the first failing segment in SEGMENT order, whichever lane finishes first; a lane
// per trajectory then decodes the words.
#include <hip/hip_runtime.h>

#include "../../include/mtg_hip.h"
#include "mtg_feasibility_lane.h"

namespace {

constexpr int kThreads = 64;   // roots + candidates per lane: 78 doubles at N = 10 (39 KB per workgroup), 102 at N = 12 (51 KB)
constexpr int kNoFailure = 0x7fffffff;

struct FeasParams {
  const double* coeffs;   // [B][K][D][N]
  const double* times;    // times[b*ts_b + k*ts_k]
  long long ts_b, ts_k;
  int* traj_word;         // [B]: kNoFailure, or min over failing segments of (segment << 8 | code); decoded in place
  int* first_failing;     // [B] or null
  int* seg_result;        // [B][K] or null
  double* seg_bounds;     // [B][K][6] or null
  long long B;
  int N, K, D;
  mtgf::Limits lim;
};

struct LdsColumn {
  double* p;   // element i at p[i * kThreads]
  __device__ double& operator[](int i) { return p[i * kThreads]; }
};

__global__ void mtg_feasibility_init_kernel(FeasParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < P.B) P.traj_word[b] = kNoFailure;
}

template <int NC>
__global__ __launch_bounds__(kThreads) void mtg_feasibility_seg_kernel(FeasParams P) {
  extern __shared__ double lds[];
  const long long total = P.B * P.K;
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const long long b = idx / P.K;
  const int seg = (int)(idx - b * P.K);
  const double T = P.times[b * P.ts_b + (long long)seg * P.ts_k];
  LdsColumn roots{lds + threadIdx.x};
  LdsColumn cand{lds + (size_t)mtgf::roots_len(NC) * kThreads + threadIdx.x};
  LdsColumn cand_jerk{lds + (size_t)(mtgf::roots_len(NC) + mtgf::cand_thrust_len(NC)) * kThreads + threadIdx.x};
  double bounds[mtgf::kNumBounds];
  const int verdict = mtgf::segment_check<NC, LdsColumn, LdsColumn>(P.coeffs + idx * (long long)(P.D * P.N), P.N, P.D, T, P.lim,
                                                                    roots, cand, cand_jerk, bounds);
  if (P.seg_result) P.seg_result[idx] = verdict;
  if (P.seg_bounds) {
    double2* o = reinterpret_cast<double2*>(P.seg_bounds + idx * mtgf::kNumBounds);   // (48 B per segment: 16-byte aligned rows)
    o[0] = make_double2(bounds[0], bounds[1]);
    o[1] = make_double2(bounds[2], bounds[3]);
    o[2] = make_double2(bounds[4], bounds[5]);
  }
  if (verdict != mtgf::kFeasible) atomicMin(P.traj_word + b, (seg << 8) | verdict);
}

// FeasibilityBase::checkInputFeasibilityTrajectory (feasibility_base.cpp:97-107): the first segment that is not feasible
__global__ void mtg_feasibility_traj_kernel(FeasParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == kNoFailure ? mtgf::kFeasible : (w & 0xff);
  if (P.first_failing) P.first_failing[b] = w == kNoFailure ? -1 : (w >> 8);
}

template <int NC>
void launch_seg(const FeasParams& P, hipStream_t stream) {
  const long long total = P.B * P.K;
  const size_t lds = (size_t)kThreads * (mtgf::roots_len(NC) + mtgf::cand_thrust_len(NC) + mtgf::cand_jerk_len(NC)) * sizeof(double);
  hipLaunchKernelGGL(mtg_feasibility_seg_kernel<NC>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), lds, stream, P);
}

}  // namespace

extern "C" int mtg_context_stream_device(mtg_context* ctx, void** stream, int* device);
extern "C" int mtg_context_set_last_error(mtg_context* ctx, int code, const char* message);   // mtg_abi.hip
extern "C" int mtg_feasibility_limits(const mtg_input_constraints* in, mtgf::Limits* out);   // mtg_feasibility_host.cpp

extern "C" int mtg_check_input_feasibility(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension,
                                           int64_t batch, const double* coeffs, const double* times, int64_t times_stride_b,
                                           int64_t times_stride_k, const mtg_input_constraints* constraints,
                                           int32_t* trajectory_result, int32_t* first_failing_segment, int32_t* segment_result,
                                           double* segment_bounds) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !constraints || !trajectory_result)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "input feasibility: coeffs, times, constraints and trajectory_result are required");
  FeasParams P;
  if (mtg_feasibility_limits(constraints, &P.lim) != MTG_OK) return MTG_ERR_INVALID_ARGUMENT;
  if (n_coeffs < mtgf::kMinCoeffs || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "input feasibility: n_coeffs must be in [5,12]");
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, P.lim) || n_segments >= (1 << 22))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "input feasibility: n_segments, dimension >= 1, batch >= 0, times strides >= 1 that do not overlap "
                                      "([B][K] or [K][B]), min_section_time_s and gravity not NaN");
  if (reinterpret_cast<uintptr_t>(segment_bounds) & 15)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "input feasibility: segment_bounds must be 16-byte aligned");
  if (batch == 0) return MTG_OK;
  void* stream = nullptr;
  int device = 0;
  int rc = mtg_context_stream_device(ctx, &stream, &device);
  if (rc != MTG_OK) return rc;
  if (hipSetDevice(device) != hipSuccess) return MTG_ERR_DEVICE;
  P.coeffs = coeffs; P.times = times; P.ts_b = times_stride_b; P.ts_k = times_stride_k;
  P.traj_word = trajectory_result; P.first_failing = first_failing_segment; P.seg_result = segment_result; P.seg_bounds = segment_bounds;
  P.B = batch; P.N = n_coeffs; P.K = n_segments; P.D = dimension;
  const dim3 per_traj((unsigned)((batch + 255) / 256));
  hipLaunchKernelGGL(mtg_feasibility_init_kernel, per_traj, dim3(256), 0, (hipStream_t)stream, P);
  // (an odd N runs in the next even instantiation on zero-padded coefficients)
  if (n_coeffs <= 6) launch_seg<6>(P, (hipStream_t)stream);
  else if (n_coeffs <= 8) launch_seg<8>(P, (hipStream_t)stream);
  else if (n_coeffs <= 10) launch_seg<10>(P, (hipStream_t)stream);
  else launch_seg<12>(P, (hipStream_t)stream);
  hipLaunchKernelGGL(mtg_feasibility_traj_kernel, per_traj, dim3(256), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
