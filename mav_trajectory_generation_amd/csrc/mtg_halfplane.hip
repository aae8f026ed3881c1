// mtg_halfplane.hip -- batched half-plane / flight-corridor feasibility check (FeasibilityBase::checkHalfPlaneFeasibility of
// mav_trajectory_generation_ros).
//
// For a batch of solved trajectories (coeffs [B][K][D][N] as written by mtg_solve_linear): which of them stay on the inner side
// of every plane of a set -> mtg_check_half_plane_feasibility.  The per-lane algorithm lives in mtg_halfplane_lane.h on top of
// the root isolation of mtg_extrema_lane.h.  Mapping: one lane per (trajectory, segment); the lane reads the 3 x N position
// coefficients once and walks its plane set, one root search of degree N - 2 per plane direction (two LDS root buffers,
// [slot][lane] layout as in mtg_extrema.hip).  A failing lane reports (segment << 8 | plane) with an atomic minimum on its
// trajectory's word: the smallest word is the first failing segment in SEGMENT order and, within it, the first failing plane
// in LIST order -- the reference's two loops -- whichever lane finishes first.  The trajectory's clearance is an atomic
// minimum too, on the ORDER-MAPPED bits of the double (sign bit flipped for positive values, all bits for negative ones:
// unsigned order = numeric order), so no scratch and no floating-point atomic on a signed value; a lane per trajectory then
// decodes both words in place.
#include "mtg_halfplane_lane.h"
#include "mtg_segment_kernel.h"

namespace {

// One wavefront per workgroup: the lanes never synchronise, and 10k x 8 segments are 1250 wavefronts for 1024 SIMDs, so the
// smallest workgroup spreads them best.  Root buffers: 2 (N - 2) doubles per lane, 10 KB per workgroup at N = 12.
constexpr int kThreads = 64;
using mtgs::kNoFailure;

struct HpParams {
  mtgs::SegShape s;
  const double* planes;   // planes + b*ps_b + k*ps_k: n_planes x (nx, ny, nz, offset)
  long long ps_b, ps_k;
  int* traj_word;         // [B]: kNoFailure, or min over failing segments of (segment << 8 | plane); decoded in place to 1 / 0
  int* first_segment;     // [B] or null
  int* first_plane;       // [B] or null
  double* seg_clearance;  // [B][K] or null
  double* traj_clearance; // [B] or null: holds the order-mapped minimum between init and decode
  int n_planes;
};

__device__ unsigned long long order_key(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
constexpr unsigned long long kKeyInfinity = 0xfff0000000000000ull;   // order_key(+infinity): "no clearance yet"
__device__ double order_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// SHARED: one plane set for every lane (both strides 0) -- the set's address is a kernel argument, its loads are scalar and
// the reuse branch of the lane code is uniform by construction.
template <int NC, bool SHARED>
__global__ __launch_bounds__(kThreads) void mtg_halfplane_seg_kernel(HpParams P) {
  __shared__ double lds[mtgh::roots_len(NC) * kThreads];
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x * kThreads + threadIdx.x);
  if (!L.in_range) return;
  const double* planes = SHARED ? P.planes : P.planes + L.b * P.ps_b + (long long)L.seg * P.ps_k;
  mtgs::LdsColumn<kThreads> roots{lds + threadIdx.x};
  double clearance;
  const int plane = mtgh::segment_check<NC, mtgs::LdsColumn<kThreads>>(L.c, P.s.N, P.s.D, L.T, planes, P.n_planes, roots, clearance);
  if (P.seg_clearance) P.seg_clearance[L.idx] = clearance;
  if (P.traj_clearance && clearance == clearance)
    atomicMin(reinterpret_cast<unsigned long long*>(P.traj_clearance) + L.b, order_key(clearance));
  if (plane >= 0) mtgs::report_failure(P.traj_word + L.b, L.seg, plane);
}

// FeasibilityBase::checkHalfPlaneFeasibility(const Trajectory&) (feasibility_base.cpp:109-117): the first segment that fails
__global__ void mtg_halfplane_traj_kernel(HpParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  const int plane = mtgs::failure_code(w);
  P.traj_word[b] = w == kNoFailure ? 1 : 0;
  if (P.first_segment) P.first_segment[b] = w == kNoFailure ? -1 : mtgs::failure_segment(w);
  if (P.first_plane) P.first_plane[b] = (w == kNoFailure || plane == mtgh::kNoPlane) ? -1 : plane;
  if (P.traj_clearance) {
    const unsigned long long k = reinterpret_cast<unsigned long long*>(P.traj_clearance)[b];
    P.traj_clearance[b] = (w != kNoFailure && plane == mtgh::kNoPlane) ? NAN : order_value(k);
  }
}

}  // namespace

extern "C" int mtg_check_half_plane_feasibility(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension,
                                                int64_t batch, const double* coeffs, const double* times, int64_t times_stride_b,
                                                int64_t times_stride_k, const double* planes, int32_t n_planes,
                                                int64_t planes_stride_b, int64_t planes_stride_k, int32_t* trajectory_feasible,
                                                int32_t* first_failing_segment, int32_t* first_failing_plane,
                                                double* segment_clearance, double* trajectory_clearance) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !planes || !trajectory_feasible)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "half-plane feasibility: coeffs, times, planes and trajectory_feasible are required");
  if (n_coeffs < 1 || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "half-plane feasibility: n_coeffs must be in [1,12]");
  if (n_planes < 1 || n_planes > mtgh::kMaxPlanes || planes_stride_b < 0 || planes_stride_k < 0)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "half-plane feasibility: n_planes must be in [1,64] and the plane strides >= 0");
  if (!mtgh::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_planes, planes_stride_b, planes_stride_k))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "half-plane feasibility: 1 <= n_segments < 2^22, dimension >= 1, batch >= 0, times strides >= 1 that do "
                                      "not overlap ([B][K] or [K][B])");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  HpParams P;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.planes = planes; P.ps_b = planes_stride_b; P.ps_k = planes_stride_k; P.n_planes = n_planes;
  P.traj_word = trajectory_feasible; P.first_segment = first_failing_segment; P.first_plane = first_failing_plane;
  P.seg_clearance = segment_clearance; P.traj_clearance = trajectory_clearance;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<unsigned long long>, per_traj, dim3(256), 0, stream, P.traj_word,
                     reinterpret_cast<unsigned long long*>(P.traj_clearance), kKeyInfinity, P.s.B);
  mtgs::with_instance<mtgh::kMinInstance>(n_coeffs, [&](auto nc) {
    const dim3 grid = mtgs::grid_for(P.s.B * P.s.K, kThreads);
    if (P.ps_b == 0 && P.ps_k == 0) hipLaunchKernelGGL((mtg_halfplane_seg_kernel<decltype(nc)::value, true>), grid, dim3(kThreads), 0, stream, P);
    else hipLaunchKernelGGL((mtg_halfplane_seg_kernel<decltype(nc)::value, false>), grid, dim3(kThreads), 0, stream, P);
  });
  hipLaunchKernelGGL(mtg_halfplane_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
