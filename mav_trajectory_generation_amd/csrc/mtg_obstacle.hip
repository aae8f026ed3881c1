// mtg_obstacle.hip -- batched sphere-obstacle clearance check: for a batch of solved trajectories (coeffs [B][K][D][N] as
// written by mtg_solve_linear) and a set of spheres, which trajectories stay clear, where the others hit first, and the exact
// minimum clearance -> mtg_check_obstacle_clearance.  The per-lane algorithm lives in mtg_obstacle_lane.h on top of the root
// isolation of mtg_extrema_lane.h.  Mapping: one lane per (trajectory, segment) in the frame of mtg_segment_kernel.h; the lane
// reads the 3 x N position coefficients once, forms the convolution and its four bounding boxes once and walks ITS OWN surviving
// obstacles, nearest bound first (two LDS root buffers of degree 2 N - 3 and the convolution behind them, [slot][lane] layout).  Nothing is staged: the
// selection scan reads obstacle m in every lane at once (scalar loads where the set is shared, one cache line per
// trajectory otherwise) and the selected sphere stays in registers.  A failing lane reports (segment << 12 | obstacle) with
// an atomic minimum on its trajectory's word; the trajectory's clearance is an atomic minimum on the order-mapped bits of the
// double, with NaN mapped below every number; a lane per trajectory then decodes both words in place.
#include "mtg_obstacle_lane.h"
#include "mtg_segment_kernel.h"

namespace {

// One wavefront per workgroup, as in mtg_halfplane.hip.  Per lane in LDS: the root buffers, 2 (2 N - 3) doubles, and the
// convolution, 2 N - 2 -- 32 KB per workgroup at N = 12 (registers: it would not fit beside a search of degree 21 without scratch).
constexpr int kThreads = 64;
using mtgs::kNoFailure;

struct ObParams {
  mtgs::SegShape s;
  const double* obstacles;   // obstacles + b * os_b: n_obstacles x (cx, cy, cz, r)
  long long os_b;
  double inflation;
  int* traj_word;            // [B]: kNoFailure, or min over failing pairs of (segment << 12 | obstacle); decoded in place to 1 / 0
  int* first_segment;        // [B] or null
  int* first_obstacle;       // [B] or null
  double* seg_clearance;     // [B][K] or null
  int* seg_nearest;          // [B][K] or null
  double* seg_time;          // [B][K] or null
  double* traj_clearance;    // [B] or null: holds the order-mapped minimum between init and decode
  int n_obstacles;
};

using mtgs::kKeyInfinity;
using mtgs::order_key;
using mtgs::order_value;

// SHARED: one obstacle set for every lane (stride 0) -- the set's address is a kernel argument and the scan's loads are scalar.
template <int NC, bool SHARED>
__global__ __launch_bounds__(kThreads) void mtg_obstacle_seg_kernel(ObParams P) {
  __shared__ double lds[mtgo::buffer_len(NC) * kThreads];
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x * kThreads + threadIdx.x);
  if (!L.in_range) return;
  const double* obstacles = SHARED ? P.obstacles : P.obstacles + L.b * P.os_b;
  mtgs::LdsColumn<kThreads> roots{lds + threadIdx.x};
  mtgo::Fold f;
  mtgo::segment_check<NC, mtgs::LdsColumn<kThreads>>(L.c, P.s.N, P.s.D, L.T, obstacles, P.n_obstacles, P.inflation, roots, f);
  if (P.seg_clearance) P.seg_clearance[L.idx] = f.clearance;
  if (P.seg_nearest) P.seg_nearest[L.idx] = f.nearest;
  if (P.seg_time) P.seg_time[L.idx] = f.time;
  if (P.traj_clearance) atomicMin(reinterpret_cast<unsigned long long*>(P.traj_clearance) + L.b, order_key(f.clearance));
  if (f.failing < mtgo::kMaxObstacles) atomicMin(P.traj_word + L.b, mtgo::failure_word(L.seg, f.failing));
}

__global__ void mtg_obstacle_traj_kernel(ObParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == kNoFailure ? 1 : 0;
  if (P.first_segment) P.first_segment[b] = w == kNoFailure ? -1 : mtgo::failure_segment(w);
  if (P.first_obstacle) P.first_obstacle[b] = w == kNoFailure ? -1 : mtgo::failure_obstacle(w);
  if (P.traj_clearance) P.traj_clearance[b] = order_value(reinterpret_cast<unsigned long long*>(P.traj_clearance)[b]);
}

}  // namespace

extern "C" int mtg_check_obstacle_clearance(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                            const double* coeffs, const double* times, int64_t times_stride_b,
                                            int64_t times_stride_k, const double* obstacles, int32_t n_obstacles,
                                            int64_t obstacles_stride_b, double inflation, int32_t* trajectory_feasible,
                                            int32_t* first_failing_segment, int32_t* first_failing_obstacle,
                                            double* segment_clearance, int32_t* segment_nearest_obstacle,
                                            double* segment_closest_time, double* trajectory_clearance) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !obstacles || !trajectory_feasible)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "obstacle clearance: coeffs, times, obstacles and trajectory_feasible are required");
  if (n_coeffs < 1 || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "obstacle clearance: n_coeffs must be in [1,12]");
  if (n_obstacles < 1 || n_obstacles > mtgo::kMaxObstacles || obstacles_stride_b < 0)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "obstacle clearance: n_obstacles must be in [1,4096] and the obstacle stride >= 0");
  if (!(inflation >= 0.0) || !(inflation <= DBL_MAX))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "obstacle clearance: inflation must be >= 0 and finite");
  if (!mtgo::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_obstacles, obstacles_stride_b, inflation))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "obstacle clearance: 1 <= n_segments < 2^19, dimension 3 or 4, batch >= 0, times strides >= 1 that do "
                                      "not overlap ([B][K] or [K][B])");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  ObParams P;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.obstacles = obstacles; P.os_b = obstacles_stride_b; P.inflation = inflation; P.n_obstacles = n_obstacles;
  P.traj_word = trajectory_feasible; P.first_segment = first_failing_segment; P.first_obstacle = first_failing_obstacle;
  P.seg_clearance = segment_clearance; P.seg_nearest = segment_nearest_obstacle; P.seg_time = segment_closest_time;
  P.traj_clearance = trajectory_clearance;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<unsigned long long>, per_traj, dim3(256), 0, stream, P.traj_word,
                     reinterpret_cast<unsigned long long*>(P.traj_clearance), kKeyInfinity, P.s.B);
  mtgs::with_instance<mtgo::kMinInstance>(n_coeffs, [&](auto nc) {
    const dim3 grid = mtgs::grid_for(P.s.B * P.s.K, kThreads);
    if (P.os_b == 0) hipLaunchKernelGGL((mtg_obstacle_seg_kernel<decltype(nc)::value, true>), grid, dim3(kThreads), 0, stream, P);
    else hipLaunchKernelGGL((mtg_obstacle_seg_kernel<decltype(nc)::value, false>), grid, dim3(kThreads), 0, stream, P);
  });
  hipLaunchKernelGGL(mtg_obstacle_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
