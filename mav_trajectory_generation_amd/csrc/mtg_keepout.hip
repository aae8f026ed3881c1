// mtg_keepout.hip -- batched keep-out zone check: for a batch of solved trajectories (coeffs [B][K][D][N] as written by
// mtg_solve_linear) and a set of convex zones (each P half spaces: boxes, prisms), which trajectories stay outside every zone,
// where the others enter first, and the minimum clearance -> mtg_check_keep_out_zones.  The per-lane algorithm lives in
// mtg_keepout_lane.h on top of the root isolation of mtg_extrema_lane.h and the quarter boxes and pruning walk of
// mtg_obstacle_lane.h.  Mapping: one lane per (trajectory, segment) in the frame of mtg_segment_kernel.h; the lane forms its four
// bounding boxes once and walks ITS OWN surviving zones, nearest bound first (two LDS root buffers of degree N - 1, [slot][lane]
// layout).  Nothing is staged: the selection scan and the searches read zone m in every lane at once (scalar loads where the
// set is shared, cache lines per trajectory otherwise); a lane keeps the selected zone's index, not its planes.  A failing lane
// reports (segment << 12 | zone) with an atomic minimum on its trajectory's word; the trajectory's clearance is an atomic
// minimum on the order-mapped bits of the double, with NaN mapped below every number; a lane per trajectory then decodes both
// words in place.
#include "mtg_keepout_lane.h"
#include "mtg_segment_kernel.h"

namespace {

// One wavefront per workgroup, as in mtg_obstacle.hip.  Per lane in LDS: the root buffers, 2 (N - 1) doubles -- 11 KB per
// workgroup at N = 12.
constexpr int kThreads = 64;
using mtgs::kNoFailure;

struct KoParams {
  mtgs::SegShape s;
  const double* zones;       // zones + b * zs_b: n_zones x n_planes x (nx, ny, nz, offset)
  long long zs_b;
  double inflation;
  int* traj_word;            // [B]: kNoFailure, or min over failing pairs of (segment << 12 | zone); decoded in place to 1 / 0
  int* first_segment;        // [B] or null
  int* first_zone;           // [B] or null
  double* seg_clearance;     // [B][K] or null
  int* seg_nearest;          // [B][K] or null
  double* seg_time;          // [B][K] or null
  double* traj_clearance;    // [B] or null: holds the order-mapped minimum between init and decode
  int n_zones, n_planes;
};

// SHARED: one zone set for every lane (stride 0) -- the set's address is a kernel argument and the loads of planes are scalar.
template <int NC, bool SHARED>
__global__ __launch_bounds__(kThreads) void mtg_keepout_seg_kernel(KoParams P) {
  __shared__ double lds[mtgk::roots_len(NC) * kThreads];
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x * kThreads + threadIdx.x);
  if (!L.in_range) return;
  const double* zones = SHARED ? P.zones : P.zones + L.b * P.zs_b;
  mtgs::LdsColumn<kThreads> roots{lds + threadIdx.x};
  mtgk::Fold f;
  mtgk::segment_check<NC, mtgs::LdsColumn<kThreads>>(L.c, P.s.N, P.s.D, L.T, zones, P.n_zones, P.n_planes, P.inflation, roots, f);
  if (P.seg_clearance) P.seg_clearance[L.idx] = f.clearance;
  if (P.seg_nearest) P.seg_nearest[L.idx] = f.nearest;
  if (P.seg_time) P.seg_time[L.idx] = f.time;
  if (P.traj_clearance) atomicMin(reinterpret_cast<unsigned long long*>(P.traj_clearance) + L.b, mtgs::order_key(f.clearance));
  if (f.failing < mtgk::kMaxZones) atomicMin(P.traj_word + L.b, mtgo::failure_word(L.seg, f.failing));
}

__global__ void mtg_keepout_traj_kernel(KoParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == kNoFailure ? 1 : 0;
  if (P.first_segment) P.first_segment[b] = w == kNoFailure ? -1 : mtgo::failure_segment(w);
  if (P.first_zone) P.first_zone[b] = w == kNoFailure ? -1 : mtgo::failure_obstacle(w);
  if (P.traj_clearance) P.traj_clearance[b] = mtgs::order_value(reinterpret_cast<unsigned long long*>(P.traj_clearance)[b]);
}

}  // namespace

extern "C" int mtg_check_keep_out_zones(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                        const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                        const double* zones, int32_t n_zones, int32_t n_planes, int64_t zones_stride_b,
                                        double inflation, int32_t* trajectory_feasible, int32_t* first_failing_segment,
                                        int32_t* first_failing_zone, double* segment_clearance, int32_t* segment_nearest_zone,
                                        double* segment_closest_time, double* trajectory_clearance) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !zones || !trajectory_feasible)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "keep-out zones: coeffs, times, zones and trajectory_feasible are required");
  if (n_coeffs < 1 || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "keep-out zones: n_coeffs must be in [1,12]");
  if (n_zones < 1 || n_zones > mtgk::kMaxZones || zones_stride_b < 0)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "keep-out zones: n_zones must be in [1,4096] and the zone stride >= 0");
  if (n_planes < 1 || n_planes > mtgk::kMaxPlanes)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "keep-out zones: n_planes must be in [1,8]");
  if (!(inflation >= 0.0) || !(inflation <= DBL_MAX))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "keep-out zones: inflation must be >= 0 and finite");
  if (!mtgk::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_zones, n_planes, zones_stride_b, inflation))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "keep-out zones: 1 <= n_segments < 2^19, dimension 3 or 4, batch >= 0, times strides >= 1 that do "
                                      "not overlap ([B][K] or [K][B])");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  KoParams P;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.zones = zones; P.zs_b = zones_stride_b; P.inflation = inflation; P.n_zones = n_zones; P.n_planes = n_planes;
  P.traj_word = trajectory_feasible; P.first_segment = first_failing_segment; P.first_zone = first_failing_zone;
  P.seg_clearance = segment_clearance; P.seg_nearest = segment_nearest_zone; P.seg_time = segment_closest_time;
  P.traj_clearance = trajectory_clearance;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<unsigned long long>, per_traj, dim3(256), 0, stream, P.traj_word,
                     reinterpret_cast<unsigned long long*>(P.traj_clearance), mtgs::kKeyInfinity, P.s.B);
  mtgs::with_instance<mtgk::kMinInstance>(n_coeffs, [&](auto nc) {
    const dim3 grid = mtgs::grid_for(P.s.B * P.s.K, kThreads);
    if (P.zs_b == 0) hipLaunchKernelGGL((mtg_keepout_seg_kernel<decltype(nc)::value, true>), grid, dim3(kThreads), 0, stream, P);
    else hipLaunchKernelGGL((mtg_keepout_seg_kernel<decltype(nc)::value, false>), grid, dim3(kThreads), 0, stream, P);
  });
  hipLaunchKernelGGL(mtg_keepout_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
