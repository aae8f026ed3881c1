// mtg_field.hip -- batched distance-field clearance check: for a batch of solved trajectories (coeffs [B][K][D][N] as written by
// mtg_solve_linear) and a voxel grid of float distances (an ESDF), which trajectories are collision-free at every sample, where
// the others fail first, and the minimum clearance -> mtg_check_distance_field.  The rules (samples, lookup, fold) live in
// mtg_field_lane.h.  Mapping: G lanes share one (trajectory, segment) of the frame of mtg_segment_kernel.h; lane g takes samples
// g, g + G, ..: lanes that share a segment look up neighbouring voxels.  Each lane keeps the three position polynomials in
// registers, folds its samples into (order key of the clearance, sample index) and the smallest failing index, the G partial
// folds are combined with cross-lane exchanges (the fold is a minimum: the result does not depend on G), and lane 0 of the group
// writes the segment's outputs and does the trajectory's two atomic minima: failure_word(segment, 0) and the order key.  A lane
// per trajectory then decodes both words in place.  No LDS, no workspace; the grid is read with plain global loads.
#include "mtg_field_lane.h"
#include "mtg_segment_kernel.h"

extern "C" int mtg_context_field_lanes(const mtg_context* ctx);   // measurement knob "field_lanes" (mtg_hip_lab.h): 0 default

namespace {

constexpr int kThreads = 64;      // one wavefront per workgroup, as in the other per-segment checks
constexpr int kDefaultLanes = 64; // G of the shipped form: the whole wavefront on one segment (DESIGN.md 4.14 has the measurement)
using mtgs::kNoFailure;

struct FieldParams {
  mtgs::SegShape s;
  mtgf::Grid g;
  double dt, inflation;
  int max_samples;
  int* traj_word;            // [B]: kNoFailure, or min over the failing segments of failure_word(segment, 0); decoded in place to 1 / 0
  int* first_segment;        // [B] or null
  double* seg_clearance;     // [B][K] or null
  int* seg_closest;          // [B][K] or null
  int* seg_first_failing;    // [B][K] or null
  int* seg_samples;          // [B][K] or null
  double* traj_clearance;    // [B] or null: holds the order-mapped minimum between init and decode
};

template <int NC, int G>
__global__ __launch_bounds__(kThreads) void mtg_field_seg_kernel(FieldParams P) {
  static_assert(G >= 1 && G <= kThreads && (G & (G - 1)) == 0, "G: a power of two within the wavefront");
  const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
  const mtgs::SegLane L = mtgs::seg_lane(P.s, lane / G);   // (the G lanes of a group are in range together)
  if (!L.in_range) return;
  const int g = (int)(threadIdx.x % G);
  double p[3][NC];
  mtgs::load_padded<NC, 3>(L.c, P.s.N, P.s.D, p);
  const int S = mtgf::sample_count(L.T, P.dt, P.max_samples);
  mtgf::Fold f;
  mtgf::fold_samples<NC>(p, L.T, P.dt, S, g, G, P.g, P.inflation, f);
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1)
    mtgf::combine(f, __shfl_xor(f.key, off), __shfl_xor(f.sample, off), __shfl_xor(f.failing, off));
  if (g != 0) return;
  const mtgf::SegmentResult r = mtgf::segment_result(f, S);
  if (P.seg_clearance) P.seg_clearance[L.idx] = r.clearance;
  if (P.seg_closest) P.seg_closest[L.idx] = r.closest;
  if (P.seg_first_failing) P.seg_first_failing[L.idx] = r.first_failing;
  if (P.seg_samples) P.seg_samples[L.idx] = r.samples;
  if (P.traj_clearance) atomicMin(reinterpret_cast<unsigned long long*>(P.traj_clearance) + L.b, mtgs::order_key(r.clearance));
  if (r.fails) atomicMin(P.traj_word + L.b, mtgs::failure_word(L.seg, 0));
}

__global__ void mtg_field_traj_kernel(FieldParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == kNoFailure ? 1 : 0;
  if (P.first_segment) P.first_segment[b] = w == kNoFailure ? -1 : mtgs::failure_segment(w);
  if (P.traj_clearance) P.traj_clearance[b] = mtgs::order_value(reinterpret_cast<unsigned long long*>(P.traj_clearance)[b]);
}

template <int G>
void launch_seg(const FieldParams& P, hipStream_t stream) {
  mtgs::with_instance<mtgf::kMinInstance>(P.s.N, [&](auto nc) {
    hipLaunchKernelGGL((mtg_field_seg_kernel<decltype(nc)::value, G>), mtgs::grid_for(P.s.B * P.s.K * G, kThreads), dim3(kThreads), 0,
                       stream, P);
  });
}

}  // namespace

extern "C" int mtg_check_distance_field(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                        const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                        const mtg_distance_field* field, double dt, int32_t max_samples, double inflation,
                                        int32_t* trajectory_feasible, int32_t* first_failing_segment, double* segment_clearance,
                                        int32_t* segment_closest_sample, int32_t* segment_first_failing_sample,
                                        int32_t* segment_samples, double* trajectory_clearance) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !field || !field->distances || !trajectory_feasible)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "distance field: coeffs, times, field, field->distances and trajectory_feasible are required");
  FieldParams P;
  if (!mtgf::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, dt, max_samples, inflation, &P.g))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "distance field: 1 <= n_coeffs <= 12, 1 <= n_segments < 2^19, dimension 3 or 4, batch >= 0, times "
                                      "strides >= 1 that do not overlap; nx, ny, nz >= 2 (nearest: 1) with at most 2^31 - 1 voxels; "
                                      "voxel_size > 0, origin and inflation >= 0 finite; outside_distance not NaN; interpolation 0 or 1; "
                                      "dt > 0 finite; max_samples in [2, 2^20]");
  int lanes = mtg_context_field_lanes(ctx);
  if (lanes != 1 && lanes != 4 && lanes != 16 && lanes != 64) lanes = kDefaultLanes;
  if ((long long)batch * n_segments > 0x7fffffffll * (kThreads / lanes))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "distance field: batch x n_segments is beyond one launch");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.dt = dt; P.inflation = inflation; P.max_samples = max_samples;
  P.traj_word = trajectory_feasible; P.first_segment = first_failing_segment; P.seg_clearance = segment_clearance;
  P.seg_closest = segment_closest_sample; P.seg_first_failing = segment_first_failing_sample; P.seg_samples = segment_samples;
  P.traj_clearance = trajectory_clearance;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<unsigned long long>, per_traj, dim3(256), 0, stream, P.traj_word,
                     reinterpret_cast<unsigned long long*>(P.traj_clearance), mtgs::kKeyInfinity, P.s.B);
  if (lanes == 1) launch_seg<1>(P, stream);
  else if (lanes == 4) launch_seg<4>(P, stream);
  else if (lanes == 16) launch_seg<16>(P, stream);
  else launch_seg<64>(P, stream);
  hipLaunchKernelGGL(mtg_field_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
