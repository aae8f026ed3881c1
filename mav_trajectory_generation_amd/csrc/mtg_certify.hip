// mtg_certify.hip -- batched CERTIFIED distance-field check: for a batch of solved trajectories (coeffs [B][K][D][N] as written by
// mtg_solve_linear) and a trilinear voxel grid of float distances with a Lipschitz constant, a verdict for every instant of every
// segment and a guaranteed lower bound of the minimum clearance next to the sampled upper bound -> mtg_certify_distance_field.
// The rules (node, fold) live in mtg_certify_lane.h.  Mapping: one 64-lane workgroup (one wavefront) per (trajectory, segment)
// of the frame of mtg_segment_kernel.h.  The interval bisection runs level-synchronously: the frontier of a level is a list of
// node numbers j in LDS, ascending; the wave walks it in chunks of 64, each lane evaluates one node from the three position
// polynomials it keeps in registers, the survivors of a chunk are compacted in order with a ballot and a population count below
// the lane, and each survivor writes its two children into the other frontier.  Every lane of the workgroup shares the segment,
// so the level loop, the chunk loop and the barrier between two levels are wave-uniform.  The lanes' partial folds (minima, a
// flag) are combined with cross-lane exchanges; lane 0 writes the segment's outputs and does the trajectory's three atomic
// minima: failure_word(segment, code) and the two order keys.  A lane per trajectory then decodes the words in place.
// Two frontiers of 1024 ints: 8 KB of LDS per workgroup; no workspace.
#include "mtg_certify_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // one wavefront per workgroup and per segment
using mtgs::kNoFailure;

struct CertifyParams {
  mtgs::SegShape s;
  mtgf::Grid g;
  mtgc::Rule rule;
  int* traj_word;          // [B]: kNoFailure, or min over the segments that are not FREE of failure_word(segment, code); decoded in place
  int* first_segment;      // [B] or null
  int* seg_result;         // [B][K] or null
  double* seg_lower;       // [B][K] or null
  double* seg_sampled;     // [B][K] or null
  double* seg_closest_time;   // [B][K] or null
  double* seg_failing_time;   // [B][K] or null
  int* seg_nodes;          // [B][K] or null
  int* seg_depth;          // [B][K] or null
  double* traj_lower;      // [B] or null: holds the order-mapped minimum between init and decode
  double* traj_sampled;    // [B] or null: likewise
};

__global__ void mtg_certify_init_kernel(CertifyParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  P.traj_word[b] = kNoFailure;
  if (P.traj_lower) reinterpret_cast<unsigned long long*>(P.traj_lower)[b] = mtgs::kKeyInfinity;
  if (P.traj_sampled) reinterpret_cast<unsigned long long*>(P.traj_sampled)[b] = mtgs::kKeyInfinity;
}

template <int NC>
__global__ __launch_bounds__(kThreads) void mtg_certify_seg_kernel(CertifyParams P) {
  __shared__ int frontier[2][mtgc::kFrontier];
  const int lane = (int)threadIdx.x;
  const mtgs::SegLane L = mtgs::seg_lane(P.s, (long long)blockIdx.x);   // the grid holds B K workgroups exactly
  if (!L.in_range) return;                                               // (the whole workgroup, ahead of every barrier)
  double p[3][NC];
  mtgs::load_padded<NC, 3>(L.c, P.s.N, P.s.D, p);
  const double T = L.T;
  const bool lone = mtgc::lone_node(T);
  int count = lone ? 1 : 1 << P.rule.min_depth, nodes = 0, depth = lone ? 0 : P.rule.min_depth, cur = 0;
  for (int j = lane; j < count; j += kThreads) frontier[0][j] = j;       // count <= kFrontier
  __syncthreads();
  mtgc::Fold f;
  bool budget = false;
  for (;; ++depth) {                                                     // at most max_depth - min_depth + 1 levels, wave-uniform
    const double w = mtgc::half_width(T, depth);
    const bool last = lone || depth == P.rule.max_depth;
    int survivors = 0;                                                   // wave-uniform: it only grows by ballot counts
    for (int base = 0; base < count; base += kThreads) {
      const int i = base + lane;
      bool survives = false;
      int j = 0;
      if (i < count) {
        j = frontier[cur][i];
        const double m = mtgc::midpoint(T, j, w);
        survives = mtgc::fold_node(f, m, mtgc::evaluate_node<NC>(p, m, w, P.g, P.rule), last);
      }
      const unsigned long long mask = __ballot(survives);
      const int slot = survivors + __popcll(mask & ((1ull << lane) - 1ull));
      if (survives && 2 * slot + 1 < mtgc::kFrontier) {                  // (beyond the buffer the level ends with BUDGET)
        frontier[cur ^ 1][2 * slot] = 2 * j;
        frontier[cur ^ 1][2 * slot + 1] = 2 * j + 1;
      }
      survivors += __popcll(mask);
    }
    nodes += count;
    if (survivors == 0) break;
    if (2 * survivors > P.rule.max_frontier) { budget = true; break; }
    count = 2 * survivors;
    cur ^= 1;
    __syncthreads();                                                     // the children are written before the next level reads them
  }
#pragma unroll
  for (int off = kThreads / 2; off > 0; off >>= 1)
    mtgc::combine(f, __shfl_xor(f.c_key, off), __shfl_xor(f.c_time, off), __shfl_xor(f.failing_time, off), __shfl_xor(f.bound_key, off),
                  __shfl_xor(f.undecided, off));
  if (lane != 0) return;
  const mtgc::SegmentResult r = mtgc::segment_result(f, budget, nodes, depth);
  if (P.seg_result) P.seg_result[L.idx] = r.result;
  if (P.seg_lower) P.seg_lower[L.idx] = r.lower_bound;
  if (P.seg_sampled) P.seg_sampled[L.idx] = r.sampled;
  if (P.seg_closest_time) P.seg_closest_time[L.idx] = r.closest_time;
  if (P.seg_failing_time) P.seg_failing_time[L.idx] = r.first_failing_time;
  if (P.seg_nodes) P.seg_nodes[L.idx] = r.nodes;
  if (P.seg_depth) P.seg_depth[L.idx] = r.depth;
  if (P.traj_lower) atomicMin(reinterpret_cast<unsigned long long*>(P.traj_lower) + L.b, mtgs::order_key(r.lower_bound));
  if (P.traj_sampled) atomicMin(reinterpret_cast<unsigned long long*>(P.traj_sampled) + L.b, mtgs::order_key(r.sampled));
  if (r.result != MTG_FIELD_FREE) atomicMin(P.traj_word + L.b, mtgs::failure_word(L.seg, r.result));
}

__global__ void mtg_certify_traj_kernel(CertifyParams P) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.s.B) return;
  const int w = P.traj_word[b];
  P.traj_word[b] = w == kNoFailure ? (int)MTG_FIELD_FREE : mtgs::failure_code(w);
  if (P.first_segment) P.first_segment[b] = w == kNoFailure ? -1 : mtgs::failure_segment(w);
  if (P.traj_lower) P.traj_lower[b] = mtgs::order_value(reinterpret_cast<unsigned long long*>(P.traj_lower)[b]);
  if (P.traj_sampled) P.traj_sampled[b] = mtgs::order_value(reinterpret_cast<unsigned long long*>(P.traj_sampled)[b]);
}

}  // namespace

extern "C" int mtg_certify_distance_field(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                          const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                          const mtg_distance_field* field, double lipschitz, int32_t min_depth, int32_t max_depth,
                                          int32_t max_frontier, double inflation, int32_t* trajectory_result,
                                          int32_t* first_failing_segment, int32_t* segment_result, double* segment_lower_bound,
                                          double* segment_sampled_clearance, double* segment_closest_time,
                                          double* segment_first_failing_time, int32_t* segment_nodes, int32_t* segment_depth,
                                          double* trajectory_lower_bound, double* trajectory_sampled_clearance) {
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  if (!coeffs || !times || !field || !field->distances || !trajectory_result)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "certified distance field: coeffs, times, field, field->distances and trajectory_result are required");
  CertifyParams P;
  if (!mtgc::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, lipschitz, min_depth, max_depth,
                          max_frontier, inflation, &P.g))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "certified distance field: the shape and field rules of the sampled check with a trilinear field; "
                                      "lipschitz > 0 finite; min_depth in [0, 10]; max_depth in [min_depth, 24]; max_frontier in "
                                      "[max(2, 2^min_depth), 1024]");
  if ((long long)batch * n_segments > 0x7fffffffll)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "certified distance field: batch x n_segments is beyond one launch");
  if (batch == 0) return MTG_OK;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  P.s = {coeffs, times, times_stride_b, times_stride_k, batch, n_coeffs, n_segments, dimension};
  P.rule = {lipschitz, inflation, min_depth, max_depth, max_frontier};
  P.traj_word = trajectory_result; P.first_segment = first_failing_segment; P.seg_result = segment_result;
  P.seg_lower = segment_lower_bound; P.seg_sampled = segment_sampled_clearance; P.seg_closest_time = segment_closest_time;
  P.seg_failing_time = segment_first_failing_time; P.seg_nodes = segment_nodes; P.seg_depth = segment_depth;
  P.traj_lower = trajectory_lower_bound; P.traj_sampled = trajectory_sampled_clearance;
  const dim3 per_traj = mtgs::grid_for(batch, 256);
  hipLaunchKernelGGL(mtg_certify_init_kernel, per_traj, dim3(256), 0, stream, P);
  mtgs::with_instance<mtgf::kMinInstance>(n_coeffs, [&](auto nc) {
    hipLaunchKernelGGL((mtg_certify_seg_kernel<decltype(nc)::value>), dim3((unsigned)(batch * n_segments)), dim3(kThreads), 0, stream, P);
  });
  hipLaunchKernelGGL(mtg_certify_traj_kernel, per_traj, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
