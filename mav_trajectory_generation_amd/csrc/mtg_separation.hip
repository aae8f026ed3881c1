// mtg_separation.hip -- batched trajectory-to-trajectory separation check: for a list of pairs (trajectory a of batch A,
// trajectory b of batch B; coeffs [B][K][D][N] as written by mtg_solve_linear, each side with its own segment count, times
// and start times), which pairs keep min_separation between their centres, where the others first come too close, and the
// exact minimum distance -> mtg_check_trajectory_separation.  The per-lane algorithm lives in mtg_separation_lane.h on top of the
// root isolation of mtg_extrema_lane.h.  Mapping: one lane per (pair, segment of A); the lane walks the segments of B that overlap
// its own in time order, owns the per-(pair, segment) outputs and prunes against its own running minimum.  Per lane in LDS,
// [slot][lane] layout: the two root buffers of degree 2 N - 3 and the 3 x N coefficients of the piece's difference curve, which
// are written once per piece and read where g is formed and where the candidates are evaluated (registers hold g and the
// search).  A failing lane reports ((i + j) << 10 | j) with an atomic minimum on its pair's word; the pair's separation is an
// atomic minimum on the order-mapped bits of the double, NaN below every number; a lane per pair then decodes both words in
// place and, when asked, scans the pair's Ka segment entries for the closest time and segment pair.
#include "mtg_separation_lane.h"
#include "mtg_segment_kernel.h"

namespace {

constexpr int kThreads = 64;   // one wavefront per workgroup, as in mtg_obstacle.hip: 39 KB of LDS at N = 12
using mtgs::kNoFailure;
using mtgs::kKeyInfinity;
using mtgs::order_key;
using mtgs::order_value;

struct SepSide {
  const double* coeffs;   // [B][K][D][N]
  const double* times;    // times[b * ts_b + k * ts_k]
  const double* start;    // [B] or null: 0
  long long ts_b, ts_k, B;
  int K;
};

struct SepParams {
  SepSide a, b;
  const int* pairs;        // [P][2]
  long long P;
  int N, D;
  double min_separation;
  int* pair_word;          // [P]: kNoFailure, kInvalidPair or the smallest failing piece word; decoded in place to 1 / 0
  int* first_a;            // [P] or null
  int* first_b;            // [P] or null
  double* pair_separation; // [P] or null: holds the order-mapped minimum between init and decode
  double* pair_time;       // [P] or null
  int* pair_a;             // [P] or null
  int* pair_b;             // [P] or null
  double* seg_separation;  // [P][Ka] or null
  double* seg_time;        // [P][Ka] or null
  int* seg_b;              // [P][Ka] or null
  int* seg_pieces;         // [P][Ka] or null
};

// the trajectory `index` of a side, or false: nothing of the side is read for an index out of range
__device__ __forceinline__ bool side_of(const SepSide& S, int index, int N, int D, mtgp::Side& out) {
  if (index < 0 || (long long)index >= S.B) return false;
  out.c = S.coeffs + (long long)index * S.K * (long long)(D * N);
  out.t = S.times + (long long)index * S.ts_b;
  out.ts_k = S.ts_k;
  out.K = S.K;
  out.start = S.start ? S.start[index] : 0.0;
  return true;
}

template <int NC>
__global__ __launch_bounds__(kThreads) void mtg_separation_seg_kernel(SepParams P) {
  __shared__ double lds[mtgp::buffer_len(NC) * kThreads];
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= P.P * P.a.K) return;
  const long long p = idx / P.a.K;
  const int i = (int)(idx - p * P.a.K);
  mtgp::Side A, B;
  mtgp::Fold f;
  const bool in_a = side_of(P.a, P.pairs[2 * p], P.N, P.D, A), in_b = side_of(P.b, P.pairs[2 * p + 1], P.N, P.D, B);
  if (in_a && in_b) {
    mtgs::LdsColumn<kThreads> buf{lds + threadIdx.x};
    mtgp::lane_check<NC, mtgs::LdsColumn<kThreads>>(A, B, i, P.N, P.D, P.min_separation, true, buf, f);
  } else {
    mtgp::fold_invalid(f);
  }
  if (P.seg_separation) P.seg_separation[idx] = f.separation;
  if (P.seg_time) P.seg_time[idx] = f.time;
  if (P.seg_b) P.seg_b[idx] = f.segment_b;
  if (P.seg_pieces) P.seg_pieces[idx] = f.pieces;
  if (P.pair_separation) atomicMin(reinterpret_cast<unsigned long long*>(P.pair_separation) + p, order_key(f.separation));
  if (f.invalid) atomicMin(P.pair_word + p, mtgp::kInvalidPair);
  else if (f.failing_b >= 0) atomicMin(P.pair_word + p, mtgp::piece_word(f.failing_a, f.failing_b));
}

__global__ void mtg_separation_pair_kernel(SepParams P) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.P) return;
  const int w = P.pair_word[p];
  const bool none = w == kNoFailure, invalid = w == mtgp::kInvalidPair;
  P.pair_word[p] = none ? 1 : 0;
  if (P.first_a) P.first_a[p] = none || invalid ? -1 : mtgp::piece_segment_a(w);
  if (P.first_b) P.first_b[p] = none || invalid ? -1 : mtgp::piece_segment_b(w);
  if (P.pair_separation) P.pair_separation[p] = order_value(reinterpret_cast<unsigned long long*>(P.pair_separation)[p]);
  if (P.pair_time || P.pair_a || P.pair_b) {   // (the entry point has made sure of the three segment arrays)
    mtgp::Fold f;
    mtgp::fold_init(f);
    if (!invalid)
      for (int i = 0; i < P.a.K; ++i) mtgp::fold_minimum(f, i, P.seg_b[p * P.a.K + i], P.seg_separation[p * P.a.K + i], P.seg_time[p * P.a.K + i]);
    if (P.pair_time) P.pair_time[p] = f.time;
    if (P.pair_a) P.pair_a[p] = f.segment_a;
    if (P.pair_b) P.pair_b[p] = f.segment_b;
  }
}

}  // namespace

extern "C" int mtg_check_trajectory_separation(mtg_context* ctx, int32_t n_coeffs, int32_t dimension, int32_t n_segments_a, int64_t batch_a,
                                               const double* coeffs_a, const double* times_a, int64_t times_a_stride_b,
                                               int64_t times_a_stride_k, const double* start_a, int32_t n_segments_b, int64_t batch_b,
                                               const double* coeffs_b, const double* times_b, int64_t times_b_stride_b,
                                               int64_t times_b_stride_k, const double* start_b, int64_t n_pairs, const int32_t* pairs,
                                               double min_separation, int32_t* pair_feasible, int32_t* first_failing_segment_a,
                                               int32_t* first_failing_segment_b, double* pair_separation, double* pair_closest_time,
                                               int32_t* pair_closest_segment_a, int32_t* pair_closest_segment_b,
                                               double* segment_separation, double* segment_closest_time,
                                               int32_t* segment_closest_segment_b, int32_t* segment_pieces) {
  // (the argument checks come first and need no context: mtg_context_set_last_error records nothing without one)
  if (!coeffs_a || !times_a || !coeffs_b || !times_b || !pairs || !pair_feasible)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "trajectory separation: coeffs and times of both sides, pairs and pair_feasible are required");
  if (n_coeffs < 1 || n_coeffs > MTG_MAX_N)
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "trajectory separation: n_coeffs must be in [1,12]");
  if (!(min_separation >= 0.0) || !(min_separation <= DBL_MAX))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT, "trajectory separation: min_separation must be >= 0 and finite");
  if (!mtgp::arguments_ok(n_coeffs, dimension, n_segments_a, batch_a, times_a_stride_b, times_a_stride_k, n_segments_b, batch_b,
                          times_b_stride_b, times_b_stride_k, n_pairs, min_separation))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "trajectory separation: per side 1 <= n_segments <= 1024, dimension 3 or 4, batch >= 0, times strides >= 1 "
                                      "that do not overlap ([B][K] or [K][B]); 0 <= n_pairs, n_pairs * n_segments_a < 2^31");
  if (!mtgp::outputs_ok(pair_closest_time, pair_closest_segment_a, pair_closest_segment_b, segment_separation, segment_closest_time,
                        segment_closest_segment_b))
    return mtg_context_set_last_error(ctx, MTG_ERR_INVALID_ARGUMENT,
                                      "trajectory separation: the pair_closest outputs need segment_separation, segment_closest_time and "
                                      "segment_closest_segment_b");
  if (n_pairs == 0) return MTG_OK;
  if (!ctx) return MTG_ERR_INVALID_ARGUMENT;
  hipStream_t stream;
  const int rc = mtgs::entry_stream(ctx, &stream);
  if (rc != MTG_OK) return rc;
  SepParams P;
  P.a = {coeffs_a, times_a, start_a, times_a_stride_b, times_a_stride_k, batch_a, n_segments_a};
  P.b = {coeffs_b, times_b, start_b, times_b_stride_b, times_b_stride_k, batch_b, n_segments_b};
  P.pairs = pairs; P.P = n_pairs; P.N = n_coeffs; P.D = dimension; P.min_separation = min_separation;
  P.pair_word = pair_feasible; P.first_a = first_failing_segment_a; P.first_b = first_failing_segment_b;
  P.pair_separation = pair_separation; P.pair_time = pair_closest_time; P.pair_a = pair_closest_segment_a; P.pair_b = pair_closest_segment_b;
  P.seg_separation = segment_separation; P.seg_time = segment_closest_time; P.seg_b = segment_closest_segment_b;
  P.seg_pieces = segment_pieces;
  const dim3 per_pair = mtgs::grid_for(n_pairs, 256);
  hipLaunchKernelGGL(mtgs::first_failure_init_kernel<unsigned long long>, per_pair, dim3(256), 0, stream, P.pair_word,
                     reinterpret_cast<unsigned long long*>(P.pair_separation), kKeyInfinity, P.P);
  mtgs::with_instance<mtgp::kMinInstance>(n_coeffs, [&](auto nc) {
    hipLaunchKernelGGL((mtg_separation_seg_kernel<decltype(nc)::value>), mtgs::grid_for(P.P * P.a.K, kThreads), dim3(kThreads), 0, stream, P);
  });
  hipLaunchKernelGGL(mtg_separation_pair_kernel, per_pair, dim3(256), 0, stream, P);
  return hipGetLastError() == hipSuccess ? MTG_OK : MTG_ERR_DEVICE;
}
