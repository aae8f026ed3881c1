// mtg_certify_host.cpp -- host build (plain g++, no HIP) of the certified distance-field check: the lane code of
// mtg_certify_lane.h run one segment after the other, every level's nodes in ascending order, and the Lipschitz helper.  For
// one-trajectory-at-a-time callers and as the reproducible form of every rule in include/mtg_hip.h.  Touches no device.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_certify_lane.h"

namespace {

struct Outputs {
  int32_t *traj_result, *first_seg, *seg_result;
  double *seg_lower, *seg_sampled, *seg_closest_time, *seg_failing_time;
  int32_t *seg_nodes, *seg_depth;
  double *traj_lower, *traj_sampled;
};

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const mtgf::Grid& g,
         const mtgc::Rule& P, const Outputs& o) {
  int frontier[2][mtgc::kFrontier];
  for (int64_t b = 0; b < B; ++b) {
    int fseg = -1, code = MTG_FIELD_FREE;
    unsigned long long lower = mtgc::kKeyNone, sampled = mtgc::kKeyNone;
    for (int k = 0; k < K; ++k) {   // (every segment is checked, as on the device: the bounds are complete whatever fails first)
      const int64_t idx = b * K + k;
      const double T = times[b * ts_b + k * ts_k];
      double p[3][NC];
      mtgs::load_padded<NC, 3>(coeffs + idx * (int64_t)(D * N), N, D, p);
      const mtgc::SegmentResult r = mtgc::walk_segment<NC>(p, T, g, P, frontier[0], frontier[1]);
      if (o.seg_result) o.seg_result[idx] = r.result;
      if (o.seg_lower) o.seg_lower[idx] = r.lower_bound;
      if (o.seg_sampled) o.seg_sampled[idx] = r.sampled;
      if (o.seg_closest_time) o.seg_closest_time[idx] = r.closest_time;
      if (o.seg_failing_time) o.seg_failing_time[idx] = r.first_failing_time;
      if (o.seg_nodes) o.seg_nodes[idx] = r.nodes;
      if (o.seg_depth) o.seg_depth[idx] = r.depth;
      const unsigned long long kl = mtgf::order_key(r.lower_bound), ks = mtgf::order_key(r.sampled);
      if (kl < lower) lower = kl;
      if (ks < sampled) sampled = ks;
      if (r.result != MTG_FIELD_FREE && fseg < 0) { fseg = k; code = r.result; }
    }
    o.traj_result[b] = code;
    if (o.first_seg) o.first_seg[b] = fseg;
    if (o.traj_lower) o.traj_lower[b] = mtgf::order_value(lower);
    if (o.traj_sampled) o.traj_sampled[b] = mtgf::order_value(sampled);
  }
}

}  // namespace

extern "C" int mtg_certify_distance_field_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                               const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                               const mtg_distance_field* field, double lipschitz, int32_t min_depth, int32_t max_depth,
                                               int32_t max_frontier, double inflation, int32_t* trajectory_result,
                                               int32_t* first_failing_segment, int32_t* segment_result, double* segment_lower_bound,
                                               double* segment_sampled_clearance, double* segment_closest_time,
                                               double* segment_first_failing_time, int32_t* segment_nodes, int32_t* segment_depth,
                                               double* trajectory_lower_bound, double* trajectory_sampled_clearance) {
  if (!coeffs || !times || !trajectory_result) return MTG_ERR_INVALID_ARGUMENT;
  mtgf::Grid g;
  if (!mtgc::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, field, lipschitz, min_depth, max_depth,
                          max_frontier, inflation, &g))
    return MTG_ERR_INVALID_ARGUMENT;
  const mtgc::Rule P{lipschitz, inflation, min_depth, max_depth, max_frontier};
  const Outputs o{trajectory_result, first_failing_segment, segment_result, segment_lower_bound, segment_sampled_clearance,
                  segment_closest_time, segment_first_failing_time, segment_nodes, segment_depth, trajectory_lower_bound,
                  trajectory_sampled_clearance};
  mtgs::with_instance<mtgf::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, g, P, o);
  });
  return MTG_OK;
}

// L = max over the cells of sqrt(gx^2 + gy^2 + gz^2) / h, rounded up (1 + 2^-50 covers the six roundings of the formula).  A cell
// with a non-finite difference makes it non-finite.
extern "C" int mtg_distance_field_lipschitz_host(const mtg_distance_field* f, double* out) {
  if (!f || !out || !f->distances || f->nx < 2 || f->ny < 2 || f->nz < 2) return MTG_ERR_INVALID_ARGUMENT;
  if ((long long)f->nx * f->ny > mtgf::kMaxVoxels || (long long)f->nx * f->ny * f->nz > mtgf::kMaxVoxels) return MTG_ERR_INVALID_ARGUMENT;
  if (!(f->voxel_size > 0.0) || !(f->voxel_size <= DBL_MAX) || !(1.0 / f->voxel_size <= DBL_MAX)) return MTG_ERR_INVALID_ARGUMENT;
  const long long sy = f->nx, sz = (long long)f->nx * f->ny;
  double worst = 0.0;
  for (int z = 0; z + 1 < f->nz && worst == worst; ++z)
    for (int y = 0; y + 1 < f->ny && worst == worst; ++y) {
      const float* row = f->distances + z * sz + y * sy;
      for (int x = 0; x + 1 < f->nx; ++x) {
        const double c = mtgc::cell_gradient(row + x, sy, sz);
        if (c > worst || c != c) worst = c;
      }
    }
  *out = worst / f->voxel_size * (1.0 + 0x1p-50);
  return MTG_OK;
}
