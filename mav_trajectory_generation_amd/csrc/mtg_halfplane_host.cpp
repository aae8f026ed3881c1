// mtg_halfplane_host.cpp -- host build (plain g++, no HIP) of the half-plane feasibility check: the lane code of
// mtg_halfplane_lane.h run one segment after the other, and the two helpers that build plane sets (HalfPlane's constructor and
// HalfPlane::createBoundingBox, feasibility_base.cpp:54-86).  For the reference's one-trajectory-at-a-time callers
// (FeasibilityBase::checkHalfPlaneFeasibility(Segment) / (Trajectory)).  Touches no device: works in a process without a GPU.
#include <cmath>
#include <cstdint>

#include "../../include/mtg_hip.h"
#include "mtg_halfplane_lane.h"

extern "C" int mtg_half_planes_from_points_normals(int32_t n, const double* points, const double* normals, double* out) {
  if (n < 0 || (n > 0 && (!points || !normals || !out))) return MTG_ERR_INVALID_ARGUMENT;
  for (int32_t i = 0; i < n; ++i) {
    const double* v = normals + 3 * (int64_t)i;
    const double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(norm > 0.0) || !std::isfinite(norm)) return MTG_ERR_INVALID_ARGUMENT;   // (CHECK_GT(normal.norm(), 0.0), :57)
    double* o = out + 4 * (int64_t)i;
    for (int d = 0; d < 3; ++d) o[d] = v[d] / norm;   // (Eigen's normalize(): a division by the norm)
    const double* p = points + 3 * (int64_t)i;
    o[3] = p[0] * o[0] + p[1] * o[1] + p[2] * o[2];
  }
  return MTG_OK;
}

extern "C" int mtg_half_planes_bounding_box(const double* center, const double* size, double* out) {
  if (!center || !size || !out) return MTG_ERR_INVALID_ARGUMENT;
  for (int axis = 0; axis < 3; ++axis) {   // per axis: the minimum face with +e, then the maximum face with -e (:77-84)
    double* lo = out + 8 * axis;
    double* hi = lo + 4;
    for (int d = 0; d < 3; ++d) lo[d] = hi[d] = 0.0;
    lo[axis] = 1.0;
    hi[axis] = -1.0;
    lo[3] = center[axis] - size[axis] / 2.0;      // bbx_min . (+e)
    hi[3] = -(center[axis] + size[axis] / 2.0);   // bbx_max . (-e)
  }
  return MTG_OK;
}

namespace {

template <int NC>
void run(int N, int K, int D, int64_t B, const double* coeffs, const double* times, int64_t ts_b, int64_t ts_k, const double* planes,
         int P, int64_t ps_b, int64_t ps_k, int32_t* feasible, int32_t* first_seg, int32_t* first_plane, double* seg_clearance,
         double* traj_clearance) {
  double roots[mtgh::roots_len(NC)];
  double* r = roots;
  for (int64_t b = 0; b < B; ++b) {
    int fseg = -1, fplane = -1;
    double lowest = INFINITY;
    for (int k = 0; k < K; ++k) {   // (every segment is checked, as on the device: the clearances are complete whatever fails first)
      const int64_t idx = b * K + k;
      double clearance;
      const int plane = mtgh::segment_check<NC, double*>(coeffs + idx * (int64_t)(D * N), N, D, times[b * ts_b + k * ts_k],
                                                         planes + b * ps_b + k * ps_k, P, r, clearance);
      if (seg_clearance) seg_clearance[idx] = clearance;
      if (clearance < lowest) lowest = clearance;
      if (plane >= 0 && fseg < 0) { fseg = k; fplane = plane; }
    }
    feasible[b] = fseg < 0 ? 1 : 0;
    if (first_seg) first_seg[b] = fseg;
    if (first_plane) first_plane[b] = fplane == mtgh::kNoPlane ? -1 : fplane;
    if (traj_clearance) traj_clearance[b] = fplane == mtgh::kNoPlane ? NAN : lowest;
  }
}

}  // namespace

extern "C" int mtg_check_half_plane_feasibility_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                                     const double* coeffs, const double* times, int64_t times_stride_b,
                                                     int64_t times_stride_k, const double* planes, int32_t n_planes,
                                                     int64_t planes_stride_b, int64_t planes_stride_k, int32_t* trajectory_feasible,
                                                     int32_t* first_failing_segment, int32_t* first_failing_plane,
                                                     double* segment_clearance, double* trajectory_clearance) {
  if (!coeffs || !times || !planes || !trajectory_feasible) return MTG_ERR_INVALID_ARGUMENT;
  if (!mtgh::arguments_ok(n_coeffs, n_segments, dimension, batch, times_stride_b, times_stride_k, n_planes, planes_stride_b,
                          planes_stride_k))
    return MTG_ERR_INVALID_ARGUMENT;
  // the host can read the planes: every normal of every set in use must have unit length (|n|^2 within 1e-9 of 1)
  const int64_t nb = planes_stride_b ? batch : (batch > 0 ? 1 : 0), nk = planes_stride_k ? n_segments : 1;
  for (int64_t b = 0; b < nb; ++b)
    for (int64_t k = 0; k < nk; ++k)
      for (int h = 0; h < n_planes; ++h) {
        const double* v = planes + b * planes_stride_b + k * planes_stride_k + 4 * h;
        if (!(std::fabs(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] - 1.0) <= 1e-9)) return MTG_ERR_INVALID_ARGUMENT;
      }
  mtgs::with_instance<mtgh::kMinInstance>(n_coeffs, [&](auto nc) {
    run<decltype(nc)::value>(n_coeffs, n_segments, dimension, batch, coeffs, times, times_stride_b, times_stride_k, planes, n_planes,
                             planes_stride_b, planes_stride_k, trajectory_feasible, first_failing_segment, first_failing_plane,
                             segment_clearance, trajectory_clearance);
  });
  return MTG_OK;
}
