// Compat veneer: FeasibilityBase (reference: mav_trajectory_generation_ros feasibility_base.h): result codes, their names, the
// trajectory loop of the input check, and the half-plane check -- HalfPlane (both constructors, Vector, createBoundingBox), the
// public member half_plane_constraints_ and checkHalfPlaneFeasibility(Segment) / (Trajectory) on the library's host build of
// the check (mtg_check_half_plane_feasibility_host, no device needed); new: checkHalfPlaneFeasibilityBatch on a
// device-resident TrajectoryBatch (mtg_check_half_plane_feasibility on the MI355X).  DESIGN.md, "Half-plane feasibility".
#ifndef MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_BASE_H_
#define MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_BASE_H_
#include <cstdint>
#include <string>
#include <vector>

#include "../mav_trajectory_generation/trajectory.h"
#include "../mav_trajectory_generation/trajectory_batch.h"
#include "input_constraints.h"

namespace mav_trajectory_generation {

enum InputFeasibilityResult {
  kInputFeasible = 0,
  kInputIndeterminable,
  kInputInfeasibleThrustHigh,
  kInputInfeasibleThrustLow,
  kInputInfeasibleVelocity,
  kInputInfeasibleRollPitchRates,
  kInputInfeasibleYawRates,
  kInputInfeasibleYawAcc,
};

inline std::string getInputFeasibilityResultName(InputFeasibilityResult fr) {
  static const char* const names[] = {"Feasible", "Indeterminable", "InfeasibleThrustHigh", "InfeasibleThrustLow",
                                      "InfeasibleVelocity", "InfeasibleRollPitchRates", "InfeasibleYawRates", "InfeasibleYawAcc"};
  return fr >= kInputFeasible && fr <= kInputInfeasibleYawAcc ? names[fr] : "Unknown!";
}

// A half plane: a point on its boundary and the unit normal that points to the allowed side.
class HalfPlane {
 public:
  typedef std::vector<HalfPlane, Eigen::aligned_allocator<HalfPlane>> Vector;
  HalfPlane(const Eigen::Vector3d& point, const Eigen::Vector3d& normal) : point(point), normal(normal) {
    CHECK_GT(normal.norm(), 0.0) << "Invalid normal.";
    this->normal.normalize();
  }
  // through three points; the normal is (b - a) x (c - a)
  HalfPlane(const Eigen::Vector3d& a, const Eigen::Vector3d& b, const Eigen::Vector3d& c) {
    CHECK(a != b);
    CHECK(a != c);
    point = a;
    normal = (b - a).cross(c - a).normalized();
  }
  // six planes, per axis: the minimum face with +e, then the maximum face with -e (mtg_half_planes_bounding_box)
  static HalfPlane::Vector createBoundingBox(const Eigen::Vector3d& point, const Eigen::Vector3d& bounding_box_size) {
    const double center[3] = {point(0), point(1), point(2)};
    const double size[3] = {bounding_box_size(0), bounding_box_size(1), bounding_box_size(2)};
    double planes[6][4];
    mtg_half_planes_bounding_box(center, size, &planes[0][0]);
    HalfPlane::Vector bounding_box;
    bounding_box.reserve(6);
    for (int h = 0; h < 6; ++h) {
      const int axis = h / 2;
      Eigen::Vector3d on_face = point;
      on_face(axis) = (h & 1) ? -planes[h][3] : planes[h][3];
      bounding_box.emplace_back(on_face, Eigen::Vector3d(planes[h][0], planes[h][1], planes[h][2]));
    }
    return bounding_box;
  }
  Eigen::Vector3d point;
  Eigen::Vector3d normal;
};

class FeasibilityBase {
 public:
  FeasibilityBase() {}
  FeasibilityBase(const InputConstraints& input_constraints) : input_constraints_(input_constraints) {}
  virtual ~FeasibilityBase() {}

  // The result of the first segment that is not feasible (no segments: indeterminable).
  virtual InputFeasibilityResult checkInputFeasibilityTrajectory(const Trajectory& trajectory) const {
    InputFeasibilityResult result = kInputIndeterminable;
    for (const Segment& segment : trajectory.segments()) {
      result = checkInputFeasibility(segment);
      if (result != kInputFeasible) break;
    }
    return result;
  }
  virtual InputFeasibilityResult checkInputFeasibility(const Segment& /*segment*/) const { return kInputIndeterminable; }
  InputConstraints getInputConstraints() const { return input_constraints_; }

  // Is the segment strictly inside every half plane of half_plane_constraints_ (positions only; dimension 3 or 4)?
  bool checkHalfPlaneFeasibility(const Segment& segment) const {
    if (!(segment.D() == 3 || segment.D() == 4)) return false;
    if (half_plane_constraints_.empty()) return true;
    std::vector<double> c;
    appendCoefficients(segment, &c);
    const double t = segment.getTime();
    const std::vector<double> planes = packedHalfPlanes();
    int32_t feasible = 0;
    return mtg_check_half_plane_feasibility_host(segment.N(), 1, segment.D(), 1, c.data(), &t, 1, 1, planes.data(),
                                                 (int32_t)half_plane_constraints_.size(), 0, 0, &feasible, nullptr, nullptr, nullptr,
                                                 nullptr) == MTG_OK && feasible == 1;
  }
  // One host call for the whole trajectory; segments of different shapes are walked one by one (the reference's loop).
  bool checkHalfPlaneFeasibility(const Trajectory& trajectory) const {
    const Segment::Vector& segments = trajectory.segments();
    bool uniform = !segments.empty() && !half_plane_constraints_.empty() && (segments[0].D() == 3 || segments[0].D() == 4);
    for (const Segment& s : segments) uniform = uniform && s.N() == segments[0].N() && s.D() == segments[0].D();
    if (!uniform) {
      for (const Segment& s : segments)
        if (!checkHalfPlaneFeasibility(s)) return false;
      return true;
    }
    std::vector<double> c, t;
    for (const Segment& s : segments) {
      appendCoefficients(s, &c);
      t.push_back(s.getTime());
    }
    const std::vector<double> planes = packedHalfPlanes();
    int32_t feasible = 0;
    return mtg_check_half_plane_feasibility_host(segments[0].N(), (int32_t)segments.size(), segments[0].D(), 1, c.data(), t.data(),
                                                 (int64_t)segments.size(), 1, planes.data(), (int32_t)half_plane_constraints_.size(), 0,
                                                 0, &feasible, nullptr, nullptr, nullptr, nullptr) == MTG_OK && feasible == 1;
  }
  // new: every trajectory of a device-resident batch against half_plane_constraints_ in one call; first_failing_segment /
  // first_failing_plane (optional): -1 where feasible.
  bool checkHalfPlaneFeasibilityBatch(const TrajectoryBatch& batch, std::vector<bool>* feasible,
                                      std::vector<int>* first_failing_segment = nullptr,
                                      std::vector<int>* first_failing_plane = nullptr) const {
    CHECK_NOTNULL(feasible);
    const int64_t B = (int64_t)batch.size();
    if (half_plane_constraints_.empty()) {
      feasible->assign(B, batch.D() == 3 || batch.D() == 4);
      if (first_failing_segment) first_failing_segment->assign(B, feasible->empty() || (*feasible)[0] ? -1 : 0);
      if (first_failing_plane) first_failing_plane->assign(B, -1);
      return true;
    }
    mtg_context* ctx = mtg_compat_detail::context();
    const std::vector<double> planes = packedHalfPlanes();
    void *d_planes = nullptr, *d_out = nullptr;
    if (mtg_device_malloc(ctx, sizeof(double) * planes.size(), &d_planes) != MTG_OK) return false;
    if (mtg_device_malloc(ctx, sizeof(int32_t) * 3 * (B > 0 ? B : 1), &d_out) != MTG_OK) { mtg_device_free(ctx, d_planes); return false; }
    int32_t* out = (int32_t*)d_out;
    std::vector<int32_t> h(3 * B);
    const bool ok = mtg_copy_to_device(ctx, d_planes, planes.data(), sizeof(double) * planes.size()) == MTG_OK &&
                    mtg_check_half_plane_feasibility(ctx, batch.N(), batch.K(), batch.D(), B, batch.deviceCoefficients(), batch.deviceTimes(),
                                                     batch.K(), 1, (const double*)d_planes, (int32_t)half_plane_constraints_.size(), 0, 0,
                                                     out, out + B, out + 2 * B, nullptr, nullptr) == MTG_OK &&
                    (B == 0 || mtg_copy_to_host(ctx, h.data(), d_out, sizeof(int32_t) * 3 * B) == MTG_OK);
    mtg_device_free(ctx, d_planes);
    mtg_device_free(ctx, d_out);
    if (!ok) return false;
    feasible->resize(B);
    for (int64_t b = 0; b < B; ++b) (*feasible)[b] = h[b] == 1;
    if (first_failing_segment) first_failing_segment->assign(h.begin() + B, h.begin() + 2 * B);
    if (first_failing_plane) first_failing_plane->assign(h.begin() + 2 * B, h.end());
    return true;
  }

  InputConstraints input_constraints_;
  HalfPlane::Vector half_plane_constraints_;

 private:
  // rows (unit normal, point . normal): the plane format of mtg_check_half_plane_feasibility
  std::vector<double> packedHalfPlanes() const {
    std::vector<double> planes;
    planes.reserve(4 * half_plane_constraints_.size());
    for (const HalfPlane& hp : half_plane_constraints_) {
      for (int d = 0; d < 3; ++d) planes.push_back(hp.normal(d));
      planes.push_back(hp.point(0) * hp.normal(0) + hp.point(1) * hp.normal(1) + hp.point(2) * hp.normal(2));
    }
    return planes;
  }
  static void appendCoefficients(const Segment& segment, std::vector<double>* c) {
    for (int d = 0; d < segment.D(); ++d) {
      const Eigen::VectorXd v = segment[d].getCoefficients();
      for (int n = 0; n < segment.N(); ++n) c->push_back(v[n]);
    }
  }
};

}  // namespace mav_trajectory_generation
#endif
