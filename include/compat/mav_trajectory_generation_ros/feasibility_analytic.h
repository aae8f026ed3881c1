// Compat veneer: FeasibilityAnalytic (reference: mav_trajectory_generation_ros feasibility_analytic.h) on the C ABI.
// One Segment / one Trajectory: the library's host build of the check (mtg_check_input_feasibility_host, no device needed);
// new: checkInputFeasibilityBatch on a device-resident TrajectoryBatch (mtg_check_input_feasibility on the MI355X).
#ifndef MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_ANALYTIC_H_
#define MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_ANALYTIC_H_
#include <cmath>
#include <cstdint>
#include <vector>

#include "../mav_trajectory_generation/segment.h"
#include "../mav_trajectory_generation/trajectory_batch.h"
#include "feasibility_base.h"

namespace mav_trajectory_generation {

class FeasibilityAnalytic : public FeasibilityBase {
 public:
  class Settings {
   public:
    Settings() : min_section_time_s_(0.05) {}
    inline void setMinSectionTimeS(double min_section_time_s) { min_section_time_s_ = std::abs(min_section_time_s); }
    inline double getMinSectionTimeS() const { return min_section_time_s_; }

   private:
    double min_section_time_s_;   // shortest section the roll/pitch split examines
  };

  FeasibilityAnalytic() {}
  FeasibilityAnalytic(const Settings& settings) : FeasibilityBase(), settings_(settings) {}
  FeasibilityAnalytic(const InputConstraints& input_constraints) : FeasibilityBase(input_constraints) {}
  FeasibilityAnalytic(const Settings& settings, const InputConstraints& input_constraints)
      : FeasibilityBase(input_constraints), settings_(settings) {}

  virtual InputFeasibilityResult checkInputFeasibility(const Segment& segment) const {
    std::vector<double> c;
    append(segment, &c);
    const double t = segment.getTime();
    int32_t result = kInputIndeterminable;
    const mtg_input_constraints ic = constraints();
    if (mtg_check_input_feasibility_host(segment.N(), 1, segment.D(), 1, c.data(), &t, 1, 1, &ic, &result, nullptr, nullptr,
                                         nullptr) != MTG_OK)
      return kInputIndeterminable;
    return (InputFeasibilityResult)result;
  }

  // One host call for the whole trajectory (the base class walks the segments one by one, with the same result).
  virtual InputFeasibilityResult checkInputFeasibilityTrajectory(const Trajectory& trajectory) const {
    const Segment::Vector& segments = trajectory.segments();
    if (segments.empty()) return kInputIndeterminable;
    std::vector<double> c, t;
    for (const Segment& s : segments) {
      if (s.N() != segments[0].N() || s.D() != segments[0].D()) return FeasibilityBase::checkInputFeasibilityTrajectory(trajectory);
      append(s, &c);
      t.push_back(s.getTime());
    }
    int32_t result = kInputIndeterminable;
    const mtg_input_constraints ic = constraints();
    if (mtg_check_input_feasibility_host(segments[0].N(), (int32_t)segments.size(), segments[0].D(), 1, c.data(), t.data(),
                                         (int64_t)segments.size(), 1, &ic, &result, nullptr, nullptr, nullptr) != MTG_OK)
      return kInputIndeterminable;
    return (InputFeasibilityResult)result;
  }

  // new: every trajectory of a device-resident batch in one launch; first_failing_segment (optional): -1 where feasible.
  bool checkInputFeasibilityBatch(const TrajectoryBatch& batch, std::vector<InputFeasibilityResult>* results,
                                  std::vector<int>* first_failing_segment = nullptr) const {
    CHECK_NOTNULL(results);
    mtg_context* ctx = mtg_compat_detail::context();
    const int64_t B = (int64_t)batch.size();
    void *d_result = nullptr, *d_first = nullptr;
    if (mtg_device_malloc(ctx, sizeof(int32_t) * B, &d_result) != MTG_OK) return false;
    if (mtg_device_malloc(ctx, sizeof(int32_t) * B, &d_first) != MTG_OK) { mtg_device_free(ctx, d_result); return false; }
    const mtg_input_constraints ic = constraints();
    std::vector<int32_t> h(B), hf(B);
    const bool ok = mtg_check_input_feasibility(ctx, batch.N(), batch.K(), batch.D(), B, batch.deviceCoefficients(), batch.deviceTimes(),
                                                batch.K(), 1, &ic, (int32_t*)d_result, (int32_t*)d_first, nullptr, nullptr) == MTG_OK &&
                    mtg_copy_to_host(ctx, h.data(), d_result, sizeof(int32_t) * B) == MTG_OK &&
                    mtg_copy_to_host(ctx, hf.data(), d_first, sizeof(int32_t) * B) == MTG_OK;
    mtg_device_free(ctx, d_result);
    mtg_device_free(ctx, d_first);
    if (!ok) return false;
    results->resize(B);
    for (int64_t b = 0; b < B; ++b) (*results)[b] = (InputFeasibilityResult)h[b];
    if (first_failing_segment) first_failing_segment->assign(hf.begin(), hf.end());
    return true;
  }

  Settings settings_;

 private:
  mtg_input_constraints constraints() const {
    mtg_input_constraints ic = input_constraints_.toC();
    ic.min_section_time_s = settings_.getMinSectionTimeS();
    return ic;
  }
  static void append(const Segment& segment, std::vector<double>* c) {
    for (int d = 0; d < segment.D(); ++d) {
      const Eigen::VectorXd v = segment[d].getCoefficients();
      for (int n = 0; n < segment.N(); ++n) c->push_back(v[n]);
    }
  }
};

}  // namespace mav_trajectory_generation
#endif
