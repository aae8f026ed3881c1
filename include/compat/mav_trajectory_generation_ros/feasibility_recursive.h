// Compat veneer: FeasibilityRecursive (reference: mav_trajectory_generation_ros feasibility_recursive.h) on the C ABI.
// One Segment: the library's host build of the check (mtg_check_input_feasibility_recursive_host, no device needed);
// checkInputFeasibilityTrajectory is FeasibilityBase's loop over the segments, as in the reference.
#ifndef MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_RECURSIVE_H_
#define MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_RECURSIVE_H_
#include <cmath>
#include <cstdint>
#include <vector>

#include "../mav_trajectory_generation/segment.h"
#include "feasibility_base.h"

namespace mav_trajectory_generation {

class FeasibilityRecursive : public FeasibilityBase {
 public:
  class Settings {
   public:
    Settings() : min_section_time_s_(0.05) {}
    inline void setMinSectionTimeS(double min_section_time_s) { min_section_time_s_ = std::abs(min_section_time_s); }
    inline double getMinSectionTimeS() const { return min_section_time_s_; }

   private:
    double min_section_time_s_;   // shortest section the binary search examines
  };

  FeasibilityRecursive() {}
  FeasibilityRecursive(const Settings& settings) : FeasibilityBase(), settings_(settings) {}
  FeasibilityRecursive(const InputConstraints& input_constraints) : FeasibilityBase(input_constraints) {}
  FeasibilityRecursive(const Settings& settings, const InputConstraints& input_constraints)
      : FeasibilityBase(input_constraints), settings_(settings) {}

  virtual InputFeasibilityResult checkInputFeasibility(const Segment& segment) const {
    std::vector<double> c;
    for (int d = 0; d < segment.D(); ++d) {
      const Eigen::VectorXd v = segment[d].getCoefficients();
      for (int n = 0; n < segment.N(); ++n) c.push_back(v[n]);
    }
    const double t = segment.getTime();
    int32_t result = kInputIndeterminable;
    mtg_input_constraints ic = input_constraints_.toC();
    ic.min_section_time_s = settings_.getMinSectionTimeS();
    if (mtg_check_input_feasibility_recursive_host(segment.N(), 1, segment.D(), 1, c.data(), &t, 1, 1, &ic, &result, nullptr, nullptr,
                                                   nullptr, nullptr) != MTG_OK)
      return kInputIndeterminable;
    return (InputFeasibilityResult)result;
  }

  Settings settings_;
};

}  // namespace mav_trajectory_generation
#endif
