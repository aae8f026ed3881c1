// Compat veneer: the input-feasibility part of FeasibilityBase (reference: mav_trajectory_generation_ros
// feasibility_base.h): result codes, their names, and the trajectory loop.  The half-plane checks are not provided
// ("Input feasibility": out of scope).
#ifndef MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_BASE_H_
#define MAV_TRAJECTORY_GENERATION_ROS_FEASIBILITY_BASE_H_
#include <string>

#include "../mav_trajectory_generation/trajectory.h"
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

  InputConstraints input_constraints_;
};

}  // namespace mav_trajectory_generation
#endif
