// Compat veneer: InputConstraints -- the dynamic limits of the vehicle (reference: mav_trajectory_generation_ros
// input_constraints.h, src/input_constraints.cpp), without the YAML members.  Public names and signatures only.
#ifndef MAV_TRAJECTORY_GENERATION_ROS_INPUT_CONSTRAINTS_H_
#define MAV_TRAJECTORY_GENERATION_ROS_INPUT_CONSTRAINTS_H_
#include <cmath>
#include <map>
#include <string>

#include "../../mtg_hip.h"

namespace mav_trajectory_generation {

enum InputConstraintType { kFMin = 0, kFMax, kVMax, kOmegaXYMax, kOmegaZMax, kOmegaZDotMax };

inline std::string getInputConstraintName(InputConstraintType type) {
  static const char* const names[] = {"f_min", "f_max", "v_max", "omega_xy_max", "omega_z_max", "omega_z_dot_max"};
  return type >= kFMin && type <= kOmegaZDotMax ? names[type] : "Unknown!";
}

class InputConstraints {
 public:
  InputConstraints() {}

  // Stored by magnitude; a new f_min lifts an existing f_max to at least it, a new f_max lowers an existing f_min.
  void addConstraint(int constraint_type, double value) {
    value = std::abs(value);
    double other;
    if (constraint_type == kFMin && getConstraint(kFMax, &other) && value > other) constraints_[kFMax] = value;
    if (constraint_type == kFMax && getConstraint(kFMin, &other) && value < other) constraints_[kFMin] = value;
    constraints_[constraint_type] = value;
  }
  void setDefaultValues() {
    mtg_input_constraints c;
    mtg_input_constraints_init(&c);
    mtg_input_constraints_set_defaults(&c);
    const double v[] = {c.f_min, c.f_max, c.v_max, c.omega_xy_max, c.omega_z_max, c.omega_z_dot_max};
    for (int i = 0; i < 6; ++i) constraints_[i] = v[i];
  }
  bool getConstraint(int constraint_type, double* value) const {
    const std::map<int, double>::const_iterator it = constraints_.find(constraint_type);
    if (it == constraints_.end()) return false;
    *value = it->second;
    return true;
  }
  bool hasConstraint(int constraint_type) const { return constraints_.count(constraint_type) != 0; }
  bool removeConstraint(int constraint_type) { return constraints_.erase(constraint_type) != 0; }

  // new: the C ABI's form (NaN = absent; min_section_time_s and gravity at their defaults)
  mtg_input_constraints toC() const {
    mtg_input_constraints c;
    mtg_input_constraints_init(&c);
    double* const slot[] = {&c.f_min, &c.f_max, &c.v_max, &c.omega_xy_max, &c.omega_z_max, &c.omega_z_dot_max};
    for (int i = 0; i < 6; ++i) getConstraint(i, slot[i]);
    return c;
  }

 private:
  std::map<int, double> constraints_;
};

}  // namespace mav_trajectory_generation
#endif
