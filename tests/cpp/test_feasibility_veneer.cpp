// FeasibilityAnalytic of the compat veneer (include/compat/mav_trajectory_generation_ros/) through the reference's API:
// one Segment and one Trajectory on the library's host entry, a TrajectoryBatch on the device, against each other and
// against rows of the reference's own verdicts (tests/golden/reference_feasibility_veneer_rows.txt).
//   test_feasibility_veneer <rows file> host      -- needs no device
//   test_feasibility_veneer <rows file> device    -- the batch form as well
#include <mav_trajectory_generation_ros/feasibility_analytic.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace mav_trajectory_generation;

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Row {
  Trajectory trajectory;
  std::vector<int> segment_result;
  int trajectory_result, first_failing_segment;
};

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;
  std::ifstream in(argv[1]);
  std::string line;
  std::getline(in, line);   // comment
  int N, K, D, n_rows;
  in >> N >> K >> D >> n_rows;
  std::string word;
  InputConstraints constraints;
  for (int i = 0; i < 6; ++i) {
    in >> word;
    if (word != "nan") constraints.addConstraint(i, std::stod(word));
  }
  double min_section;
  in >> min_section;
  std::vector<Row> rows(n_rows);
  for (Row& row : rows) {
    std::vector<double> times(K);
    for (double& t : times) in >> t;
    Segment::Vector segments(K, Segment(N, D));
    for (int k = 0; k < K; ++k) {
      segments[k].setTime(times[k]);
      for (int d = 0; d < D; ++d) {
        Eigen::VectorXd c(N);
        for (int n = 0; n < N; ++n) in >> c[n];
        segments[k][d] = Polynomial(N, c);
      }
    }
    row.trajectory.setSegments(segments);
    row.segment_result.resize(K);
    for (int& r : row.segment_result) in >> r;
    in >> row.trajectory_result >> row.first_failing_segment;
  }
  EXPECT(!in.fail() && n_rows >= 2);

  // names and the constraint container
  EXPECT(getInputFeasibilityResultName(kInputFeasible) == "Feasible");
  EXPECT(getInputFeasibilityResultName(kInputInfeasibleYawAcc) == "InfeasibleYawAcc");
  EXPECT(kInputInfeasibleRollPitchRates == 5 && kInputInfeasibleYawAcc == 7);
  EXPECT(getInputConstraintName(kOmegaZDotMax) == "omega_z_dot_max");
  {
    InputConstraints ic;
    double v = 0.0;
    EXPECT(!ic.hasConstraint(kFMin) && !ic.getConstraint(kVMax, &v));
    ic.addConstraint(kFMax, -10.0);
    ic.addConstraint(kFMin, 12.0);
    EXPECT(ic.getConstraint(kFMax, &v) && v == 12.0);
    ic.addConstraint(kFMax, 6.0);
    EXPECT(ic.getConstraint(kFMin, &v) && v == 6.0);
    EXPECT(ic.removeConstraint(kFMin) && !ic.removeConstraint(kFMin));
    ic.setDefaultValues();
    EXPECT(ic.getConstraint(kFMin, &v) && v == 0.5 * 9.81 && ic.getConstraint(kOmegaZDotMax, &v) && v == 2.0 * M_PI);
    FeasibilityAnalytic::Settings s;
    EXPECT(s.getMinSectionTimeS() == 0.05);
    s.setMinSectionTimeS(-0.01);
    EXPECT(s.getMinSectionTimeS() == 0.01);
  }

  FeasibilityAnalytic::Settings settings;
  settings.setMinSectionTimeS(min_section);
  const FeasibilityAnalytic checker(settings, constraints);
  const FeasibilityBase& as_base = checker;
  bool saw_infeasible = false, saw_feasible = false;
  std::vector<Trajectory> all;
  for (const Row& row : rows) {
    for (int k = 0; k < K; ++k)
      EXPECT((int)checker.checkInputFeasibility(row.trajectory.segments()[k]) == row.segment_result[k]);
    const InputFeasibilityResult r = checker.checkInputFeasibilityTrajectory(row.trajectory);
    EXPECT((int)r == row.trajectory_result);
    EXPECT(as_base.checkInputFeasibilityTrajectory(row.trajectory) == r);                   // virtual dispatch
    EXPECT(checker.FeasibilityBase::checkInputFeasibilityTrajectory(row.trajectory) == r);   // the segment-by-segment loop
    saw_infeasible = saw_infeasible || r != kInputFeasible;
    saw_feasible = saw_feasible || r == kInputFeasible;
    all.push_back(row.trajectory);
  }
  EXPECT(saw_infeasible && saw_feasible);
  EXPECT(FeasibilityAnalytic().checkInputFeasibility(rows[0].trajectory.segments()[0]) == kInputFeasible);   // no limits: feasible
  EXPECT(FeasibilityBase().checkInputFeasibility(rows[0].trajectory.segments()[0]) == kInputIndeterminable);
  EXPECT(checker.checkInputFeasibility(Segment(N, 2)) == kInputIndeterminable);

  if (device) {
    TrajectoryBatch batch(all);
    std::vector<InputFeasibilityResult> results;
    std::vector<int> first;
    EXPECT(checker.checkInputFeasibilityBatch(batch, &results, &first));
    EXPECT(results.size() == rows.size());
    for (size_t b = 0; b < rows.size() && b < results.size(); ++b) {
      EXPECT((int)results[b] == rows[b].trajectory_result);
      EXPECT(first[b] == rows[b].first_failing_segment);
      EXPECT(results[b] == checker.checkInputFeasibilityTrajectory(rows[b].trajectory));
    }
  }
  if (failures == 0) std::printf("FEASIBILITY VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
