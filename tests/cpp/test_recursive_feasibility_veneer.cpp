// FeasibilityRecursive of the compat veneer (include/compat/mav_trajectory_generation_ros/feasibility_recursive.h) through the
// reference's API: Settings, the three constructors, checkInputFeasibility(Segment) on the library's host entry and
// checkInputFeasibilityTrajectory of FeasibilityBase, against rows of the reference's verdicts
// (tests/golden/reference_recursive_feasibility_veneer_rows.txt, written from reference_recursive_feasibility_n12_k4_d4.npz).
//   test_recursive_feasibility_veneer <rows file>      -- needs no device
#include <mav_trajectory_generation_ros/feasibility_recursive.h>

#include <cmath>
#include <cstdio>
#include <fstream>
#include <set>
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
  int result, first_segment;
};

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s <rows file>\n", argv[0]); return 2; }

  // ---- Settings and the constructors ----
  {
    FeasibilityRecursive::Settings settings;
    EXPECT(settings.getMinSectionTimeS() == 0.05);
    settings.setMinSectionTimeS(-0.2);
    EXPECT(settings.getMinSectionTimeS() == 0.2);
    EXPECT(FeasibilityRecursive().settings_.getMinSectionTimeS() == 0.05);
    EXPECT(FeasibilityRecursive(settings).settings_.getMinSectionTimeS() == 0.2);
    InputConstraints limits;
    limits.addConstraint(kVMax, 1.0);
    EXPECT(FeasibilityRecursive(limits).settings_.getMinSectionTimeS() == 0.05);
    EXPECT(FeasibilityRecursive(settings, limits).settings_.getMinSectionTimeS() == 0.2);

    // x' = 2: velocity; hover with no limit: feasible, but indeterminable once the segment is shorter than a section
    Eigen::VectorXd line = Eigen::VectorXd::Zero(6), zero = Eigen::VectorXd::Zero(6);
    line(1) = 2.0;
    Segment segment(6, 3);
    segment[0] = Polynomial(6, line);
    segment[1] = Polynomial(6, zero);
    segment[2] = Polynomial(6, zero);
    segment.setTime(0.1);
    EXPECT(FeasibilityRecursive(limits).checkInputFeasibility(segment) == kInputInfeasibleVelocity);
    EXPECT(FeasibilityRecursive().checkInputFeasibility(segment) == kInputFeasible);
    EXPECT(FeasibilityRecursive(settings).checkInputFeasibility(segment) == kInputIndeterminable);
    EXPECT(FeasibilityRecursive(limits).checkInputFeasibility(Segment(6, 2)) == kInputIndeterminable);
    const FeasibilityBase& base = FeasibilityRecursive(limits);   // virtual: the base's trajectory loop reaches the recursive check
    Trajectory trajectory;
    trajectory.setSegments(Segment::Vector(2, segment));
    EXPECT(base.checkInputFeasibilityTrajectory(trajectory) == kInputInfeasibleVelocity);
  }

  // ---- rows of the reference's verdicts ----
  std::ifstream in(argv[1]);
  std::string line;
  std::getline(in, line);   // comment
  int N, K, D, n_rows;
  in >> N >> K >> D >> n_rows;
  InputConstraints limits;
  for (int type = kFMin; type <= kOmegaZDotMax; ++type) {
    std::string word;
    in >> word;
    if (word != "nan") limits.addConstraint(type, std::stod(word));
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
    in >> row.result >> row.first_segment;
  }
  EXPECT(!in.fail() && n_rows == 8);

  FeasibilityRecursive::Settings settings;
  settings.setMinSectionTimeS(min_section);
  const FeasibilityRecursive checker(settings, limits);
  std::set<int> seen;
  for (const Row& row : rows) {
    int first = -1;
    for (int k = 0; k < K; ++k) {
      const InputFeasibilityResult r = checker.checkInputFeasibility(row.trajectory.segments()[k]);
      EXPECT((int)r == row.segment_result[k]);
      if (r != kInputFeasible && first < 0) first = k;
    }
    EXPECT(first == row.first_segment);
    EXPECT((int)checker.checkInputFeasibilityTrajectory(row.trajectory) == row.result);
    seen.insert(row.result);
  }
  EXPECT(seen.size() >= 3 && seen.count(kInputFeasible) == 1);

  if (failures == 0) std::printf("RECURSIVE FEASIBILITY VENEER TESTS PASSED (host)\n");
  return failures == 0 ? 0 : 1;
}
