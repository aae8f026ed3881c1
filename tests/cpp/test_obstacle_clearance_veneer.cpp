// The sphere-obstacle clearance check of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCheckObstacleClearance(Trajectory) on the library's host entry and TrajectoryBatch::checkObstacleClearance on the device
// entry; the reference test's curve x = t, z = t^2 (test/test_feasibility.cpp:296-309) past one sphere and rows of the
// reference's results (tests/golden/reference_obstacle_clearance_veneer_rows.txt, written from
// reference_obstacle_clearance_n10_k8_d3_fast.npz).
//   test_obstacle_clearance_veneer <rows file> host      -- needs no device
//   test_obstacle_clearance_veneer <rows file> device    -- the batch form as well
#include <mav_trajectory_generation/trajectory_batch.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
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
  int feasible, first_segment, first_obstacle;
  double clearance, scale;
};

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;

  // ---- the reference test's curve: N = 3, x = t, z = t^2, T = 1, past a sphere at (0.5, 0, -1) ----
  {
    Eigen::VectorXd coeffs_x(3), coeffs_y(3), coeffs_z(3);
    coeffs_x(1) = 1;
    coeffs_z(2) = 1;
    Segment segment(3, 3);
    segment[0] = Polynomial(3, coeffs_x);
    segment[1] = Polynomial(3, coeffs_y);
    segment[2] = Polynomial(3, coeffs_z);
    segment.setTime(1.0);
    Trajectory trajectory;
    trajectory.setSegments(Segment::Vector(1, segment));
    // the squared distance (t - 1/2)^2 + (t^2 + 1)^2 has the derivative 4 t^3 + 6 t - 1: one real root, by Cardano
    const double disc = std::sqrt(1.0 / 64.0 + 1.0 / 8.0);
    const double t = std::cbrt(0.125 + disc) + std::cbrt(0.125 - disc);
    const double exact = std::sqrt((t - 0.5) * (t - 0.5) + (t * t + 1.0) * (t * t + 1.0));
    for (double radius = 0.5; radius < 1.5; radius += 0.05) {
      if (std::fabs(exact - radius) <= 1e-9) continue;
      int first_segment = 7, first_obstacle = 7;
      double clearance = 0.0;
      const bool feasible = mtgCheckObstacleClearance(trajectory, {0.5, 0.0, -1.0, radius}, 0.0, &first_segment, &first_obstacle, &clearance);
      EXPECT(feasible == (exact > radius));
      EXPECT(first_segment == (feasible ? -1 : 0) && first_obstacle == (feasible ? -1 : 0));
      EXPECT(std::fabs(clearance - (exact - radius)) <= 1e-12);
    }
    double clearance = 0.0;
    EXPECT(!mtgCheckObstacleClearance(trajectory, {0.5, 0.0, -1.0, -0.1}, 0.0, nullptr, nullptr, &clearance) && clearance != clearance);
    EXPECT(!mtgCheckObstacleClearance(trajectory, {}, 0.0));
    EXPECT(!mtgCheckObstacleClearance(trajectory, {9.0, 9.0, 9.0, 0.1}, -1.0));
    EXPECT(mtgCheckObstacleClearance(trajectory, {9.0, 9.0, 9.0, 0.1}, 0.5));
  }

  // ---- rows of the reference's results ----
  std::ifstream in(argv[1]);
  std::string line;
  std::getline(in, line);   // comment
  int N, K, D, n_rows, M;
  double inflation;
  in >> N >> K >> D >> n_rows >> M >> inflation;
  std::vector<double> obstacles(4 * (size_t)M);
  for (double& v : obstacles) in >> v;
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
    in >> row.feasible >> row.first_segment >> row.first_obstacle >> row.clearance >> row.scale;
  }
  EXPECT(!in.fail() && n_rows >= 2 && M >= 1);

  bool saw_feasible = false, saw_infeasible = false;
  std::vector<Trajectory> all;
  for (const Row& row : rows) {
    int first_segment = 7, first_obstacle = 7;
    double clearance = 0.0;
    const bool feasible = mtgCheckObstacleClearance(row.trajectory, obstacles, inflation, &first_segment, &first_obstacle, &clearance);
    EXPECT((int)feasible == row.feasible && first_segment == row.first_segment && first_obstacle == row.first_obstacle);
    // (the reference's minimum can only be too large: one-sided 1e-9, the other side 1e-6 of the scale)
    EXPECT(clearance - row.clearance <= 1e-9 * row.scale && row.clearance - clearance <= 1e-6 * row.scale);
    saw_feasible = saw_feasible || feasible;
    saw_infeasible = saw_infeasible || !feasible;
    all.push_back(row.trajectory);
  }
  EXPECT(saw_feasible && saw_infeasible);

  if (device) {
    TrajectoryBatch batch(all);
    std::vector<char> feasible;
    std::vector<int> first_segment, first_obstacle;
    std::vector<double> clearance;
    EXPECT(batch.checkObstacleClearance(obstacles, inflation, &feasible, &first_segment, &first_obstacle, &clearance));
    EXPECT(feasible.size() == rows.size() && clearance.size() == rows.size());
    for (size_t b = 0; b < rows.size() && b < feasible.size(); ++b) {
      EXPECT((int)feasible[b] == rows[b].feasible);
      EXPECT(first_segment[b] == rows[b].first_segment && first_obstacle[b] == rows[b].first_obstacle);
      EXPECT(clearance[b] - rows[b].clearance <= 1e-9 * rows[b].scale && rows[b].clearance - clearance[b] <= 1e-6 * rows[b].scale);
    }
    EXPECT(!batch.checkObstacleClearance({}, 0.0, &feasible));
    EXPECT(!batch.checkObstacleClearance(obstacles, -1.0, &feasible));
  }
  if (failures == 0) std::printf("OBSTACLE CLEARANCE VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
