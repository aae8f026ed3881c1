// The trajectory-to-trajectory separation check of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCheckTrajectorySeparation(Trajectory, Trajectory) on the library's host entry and TrajectoryBatch::checkSeparation on the
// device entry; two straight lines whose closest approach is known in closed form, and rows of the reference's results
// (tests/golden/reference_trajectory_separation_veneer_rows.txt, written from reference_trajectory_separation_n10_k8_d3_fast.npz).
//   test_trajectory_separation_veneer <rows file> host      -- needs no device
//   test_trajectory_separation_veneer <rows file> device    -- the batch form as well
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
  Trajectory a, b;
  double start_a, start_b;
  int feasible, first_a, first_b;
  double separation, scale;
};

// p(t) = origin + velocity t over `time`, N = 4
static Trajectory line(const double (&origin)[3], const double (&velocity)[3], double time) {
  Segment segment(4, 3);
  for (int d = 0; d < 3; ++d) {
    Eigen::VectorXd c(4);
    c.setZero();
    c[0] = origin[d];
    c[1] = velocity[d];
    segment[d] = Polynomial(4, c);
  }
  segment.setTime(time);
  Trajectory trajectory;
  trajectory.setSegments(Segment::Vector(1, segment));
  return trajectory;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;

  // ---- two straight lines: a along x from the origin, b along y from (2, -3, 1), both at unit speed from t = 0 for 6 s.
  // The difference is (t - 2, 3 - t, -1): squared distance 2 t^2 - 10 t + 14, smallest at t = 2.5: sqrt(1.5). ----
  {
    const Trajectory a = line({0.0, 0.0, 0.0}, {1.0, 0.0, 0.0}, 6.0), b = line({2.0, -3.0, 1.0}, {0.0, 1.0, 0.0}, 6.0);
    const double exact = std::sqrt(1.5);
    for (double need = 0.5; need < 2.0; need += 0.25) {
      int first_a = 7, first_b = 7;
      double separation = 0.0, when = 0.0;
      const bool feasible = mtgCheckTrajectorySeparation(a, b, need, 0.0, 0.0, &first_a, &first_b, &separation, &when);
      EXPECT(feasible == (exact > need));
      EXPECT(first_a == (feasible ? -1 : 0) && first_b == (feasible ? -1 : 0));
      EXPECT(std::fabs(separation - (exact - need)) <= 1e-12 && std::fabs(when - 2.5) <= 1e-9);
    }
    // b starts 1 s later: (t - 2, 4 - t, -1) on [1, 6], smallest at t = 3: sqrt(3); the time is global
    double separation = 0.0, when = 0.0;
    EXPECT(mtgCheckTrajectorySeparation(a, b, 1.0, 0.0, 1.0, nullptr, nullptr, &separation, &when));
    EXPECT(std::fabs(separation - (std::sqrt(3.0) - 1.0)) <= 1e-12 && std::fabs(when - 3.0) <= 1e-9);
    // never at the same time: apart, +inf, no time
    EXPECT(mtgCheckTrajectorySeparation(a, b, 1.0, 0.0, 6.0, nullptr, nullptr, &separation, &when) && std::isinf(separation) && when != when);
    // against itself: exactly -min_separation
    EXPECT(!mtgCheckTrajectorySeparation(a, a, 0.75, 0.0, 0.0, nullptr, nullptr, &separation) && separation == -0.75);
    // refused arguments
    EXPECT(!mtgCheckTrajectorySeparation(a, b, -1.0, 0.0, 0.0, nullptr, nullptr, &separation) && separation != separation);
    EXPECT(!mtgCheckTrajectorySeparation(a, b, 1.0, 0.0, std::nan(""), nullptr, nullptr, &separation) && separation != separation);
  }

  // ---- rows of the reference's results ----
  std::ifstream in(argv[1]);
  std::string header;
  std::getline(in, header);   // comment
  int N, K, D, n_rows;
  double min_separation;
  in >> N >> K >> D >> n_rows >> min_separation;
  std::vector<Row> rows(n_rows);
  auto read = [&](Trajectory& trajectory, double& start) {
    in >> start;
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
    trajectory.setSegments(segments);
  };
  for (Row& row : rows) {
    read(row.a, row.start_a);
    read(row.b, row.start_b);
    in >> row.feasible >> row.first_a >> row.first_b >> row.separation >> row.scale;
  }
  EXPECT(!in.fail() && n_rows >= 2);

  bool saw_feasible = false, saw_infeasible = false;
  std::vector<Trajectory> all;
  std::vector<double> starts;
  std::vector<int32_t> pairs;
  for (const Row& row : rows) {
    int first_a = 7, first_b = 7;
    double separation = 0.0;
    const bool feasible = mtgCheckTrajectorySeparation(row.a, row.b, min_separation, row.start_a, row.start_b, &first_a, &first_b, &separation);
    EXPECT((int)feasible == row.feasible && first_a == row.first_a && first_b == row.first_b);
    // (the reference's minimum can only be too large: one-sided 1e-9, the other side 1e-6 of the scale)
    EXPECT(separation - row.separation <= 1e-9 * row.scale && row.separation - separation <= 1e-6 * row.scale);
    saw_feasible = saw_feasible || feasible;
    saw_infeasible = saw_infeasible || !feasible;
    pairs.push_back((int32_t)all.size());
    pairs.push_back((int32_t)all.size() + 1);
    all.push_back(row.a);
    all.push_back(row.b);
    starts.push_back(row.start_a);
    starts.push_back(row.start_b);
  }
  EXPECT(saw_feasible && saw_infeasible);

  if (device) {
    TrajectoryBatch batch(all);
    std::vector<char> feasible;
    std::vector<int> first_a, first_b;
    std::vector<double> separation, when;
    EXPECT(batch.checkSeparation(batch, pairs, min_separation, starts, starts, &feasible, &first_a, &first_b, &separation, &when));
    EXPECT(feasible.size() == rows.size() && separation.size() == rows.size());
    for (size_t p = 0; p < rows.size() && p < feasible.size(); ++p) {
      EXPECT((int)feasible[p] == rows[p].feasible);
      EXPECT(first_a[p] == rows[p].first_a && first_b[p] == rows[p].first_b);
      EXPECT(separation[p] - rows[p].separation <= 1e-9 * rows[p].scale && rows[p].separation - separation[p] <= 1e-6 * rows[p].scale);
      EXPECT(when[p] >= starts[2 * p] && when[p] >= starts[2 * p + 1]);
    }
    // an index out of range: that pair alone is infeasible with a NaN separation
    std::vector<int32_t> with_bad = pairs;
    with_bad[1] = (int32_t)all.size();
    EXPECT(batch.checkSeparation(batch, with_bad, min_separation, starts, starts, &feasible, nullptr, nullptr, &separation));
    EXPECT(!feasible[0] && separation[0] != separation[0] && (int)feasible[1] == rows[1].feasible);
    EXPECT(!batch.checkSeparation(batch, pairs, -1.0, starts, starts, &feasible));
    EXPECT(!batch.checkSeparation(batch, {0, 1, 2}, 1.0, starts, starts, &feasible));
    EXPECT(!batch.checkSeparation(batch, pairs, 1.0, {0.0}, starts, &feasible));
    EXPECT(batch.checkSeparation(batch, {}, 1.0, {}, {}, &feasible) && feasible.empty());
  }
  if (failures == 0) std::printf("TRAJECTORY SEPARATION VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
