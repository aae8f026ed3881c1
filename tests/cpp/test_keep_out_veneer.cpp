// The keep-out zone check of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCheckKeepOutZones(Trajectory) on the library's host entry and TrajectoryBatch::checkKeepOutZones on the device entry; two
// straight lines past the unit box whose answers are known by hand, and rows of the reference's results
// (tests/golden/reference_keep_out_veneer_rows.txt, written from reference_keep_out_n10_k8_d3_fast.npz).
//   test_keep_out_veneer <rows file> host      -- needs no device
//   test_keep_out_veneer <rows file> device    -- the batch form as well
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
  int feasible, first_segment, first_zone;
  double clearance, scale;
};

// p(t) = a + v t over T as a one-segment trajectory, N = 4
static Trajectory line(const double (&a)[3], const double (&v)[3], double T) {
  Segment segment(4, 3);
  for (int d = 0; d < 3; ++d) {
    Eigen::VectorXd c(4);
    c.setZero();
    c(0) = a[d];
    c(1) = v[d];
    segment[d] = Polynomial(4, c);
  }
  segment.setTime(T);
  Trajectory trajectory;
  trajectory.setSegments(Segment::Vector(1, segment));
  return trajectory;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;

  // ---- the unit box at the origin, HalfPlane::createBoundingBox's planes as they stand ----
  {
    std::vector<double> box(24);
    const double center[3] = {0.0, 0.0, 0.0}, size[3] = {1.0, 1.0, 1.0};
    EXPECT(mtg_half_planes_bounding_box(center, size, box.data()) == MTG_OK);
    int first_segment = 7, first_zone = 7;
    double clearance = 0.0;
    // (t - 2, 0.3, 0) through the box: 0.2 inside the face y = 0.5
    EXPECT(!mtgCheckKeepOutZones(line({-2.0, 0.3, 0.0}, {1.0, 0.0, 0.0}, 4.0), box, 6, 0.0, &first_segment, &first_zone, &clearance));
    EXPECT(first_segment == 0 && first_zone == 0 && std::fabs(clearance + 0.2) <= 1e-12);
    // (1.6 - t, t, 0) past the edge (0.5, 0.5, z): 0.3 at the crossing of two planes, t = 0.8
    EXPECT(mtgCheckKeepOutZones(line({1.6, 0.0, 0.0}, {-1.0, 1.0, 0.0}, 1.6), box, 6, 0.0, &first_segment, &first_zone, &clearance));
    EXPECT(first_segment == -1 && first_zone == -1 && std::fabs(clearance - 0.3) <= 1e-11);
    EXPECT(!mtgCheckKeepOutZones(line({1.6, 0.0, 0.0}, {-1.0, 1.0, 0.0}, 1.6), box, 6, 0.31));
    // refused arguments
    EXPECT(!mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), box, 6, -1.0, &first_segment, &first_zone, &clearance));
    EXPECT(first_segment == -1 && first_zone == -1 && clearance != clearance);
    EXPECT(!mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), {}, 6));
    EXPECT(!mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), box, 5));
    EXPECT(!mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), box, 0));
    std::vector<double> bent = box;
    bent[0] = 1.001;
    EXPECT(!mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), bent, 6));
    EXPECT(mtgCheckKeepOutZones(line({9.0, 9.0, 9.0}, {1.0, 0.0, 0.0}, 1.0), box, 6, 0.5));
  }

  // ---- rows of the reference's results ----
  std::ifstream in(argv[1]);
  std::string text;
  std::getline(in, text);   // comment
  int N, K, D, n_rows, M, P;
  double inflation;
  in >> N >> K >> D >> n_rows >> M >> P >> inflation;
  std::vector<double> zones(4 * (size_t)M * P);
  for (double& v : zones) in >> v;
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
    in >> row.feasible >> row.first_segment >> row.first_zone >> row.clearance >> row.scale;
  }
  EXPECT(!in.fail() && n_rows >= 2 && M >= 1 && P >= 1);

  bool saw_feasible = false, saw_infeasible = false;
  std::vector<Trajectory> all;
  for (const Row& row : rows) {
    int first_segment = 7, first_zone = 7;
    double clearance = 0.0;
    const bool feasible = mtgCheckKeepOutZones(row.trajectory, zones, P, inflation, &first_segment, &first_zone, &clearance);
    EXPECT((int)feasible == row.feasible && first_segment == row.first_segment && first_zone == row.first_zone);
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
    std::vector<int> first_segment, first_zone;
    std::vector<double> clearance;
    EXPECT(batch.checkKeepOutZones(zones, P, inflation, &feasible, &first_segment, &first_zone, &clearance));
    EXPECT(feasible.size() == rows.size() && clearance.size() == rows.size());
    for (size_t b = 0; b < rows.size() && b < feasible.size(); ++b) {
      EXPECT((int)feasible[b] == rows[b].feasible);
      EXPECT(first_segment[b] == rows[b].first_segment && first_zone[b] == rows[b].first_zone);
      EXPECT(clearance[b] - rows[b].clearance <= 1e-9 * rows[b].scale && rows[b].clearance - clearance[b] <= 1e-6 * rows[b].scale);
    }
    EXPECT(!batch.checkKeepOutZones({}, P, 0.0, &feasible));
    EXPECT(!batch.checkKeepOutZones(zones, 9, 0.0, &feasible));
    EXPECT(!batch.checkKeepOutZones(zones, P, -1.0, &feasible));
  }
  if (failures == 0) std::printf("KEEP-OUT ZONE VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
