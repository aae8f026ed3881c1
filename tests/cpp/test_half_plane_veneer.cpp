// The half-plane check of the compat veneer (include/compat/mav_trajectory_generation_ros/feasibility_base.h) through the
// reference's API: HalfPlane, createBoundingBox, half_plane_constraints_, checkHalfPlaneFeasibility(Segment | Trajectory) on the
// library's host entry; the reference's own HalfPlaneFeasibility scenario (test/test_feasibility.cpp:296-343) and rows of the
// reference's verdicts (tests/golden/reference_half_plane_veneer_rows.txt, written from reference_half_plane_n10_k8_d3_fast.npz).
//   test_half_plane_veneer <rows file> host      -- needs no device
//   test_half_plane_veneer <rows file> device    -- the batch form as well
#include <mav_trajectory_generation_ros/feasibility_base.h>

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
  std::vector<int> box_segment_feasible, oblique_segment_feasible;
  int box_feasible, oblique_feasible, box_first_segment, box_first_plane;
};

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;

  // ---- the reference's own scenario: N = 3, x = t, z = t^2, T = 1 ----
  {
    Eigen::VectorXd coeffs_x(3), coeffs_y(3), coeffs_z(3);
    coeffs_x(1) = 1;
    coeffs_z(2) = 1;
    Segment segment(3, 3);
    segment[0] = Polynomial(3, coeffs_x);
    segment[1] = Polynomial(3, coeffs_y);
    segment[2] = Polynomial(3, coeffs_z);
    segment.setTime(1.0);

    FeasibilityBase half_space_check;
    EXPECT(half_space_check.checkHalfPlaneFeasibility(segment));   // no planes: feasible
    Eigen::Vector3d point(0.0, 0.0, 0.0);
    Eigen::Vector3d normal(-1.0, 0.0, 1.0);
    int skipped = 0;
    while (point.z() > -1.0) {   // shift the boundary down
      half_space_check.half_plane_constraints_.emplace_back(point, normal);
      const bool feasible = half_space_check.checkHalfPlaneFeasibility(segment);
      if (std::fabs(-0.25 - point.z()) <= 1e-9) ++skipped;   // the exact clearance is (-1/4 - z) / sqrt 2
      else EXPECT(feasible == !(point.z() >= -0.25));
      half_space_check.half_plane_constraints_.clear();
      point.z() -= 0.05;
    }
    EXPECT(skipped <= 1);

    FeasibilityBase box_check;
    Eigen::Vector3d box_center(0.0, 0.0, 0.0);
    skipped = 0;
    double l = 0.0;
    while (l < 4.0) {   // grow the box
      box_check.half_plane_constraints_ = HalfPlane::createBoundingBox(box_center, Eigen::Vector3d::Constant(l));
      const bool feasible = box_check.checkHalfPlaneFeasibility(segment);
      if (std::fabs(l / 2.0 - 1.0) <= 1e-9) ++skipped;
      else EXPECT(feasible == !(l <= 2.0));
      l += 0.05;
    }
    EXPECT(skipped <= 1);

    // HalfPlane itself
    const HalfPlane hp(Eigen::Vector3d(1.0, 2.0, 3.0), Eigen::Vector3d(0.0, 3.0, 4.0));
    EXPECT(hp.normal(0) == 0.0 && std::fabs(hp.normal(1) - 0.6) < 1e-15 && std::fabs(hp.normal(2) - 0.8) < 1e-15);
    const HalfPlane through(Eigen::Vector3d(0.0, 0.0, 1.0), Eigen::Vector3d(2.0, 0.0, 1.0), Eigen::Vector3d(0.0, 5.0, 1.0));
    EXPECT(through.normal(0) == 0.0 && through.normal(1) == 0.0 && through.normal(2) == 1.0 && through.point(2) == 1.0);
    const HalfPlane::Vector box = HalfPlane::createBoundingBox(Eigen::Vector3d(1.0, -2.0, 0.5), Eigen::Vector3d(4.0, 6.0, 1.0));
    EXPECT(box.size() == 6);
    EXPECT(box[0].normal(0) == 1.0 && box[0].point(0) == -1.0 && box[1].normal(0) == -1.0 && box[1].point(0) == 3.0);
    EXPECT(box[2].normal(1) == 1.0 && box[2].point(1) == -5.0 && box[3].normal(1) == -1.0 && box[3].point(1) == 1.0);
    EXPECT(box[4].normal(2) == 1.0 && box[4].point(2) == 0.0 && box[5].normal(2) == -1.0 && box[5].point(2) == 1.0);
    EXPECT(!FeasibilityBase().checkHalfPlaneFeasibility(Segment(3, 2)));   // dimension 2: false, as the reference
  }

  // ---- rows of the reference's verdicts ----
  std::ifstream in(argv[1]);
  std::string line;
  std::getline(in, line);   // comment
  int N, K, D, n_rows;
  double edge;
  in >> N >> K >> D >> n_rows >> edge;
  double oblique[2][6];
  for (auto& pl : oblique)
    for (double& v : pl) in >> v;
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
    row.box_segment_feasible.resize(K);
    row.oblique_segment_feasible.resize(K);
    for (int& r : row.box_segment_feasible) in >> r;
    for (int& r : row.oblique_segment_feasible) in >> r;
    in >> row.box_feasible >> row.oblique_feasible >> row.box_first_segment >> row.box_first_plane;
  }
  EXPECT(!in.fail() && n_rows >= 2);

  FeasibilityBase box_check, oblique_check;
  box_check.half_plane_constraints_ = HalfPlane::createBoundingBox(Eigen::Vector3d::Zero(), Eigen::Vector3d::Constant(edge));
  for (const auto& pl : oblique)
    oblique_check.half_plane_constraints_.emplace_back(Eigen::Vector3d(pl[0], pl[1], pl[2]), Eigen::Vector3d(pl[3], pl[4], pl[5]));
  bool saw_feasible = false, saw_infeasible = false;
  std::vector<Trajectory> all;
  for (const Row& row : rows) {
    for (int k = 0; k < K; ++k) {
      EXPECT((int)box_check.checkHalfPlaneFeasibility(row.trajectory.segments()[k]) == row.box_segment_feasible[k]);
      EXPECT((int)oblique_check.checkHalfPlaneFeasibility(row.trajectory.segments()[k]) == row.oblique_segment_feasible[k]);
    }
    const bool feasible = box_check.checkHalfPlaneFeasibility(row.trajectory);
    EXPECT((int)feasible == row.box_feasible);
    EXPECT((int)oblique_check.checkHalfPlaneFeasibility(row.trajectory) == row.oblique_feasible);
    saw_feasible = saw_feasible || feasible;
    saw_infeasible = saw_infeasible || !feasible;
    all.push_back(row.trajectory);
  }
  EXPECT(saw_feasible && saw_infeasible);

  if (device) {
    TrajectoryBatch batch(all);
    std::vector<bool> feasible;
    std::vector<int> first_segment, first_plane;
    EXPECT(box_check.checkHalfPlaneFeasibilityBatch(batch, &feasible, &first_segment, &first_plane));
    EXPECT(feasible.size() == rows.size());
    for (size_t b = 0; b < rows.size() && b < feasible.size(); ++b) {
      EXPECT((int)feasible[b] == rows[b].box_feasible);
      EXPECT(first_segment[b] == rows[b].box_first_segment && first_plane[b] == rows[b].box_first_plane);
    }
  }
  if (failures == 0) std::printf("HALF-PLANE VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
