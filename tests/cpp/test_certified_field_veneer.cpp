// The certified distance-field check of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCertifyDistanceField(Trajectory) on the library's host entry and TrajectoryBatch::certifyDistanceField on the device entry, on
// straight lines through fields that are linear in one axis (origin 0, h = 1, an 8 x 6 x 4 grid, inflation = the slope: the answers
// are known by hand, as in tests/test_certified_field.py).
//   test_certified_field_veneer host      -- needs no device
//   test_certified_field_veneer device    -- the batch form as well
#include <mav_trajectory_generation/trajectory_batch.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace mav_trajectory_generation;

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

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

constexpr int NX = 8, NY = 6, NZ = 4;

// d = x, 2 y or 3 z
static std::vector<float> linear_grid(int axis) {
  std::vector<float> g((size_t)NX * NY * NZ);
  for (int z = 0; z < NZ; ++z)
    for (int y = 0; y < NY; ++y)
      for (int x = 0; x < NX; ++x) g[((size_t)z * NY + y) * NX + x] = (float)((axis + 1) * (axis == 0 ? x : axis == 1 ? y : z));
  return g;
}

static mtg_distance_field field_of(const std::vector<float>& grid, double outside) {
  mtg_distance_field f;
  mtg_distance_field_init(&f);
  f.distances = grid.data();
  f.nx = NX; f.ny = NY; f.nz = NZ;
  f.voxel_size = 1.0;
  f.outside_distance = outside;
  return f;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[1], "device") == 0;
  const double inf = std::numeric_limits<double>::infinity();
  const std::vector<float> gx = linear_grid(0), gy = linear_grid(1), gz = linear_grid(2);
  const mtg_distance_field fx = field_of(gx, inf), fy = field_of(gy, inf), fz = field_of(gz, inf);
  double lip = 0.0;
  EXPECT(mtg_distance_field_lipschitz_host(&fz, &lip) == MTG_OK && lip >= 3.0 && lip < 3.0 + 1e-11);

  std::vector<Trajectory> all;
  std::vector<int> want_result, want_segment;
  std::vector<double> want_sampled;
  int first_segment = 7;
  double first_time = 7.0, lower = 7.0, sampled = 7.0;
  // d = x, inflation 1, along x = 3 - t / 2 over T = 2: ends at x = 2, clear by 1 everywhere; min_depth 0: the root certifies it
  all.push_back(line({3.0, 1.0, 1.0}, {-0.5, 0.0, 0.0}, 2.0));
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, &first_segment, &first_time, &lower, &sampled, 0) == MTG_FIELD_FREE);
  EXPECT(first_segment == -1 && first_time != first_time && lower < 1.0 && lower > 1.0 - 1e-8 && sampled == 1.5);
  // (with the default min_depth of 4 the lowest sample is the last of the sixteen, at t = 2 - 1 / 16)
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, nullptr, nullptr, &lower, &sampled) == MTG_FIELD_FREE && sampled == 1.0 + 1.0 / 32.0);
  EXPECT(lower < 1.0 && lower > 1.0 - 1e-8);
  want_result.push_back(MTG_FIELD_FREE); want_segment.push_back(-1); want_sampled.push_back(1.0 + 1.0 / 32.0);
  // x = 3 - t over T = 3 crosses x = 1 at t = 2: collides; the lower bound is the true minimum -1 less the slack
  all.push_back(line({3.0, 1.0, 1.0}, {-1.0, 0.0, 0.0}, 3.0));
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, &first_segment, &first_time, &lower, &sampled, 0) == MTG_FIELD_COLLIDES);
  EXPECT(first_segment == 0 && first_time == 2.25 && sampled == -0.25 && lower < -1.0 && lower > -1.0 - 1e-8);
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, &first_segment, &first_time, &lower, &sampled) == MTG_FIELD_COLLIDES);
  // (16 nodes of half-width 3 / 32: the one around t = 2 (m = 63 / 32) splits, its second child m = 129 / 64 fails: the earliest failing
  // sample; the lowest sample is the last of the sixteen)
  EXPECT(first_segment == 0 && first_time == 129.0 / 64.0 && sampled == -1.0 + 3.0 / 32.0);
  want_result.push_back(MTG_FIELD_COLLIDES); want_segment.push_back(0); want_sampled.push_back(-1.0 + 3.0 / 32.0);
  // x = 3 - t over T = 2 grazes x = 1 at t = T: undecided at any depth
  all.push_back(line({3.0, 1.0, 1.0}, {-1.0, 0.0, 0.0}, 2.0));
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, &first_segment, &first_time, &lower, &sampled, 0, 6) == MTG_FIELD_UNDECIDED_DEPTH);
  EXPECT(first_segment == 0 && first_time != first_time && sampled == 1.0 / 64.0 && lower < 0.0 && lower > -1e-8);
  EXPECT(mtgCertifyDistanceField(all.back(), fx, 1.0, 1.0, nullptr, nullptr, nullptr, &sampled) == MTG_FIELD_UNDECIDED_DEPTH && sampled == std::ldexp(1.0, -16));
  want_result.push_back(MTG_FIELD_UNDECIDED_DEPTH); want_segment.push_back(0); want_sampled.push_back(std::ldexp(1.0, -16));
  // a constant far too large for the clearance: nothing is certified and the budget stops it
  EXPECT(mtgCertifyDistanceField(all[0], fx, 1e6, 1.0, &first_segment, nullptr, &lower, nullptr, 0, 16, 2) == MTG_FIELD_UNDECIDED_BUDGET);
  EXPECT(first_segment == 0 && lower == -inf);
  // the other two fields, with the constant computed from the grid (lipschitz <= 0): an axis mix-up cannot pass
  const Trajectory along_y = line({1.0, 3.0, 1.0}, {0.0, -0.5, 0.0}, 2.0), along_z = line({1.0, 1.0, 3.0}, {0.0, 0.0, -0.5}, 2.0);
  EXPECT(mtgCertifyDistanceField(along_y, fy, 0.0, 2.0, nullptr, nullptr, &lower, &sampled, 0) == MTG_FIELD_FREE && sampled == 3.0);
  EXPECT(lower < 2.0 && lower > 2.0 - 1e-8);
  EXPECT(mtgCertifyDistanceField(along_z, fz, 0.0, 3.0, nullptr, nullptr, &lower, &sampled, 0) == MTG_FIELD_FREE && sampled == 4.5);
  EXPECT(lower < 3.0 && lower > 3.0 - 1e-8);
  EXPECT(mtgCertifyDistanceField(along_y, fz, 0.0, 3.0, nullptr, nullptr, nullptr, &sampled, 0) == MTG_FIELD_COLLIDES && sampled == 0.0);
  // leaving the grid: free where unknown space is free, colliding where it is an obstacle
  const Trajectory leaves = line({6.0, 1.0, 1.0}, {1.0, 0.0, 0.0}, 3.0);
  EXPECT(mtgCertifyDistanceField(leaves, fx, 1.0, 0.0, nullptr, nullptr, &lower, nullptr, 0) == MTG_FIELD_FREE && lower < 5.5 && lower > 5.5 - 1e-8);
  const mtg_distance_field closed = field_of(gx, 0.0);
  EXPECT(mtgCertifyDistanceField(leaves, closed, 1.0, 0.0, &first_segment, &first_time, nullptr, nullptr, 0) == MTG_FIELD_COLLIDES && first_time == 1.5);
  // refused arguments
  mtg_distance_field bad = fx;
  bad.interpolation = MTG_FIELD_NEAREST;
  EXPECT(mtgCertifyDistanceField(all[0], bad, 1.0, 1.0, &first_segment, &first_time, &lower, &sampled) == -1);
  EXPECT(first_segment == -1 && first_time != first_time && lower != lower && sampled != sampled);
  EXPECT(mtgCertifyDistanceField(all[0], fx, inf, 1.0) == -1);
  EXPECT(mtgCertifyDistanceField(all[0], fx, 1.0, -1.0) == -1);
  EXPECT(mtgCertifyDistanceField(all[0], fx, 1.0, 1.0, nullptr, nullptr, nullptr, nullptr, 11) == -1);
  EXPECT(mtgCertifyDistanceField(all[0], fx, 1.0, 1.0, nullptr, nullptr, nullptr, nullptr, 4, 3) == -1);
  EXPECT(mtgCertifyDistanceField(all[0], fx, 1.0, 1.0, nullptr, nullptr, nullptr, nullptr, 4, 16, 15) == -1);
  bad = fx;
  bad.distances = nullptr;
  EXPECT(mtgCertifyDistanceField(all[0], bad, 0.0, 1.0) == -1);

  if (device) {
    TrajectoryBatch batch(all);
    DeviceDistanceField on_device(fx);
    std::vector<int> result, segment;
    std::vector<double> lowest, lowest_sample;
    EXPECT(batch.certifyDistanceField(on_device.field(), 1.0, 1.0, &result, &segment, &lowest, &lowest_sample));
    EXPECT(result.size() == all.size() && segment.size() == all.size() && lowest.size() == all.size() && lowest_sample.size() == all.size());
    for (size_t b = 0; b < all.size() && b < result.size(); ++b) {
      double host_lower = 0.0;
      mtgCertifyDistanceField(all[b], fx, 1.0, 1.0, nullptr, nullptr, &host_lower);
      EXPECT(result[b] == want_result[b] && segment[b] == want_segment[b] && lowest_sample[b] == want_sampled[b] && lowest[b] == host_lower);
    }
    EXPECT(batch.certifyDistanceField(on_device.field(), 1e6, 1.0, &result, nullptr, &lowest, nullptr, 0, 16, 2));
    EXPECT(result.size() == all.size() && result[0] == MTG_FIELD_UNDECIDED_BUDGET && result[1] == MTG_FIELD_COLLIDES && lowest[0] == -inf);
    EXPECT(!batch.certifyDistanceField(on_device.field(), 0.0, 1.0, &result));
    EXPECT(!batch.certifyDistanceField(on_device.field(), 1.0, -1.0, &result));
    EXPECT(!batch.certifyDistanceField(on_device.field(), 1.0, 1.0, &result, nullptr, nullptr, nullptr, 4, 25));
    mtg_distance_field refused = on_device.field();
    refused.interpolation = MTG_FIELD_NEAREST;
    EXPECT(!batch.certifyDistanceField(refused, 1.0, 1.0, &result));
  }
  if (failures == 0) std::printf("CERTIFIED-FIELD VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
