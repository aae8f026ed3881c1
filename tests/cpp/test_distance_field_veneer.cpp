// The distance-field check of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCheckDistanceField(Trajectory) on the library's host entry and TrajectoryBatch::checkDistanceField on the device entry, on
// straight lines through fields that are linear in one axis (origin 0, h = 0.5, dt = 0.25, an 8 x 6 x 4 grid: every number is exact
// and the answers are known by hand, as in tests/test_distance_field.py).
//   test_distance_field_veneer host      -- needs no device
//   test_distance_field_veneer device    -- the batch form as well
#include <mav_trajectory_generation/trajectory_batch.h>

#include <cmath>
#include <cstdio>
#include <cstring>
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
      for (int x = 0; x < NX; ++x) g[((size_t)z * NY + y) * NX + x] = 0.5f * (axis + 1) * (axis == 0 ? x : axis == 1 ? y : z);
  return g;
}

static mtg_distance_field field_of(const std::vector<float>& grid, double outside = -7.0, int interpolation = MTG_FIELD_TRILINEAR) {
  mtg_distance_field f;
  mtg_distance_field_init(&f);
  EXPECT(f.interpolation == MTG_FIELD_TRILINEAR && f.outside_distance == 0.0 && f.distances == nullptr && f.nx == 0);
  f.distances = grid.data();
  f.nx = NX; f.ny = NY; f.nz = NZ;
  f.voxel_size = 0.5;
  f.outside_distance = outside;
  f.interpolation = interpolation;
  return f;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[1], "device") == 0;
  const std::vector<float> gx = linear_grid(0), gy = linear_grid(1), gz = linear_grid(2);
  const mtg_distance_field fx = field_of(gx), fy = field_of(gy), fz = field_of(gz);

  std::vector<Trajectory> all;
  std::vector<int> want_feasible, want_segment;
  std::vector<double> want_clearance;
  int first_segment = 7;
  double first_time = 7.0, clearance = 7.0;
  // d = x along (2 - t / 2, 1, 0.5), T = 3, inflation 1: x - 1 fails first at t = 2 (sample 8), lowest at the end, -0.5
  all.push_back(line({2.0, 1.0, 0.5}, {-0.5, 0.0, 0.0}, 3.0));
  EXPECT(!mtgCheckDistanceField(all.back(), fx, 0.25, 1.0, &first_segment, &first_time, &clearance));
  EXPECT(first_segment == 0 && first_time == 2.0 && clearance == -0.5);
  want_feasible.push_back(0); want_segment.push_back(0); want_clearance.push_back(-0.5);
  // the same line over T = 1.75 ends at x = 1.125: clear by 0.125 at the last sample
  all.push_back(line({2.0, 1.0, 0.5}, {-0.5, 0.0, 0.0}, 1.75));
  EXPECT(mtgCheckDistanceField(all.back(), fx, 0.25, 1.0, &first_segment, &first_time, &clearance));
  EXPECT(first_segment == -1 && first_time != first_time && clearance == 0.125);
  want_feasible.push_back(1); want_segment.push_back(-1); want_clearance.push_back(0.125);
  // the last centre of every axis (f = 1 in the last cell), reached at T: x = 3.5 is clear by 2.5
  all.push_back(line({3.0, 2.0, 1.0}, {0.5, 0.5, 0.5}, 1.0));
  EXPECT(mtgCheckDistanceField(all.back(), fx, 0.25, 1.0, &first_segment, &first_time, &clearance));
  EXPECT(clearance == 2.0);       // x = 3 at t = 0
  want_feasible.push_back(1); want_segment.push_back(-1); want_clearance.push_back(2.0);
  // one step beyond the last centre: the last sample (t = 1.25, x = 3.625) is outside the grid and takes -7 - 1
  all.push_back(line({3.0, 2.0, 1.0}, {0.5, 0.0, 0.0}, 1.25));
  EXPECT(!mtgCheckDistanceField(all.back(), fx, 0.25, 1.0, &first_segment, &first_time, &clearance));
  EXPECT(first_segment == 0 && first_time == 1.25 && clearance == -8.0);
  want_feasible.push_back(0); want_segment.push_back(0); want_clearance.push_back(-8.0);
  // the other two fields on a diagonal: d = 2 y on (0.5 + t, 0.25 + t / 2, t / 4) is lowest at t = 0 (0.5), d = 3 z there 0
  const Trajectory diagonal = line({0.5, 0.25, 0.0}, {1.0, 0.5, 0.25}, 1.0);
  EXPECT(mtgCheckDistanceField(diagonal, fy, 0.25, 0.0, &first_segment, &first_time, &clearance) && clearance == 0.5);
  EXPECT(!mtgCheckDistanceField(diagonal, fz, 0.25, 0.0, &first_segment, &first_time, &clearance) && clearance == 0.0 && first_time == 0.0);
  EXPECT(mtgCheckDistanceField(diagonal, fz, 0.25, 0.0) == false);
  // nearest: (1.125, 0.875, 0.625) is voxel (2, 2, 1): 1, 2, 1.5
  {
    const Trajectory rest = line({1.125, 0.875, 0.625}, {0.0, 0.0, 0.0}, 0.5);
    const mtg_distance_field nx = field_of(gx, -7.0, MTG_FIELD_NEAREST), ny = field_of(gy, -7.0, MTG_FIELD_NEAREST),
                             nz = field_of(gz, -7.0, MTG_FIELD_NEAREST);
    EXPECT(mtgCheckDistanceField(rest, nx, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 1.0);
    EXPECT(mtgCheckDistanceField(rest, ny, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 2.0);
    EXPECT(mtgCheckDistanceField(rest, nz, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 1.5);
    EXPECT(mtgCheckDistanceField(rest, fx, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 1.125);
    EXPECT(mtgCheckDistanceField(rest, fy, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 1.75);
    EXPECT(mtgCheckDistanceField(rest, fz, 0.25, 0.0, nullptr, nullptr, &clearance) && clearance == 1.875);
  }
  // the cap on samples: T = 3 has 13 samples
  EXPECT(!mtgCheckDistanceField(all[0], fx, 0.25, 0.0, &first_segment, &first_time, &clearance, 12));
  EXPECT(first_segment == 0 && first_time != first_time && clearance != clearance);
  EXPECT(mtgCheckDistanceField(all[0], fx, 0.25, 0.0, &first_segment, &first_time, &clearance, 13) && clearance == 0.5);
  // refused arguments
  EXPECT(!mtgCheckDistanceField(all[1], fx, 0.0, 0.0, &first_segment, &first_time, &clearance));
  EXPECT(first_segment == -1 && first_time != first_time && clearance != clearance);
  EXPECT(!mtgCheckDistanceField(all[1], fx, 0.25, -1.0));
  mtg_distance_field bad = fx;
  bad.voxel_size = 0.0;
  EXPECT(!mtgCheckDistanceField(all[1], bad, 0.25, 0.0));
  bad = fx;
  bad.interpolation = 2;
  EXPECT(!mtgCheckDistanceField(all[1], bad, 0.25, 0.0));
  bad = fx;
  bad.distances = nullptr;
  EXPECT(!mtgCheckDistanceField(all[1], bad, 0.25, 0.0));

  if (device) {
    TrajectoryBatch batch(all);
    DeviceDistanceField on_device(fx);
    std::vector<char> feasible;
    std::vector<int> segment;
    std::vector<double> lowest;
    EXPECT(batch.checkDistanceField(on_device.field(), 0.25, 1.0, &feasible, &segment, &lowest));
    EXPECT(feasible.size() == all.size() && segment.size() == all.size() && lowest.size() == all.size());
    for (size_t b = 0; b < all.size() && b < feasible.size(); ++b)
      EXPECT((int)feasible[b] == want_feasible[b] && segment[b] == want_segment[b] && lowest[b] == want_clearance[b]);
    EXPECT(batch.checkDistanceField(on_device.field(), 0.25, 1.0, &feasible, nullptr, nullptr, 12));
    EXPECT(feasible.size() == all.size() && !feasible[0] && feasible[1]);        // (13 samples in trajectory 0 only)
    EXPECT(!batch.checkDistanceField(on_device.field(), 0.0, 1.0, &feasible));
    EXPECT(!batch.checkDistanceField(on_device.field(), 0.25, -1.0, &feasible));
    mtg_distance_field refused = on_device.field();
    refused.nx = 1;
    EXPECT(!batch.checkDistanceField(refused, 0.25, 1.0, &feasible));
  }
  if (failures == 0) std::printf("DISTANCE-FIELD VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
