// The distance-field collision cost of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
// mtgCollisionCost(Trajectory) on the library's host entry and TrajectoryBatch::collisionCost / mtgCollisionCost(TrajectoryBatch,
// DeviceDistanceField) on the device entry, on straight constant-speed lines through fields that are linear in one axis (origin 0,
// h = 0.5, dt = 0.5, an 8 x 6 x 4 grid, epsilon 1, inflation 0.25, speed_epsilon 0: every number is a small dyadic rational and
// the answers are known by hand, as in tests/test_collision_cost.py).
//   test_collision_cost_veneer host      -- needs no device
//   test_collision_cost_veneer device    -- the batch form as well
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

constexpr int N = 4, NX = 8, NY = 6, NZ = 4;

// p(t) = a + v t over T as a one-segment trajectory
static Trajectory line(const double (&a)[3], const double (&v)[3], double T) {
  Segment segment(N, 3);
  for (int d = 0; d < 3; ++d) {
    Eigen::VectorXd c(N);
    c.setZero();
    c(0) = a[d];
    c(1) = v[d];
    segment[d] = Polynomial(N, c);
  }
  segment.setTime(T);
  Trajectory trajectory;
  trajectory.setSegments(Segment::Vector(1, segment));
  return trajectory;
}

// d = x, 2 y or 3 z
static std::vector<float> linear_grid(int axis) {
  std::vector<float> g((size_t)NX * NY * NZ);
  for (int z = 0; z < NZ; ++z)
    for (int y = 0; y < NY; ++y)
      for (int x = 0; x < NX; ++x) g[((size_t)z * NY + y) * NX + x] = 0.5f * (axis + 1) * (axis == 0 ? x : axis == 1 ? y : z);
  return g;
}

static mtg_distance_field field_of(const std::vector<float>& grid) {
  mtg_distance_field f;
  mtg_distance_field_init(&f);
  f.distances = grid.data();
  f.nx = NX; f.ny = NY; f.nz = NZ;
  f.voxel_size = 0.5;
  f.outside_distance = 4.0;
  return f;
}

// the cost and the gradient [3][N] of p = a + (speed, 0, 0) t over T with dt = 0.5 (T a multiple of it) in the field
// d = (axis + 1) p_axis, epsilon 1, inflation 0.25, speed_epsilon 0, written out sample by sample
static double by_hand(const double (&a)[3], double speed, double T, int axis, double (&grad)[3][N]) {
  const int S = (int)(T / 0.5) + 1;
  double cost = 0.0;
  for (int d = 0; d < 3; ++d)
    for (int j = 0; j < N; ++j) grad[d][j] = 0.0;
  for (int i = 0; i < S; ++i) {
    const double t = 0.5 * i, w = (i == 0 || i == S - 1) ? 0.25 : 0.5;
    const double p[3] = {a[0] + speed * t, a[1], a[2]};
    const double x = (axis + 1) * p[axis] - 0.25;
    const double c = x < 0 ? 0.5 - x : x <= 1.0 ? (x - 1.0) * (x - 1.0) / 2.0 : 0.0;
    const double dc = x < 0 ? -1.0 : x <= 1.0 ? x - 1.0 : 0.0;
    cost += w * c * speed;
    double pw = 1.0, below = 0.0;      // t^j and j t^(j-1)
    for (int j = 0; j < N; ++j) {
      grad[axis][j] += w * dc * speed * (axis + 1) * pw;
      grad[0][j] += w * c * below;      // v / s = (1, 0, 0)
      below = (j + 1) * pw;
      pw *= t;
    }
  }
  return cost;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[1], "device") == 0;
  std::vector<std::vector<float>> grids = {linear_grid(0), linear_grid(1), linear_grid(2)};
  const double starts[3][3] = {{0.5, 0.5, 0.25}, {0.25, 0.125, 0.125}, {1.0, 0.375, 0.0625}};
  const double lengths[3] = {2.0, 1.5, 1.0};
  std::vector<Trajectory> all;
  for (int l = 0; l < 3; ++l) all.push_back(line(starts[l], {0.5, 0.0, 0.0}, lengths[l]));

  for (int axis = 0; axis < 3; ++axis) {
    const mtg_distance_field f = field_of(grids[axis]);
    std::vector<double> want_cost;
    std::vector<std::vector<double>> want_grad;
    for (int l = 0; l < 3; ++l) {
      double grad[3][N];
      const double cost = by_hand(starts[l], 0.5, lengths[l], axis, grad);
      want_cost.push_back(cost);
      want_grad.emplace_back(&grad[0][0], &grad[0][0] + 3 * N);
      std::vector<double> g, seg;
      EXPECT(mtgCollisionCost(all[l], f, 0.5, 0.25, 1.0, 0.0, &g, &seg) == cost);
      EXPECT(seg.size() == 1 && seg[0] == cost && g == want_grad.back());
      EXPECT(mtgCollisionCost(all[l], f, 0.5, 0.25, 1.0, 0.0) == cost);     // (cost only)
    }
    EXPECT(want_cost[0] > 0.0);
    if (device) {
      TrajectoryBatch batch(all);
      DeviceDistanceField on_device(f);
      std::vector<double> cost, grad, seg;
      EXPECT(mtgCollisionCost(batch, on_device, 0.5, 0.25, 1.0, 0.0, &cost, &grad, &seg));
      EXPECT(cost == want_cost && seg == want_cost && grad.size() == 3 * 3 * N);
      for (size_t b = 0; b < 3 && grad.size() == 3 * 3 * N; ++b)
        EXPECT(std::vector<double>(grad.begin() + b * 3 * N, grad.begin() + (b + 1) * 3 * N) == want_grad[b]);
      std::vector<double> cost_only;
      EXPECT(batch.collisionCost(on_device.field(), 0.5, 0.25, 1.0, 0.0, &cost_only) && cost_only == want_cost);
      // the cap: T = 2 has 5 samples
      EXPECT(batch.collisionCost(on_device.field(), 0.5, 0.25, 1.0, 0.0, &cost, nullptr, nullptr, 4));
      EXPECT(cost.size() == 3 && cost[0] != cost[0] && cost[1] == want_cost[1]);
      // refused arguments
      EXPECT(!batch.collisionCost(on_device.field(), 0.5, 0.25, 0.0, 0.0, &cost));
      EXPECT(!batch.collisionCost(on_device.field(), 0.5, 0.25, 1.0, -1.0, &cost));
      mtg_distance_field nearest = on_device.field();
      nearest.interpolation = MTG_FIELD_NEAREST;
      EXPECT(!batch.collisionCost(nearest, 0.5, 0.25, 1.0, 0.0, &cost));
    }
  }
  // the host form: the cap and refused arguments
  const mtg_distance_field fx = field_of(grids[0]);
  std::vector<double> g, seg;
  double cost = mtgCollisionCost(all[0], fx, 0.5, 0.25, 1.0, 0.0, &g, &seg, 4);
  EXPECT(cost != cost && seg.size() == 1 && seg[0] != seg[0] && g.size() == 3 * N && g[0] != g[0]);
  cost = mtgCollisionCost(all[0], fx, 0.5, 0.25, 0.0, 0.0, &g, &seg);
  EXPECT(cost != cost && g.empty() && seg.empty());
  mtg_distance_field nearest = fx;
  nearest.interpolation = MTG_FIELD_NEAREST;
  cost = mtgCollisionCost(all[0], nearest, 0.5, 0.25, 1.0);
  EXPECT(cost != cost);
  cost = mtgCollisionCost(all[0], fx, 0.5, 0.25, 1.0, -1.0);
  EXPECT(cost != cost);
  if (failures == 0) std::printf("COLLISION-COST VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
