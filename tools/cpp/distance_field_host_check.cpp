// Stand-alone check of the distance-field check's HOST translation unit under the sanitizers (host code only; nothing here touches
// a device or is loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o distance_field_host_check \
//       distance_field_host_check.cpp ../../mav_trajectory_generation_amd/csrc/mtg_field_host.cpp
//   ./distance_field_host_check [case.txt]
// It runs the hand-computed lines of tests/test_distance_field.py (fields linear in one axis, 8 x 6 x 4 voxels, h = 0.5, dt = 0.25:
// every number exact), the edges of the grid on every axis and side in both interpolation modes (where an index error would read
// out of bounds), segments with too many samples, and -- with a file written by tools/dump_distance_field_case.py -- one of the
// committed fixtures, whose outputs must equal the recorded ones of the library's own build bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mtg_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

constexpr int NX = 8, NY = 6, NZ = 4;

struct Out {
  int32_t feasible = -9, first_segment = -9, closest = -9, first_failing = -9, samples = -9;
  double seg_clearance = -9.0, clearance = -9.0;
};

// one segment p = a + v t (N = 2) over T
static Out run_line(const mtg_distance_field& f, const double (&a)[3], const double (&v)[3], double T, double dt, double inflation,
                    int max_samples = 4096, int* rc_out = nullptr) {
  // exactly sized heap buffers: a read or write past either end is the sanitizer's to find
  std::vector<double> c = {a[0], v[0], a[1], v[1], a[2], v[2]}, t = {T};
  Out o;
  const int rc = mtg_check_distance_field_host(2, 1, 3, 1, c.data(), t.data(), 1, 1, &f, dt, max_samples, inflation, &o.feasible,
                                               &o.first_segment, &o.seg_clearance, &o.closest, &o.first_failing, &o.samples, &o.clearance);
  if (rc_out) *rc_out = rc;
  else EXPECT(rc == MTG_OK);
  return o;
}

static double value_at(const mtg_distance_field& f, double x, double y, double z) {
  return run_line(f, {x, y, z}, {0.0, 0.0, 0.0}, 0.0, 0.25, 0.0).seg_clearance;
}

int main(int argc, char** argv) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int axis = 0; axis < 3; ++axis) {
    std::vector<float> grid((size_t)NX * NY * NZ);   // exactly sized
    for (int z = 0; z < NZ; ++z)
      for (int y = 0; y < NY; ++y)
        for (int x = 0; x < NX; ++x) grid[((size_t)z * NY + y) * NX + x] = 0.5f * (axis + 1) * (axis == 0 ? x : axis == 1 ? y : z);
    mtg_distance_field f;
    mtg_distance_field_init(&f);
    f.distances = grid.data();
    f.nx = NX; f.ny = NY; f.nz = NZ;
    f.voxel_size = 0.5;
    f.outside_distance = -7.0;
    const double k = axis + 1.0;
    const double pts[6][3] = {{0.0, 0.0, 0.0}, {1.0, 1.0, 0.5}, {1.125, 0.875, 0.625}, {3.5, 2.5, 1.5}, {3.375, 0.125, 1.375}, {3.5, 0.0, 1.5}};
    for (const auto& p : pts) EXPECT(value_at(f, p[0], p[1], p[2]) == k * p[axis]);
    // one ulp beyond every face: outside
    const double hi[3] = {3.5, 2.5, 1.5};
    for (int a = 0; a < 3; ++a) {
      double p[3] = {1.0, 1.0, 1.0};
      p[a] = std::nextafter(hi[a], inf);
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = std::nextafter(0.0, -inf);
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = 1e300;
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = -inf;
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = std::nan("");
      EXPECT(std::isnan(value_at(f, p[0], p[1], p[2])));
    }
    f.interpolation = MTG_FIELD_NEAREST;
    for (const auto& p : pts) EXPECT(value_at(f, p[0], p[1], p[2]) == k * 0.5 * std::floor(p[axis] / 0.5 + 0.5));
    for (int a = 0; a < 3; ++a) {
      double p[3] = {1.0, 1.0, 1.0};
      p[a] = std::nextafter(hi[a] + 0.25, 0.0);
      EXPECT(value_at(f, p[0], p[1], p[2]) == k * (a == axis ? hi[a] : 1.0));
      p[a] = hi[a] + 0.25;
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = -0.25;
      EXPECT(value_at(f, p[0], p[1], p[2]) == k * (a == axis ? 0.0 : 1.0));
      p[a] = std::nextafter(-0.25, -inf);
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
      p[a] = -1e300;
      EXPECT(value_at(f, p[0], p[1], p[2]) == -7.0);
    }
    f.interpolation = MTG_FIELD_TRILINEAR;
    if (axis == 0) {
      Out o = run_line(f, {2.0, 1.0, 0.5}, {-0.5, 0.0, 0.0}, 3.0, 0.25, 1.0);
      EXPECT(o.samples == 13 && o.seg_clearance == -0.5 && o.closest == 12 && o.first_failing == 8 && o.feasible == 0 && o.first_segment == 0);
      o = run_line(f, {2.0, 1.0, 0.5}, {-0.5, 0.0, 0.0}, 1.75, 0.25, 1.0);
      EXPECT(o.samples == 8 && o.seg_clearance == 0.125 && o.closest == 7 && o.first_failing == -1 && o.feasible == 1 && o.first_segment == -1);
      o = run_line(f, {2.0, 1.0, 0.5}, {-0.5, 0.0, 0.0}, 3.0, 0.25, 1.0, 12);
      EXPECT(o.samples == -1 && std::isnan(o.seg_clearance) && o.closest == -1 && o.first_failing == -1 && o.feasible == 0);
      o = run_line(f, {2.0, 1.0, 0.5}, {0.0, 0.0, 0.0}, 1e300, 1.0, 0.0);
      EXPECT(o.samples == -1 && o.feasible == 0 && std::isnan(o.clearance));
      o = run_line(f, {2.0, 1.0, 0.5}, {0.0, 0.0, 0.0}, 0.25 * ((1 << 20) - 2), 0.25, 0.0, 1 << 20);
      EXPECT(o.samples == (1 << 20) - 1 && o.feasible == 1 && o.clearance == 2.0);
      o = run_line(f, {2.0, 1.0, 0.5}, {1.0, 0.0, 0.0}, std::nan(""), 0.25, 0.0);
      EXPECT(o.samples == 2 && std::isnan(o.seg_clearance) && o.closest == 1 && o.feasible == 0);
      int rc = 0;
      run_line(f, {2.0, 1.0, 0.5}, {0.0, 0.0, 0.0}, 1.0, 0.0, 0.0, 4096, &rc);
      EXPECT(rc == MTG_ERR_INVALID_ARGUMENT);
      run_line(f, {2.0, 1.0, 0.5}, {0.0, 0.0, 0.0}, 1.0, 0.25, 0.0, 1, &rc);
      EXPECT(rc == MTG_ERR_INVALID_ARGUMENT);
    }
  }
  std::printf("hand cases: %s\n", failures ? "FAILED" : "ok");

  if (argc > 1) {   // a fixture with recorded outputs (tools/dump_distance_field_case.py)
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int N, K, D, B, max_samples;
    mtg_distance_field f;
    mtg_distance_field_init(&f);
    double dt, inflation;
    char word[32];
    bool ok = std::fscanf(in, "%d %d %d %d %d %d %d %lf %lf %lf %lf %31s %d %lf %d %lf", &N, &K, &D, &B, &f.nx, &f.ny, &f.nz, &f.origin[0],
                          &f.origin[1], &f.origin[2], &f.voxel_size, word, &f.interpolation, &dt, &max_samples, &inflation) == 16;
    f.outside_distance = std::strcmp(word, "inf") == 0 ? inf : std::atof(word);
    std::vector<double> coeffs((size_t)B * K * D * N), times((size_t)B * K);
    std::vector<float> grid((size_t)f.nx * f.ny * f.nz);
    for (double& v : coeffs) ok = ok && std::fscanf(in, "%la", &v) == 1;
    for (double& v : times) ok = ok && std::fscanf(in, "%la", &v) == 1;
    for (float& v : grid) ok = ok && std::fscanf(in, "%a", &v) == 1;
    std::vector<int32_t> want_i((size_t)2 * B + (size_t)3 * B * K);
    std::vector<double> want_c((size_t)B * K);
    for (int32_t& v : want_i) ok = ok && std::fscanf(in, "%d", &v) == 1;
    for (double& v : want_c) ok = ok && std::fscanf(in, "%la", &v) == 1;
    std::fclose(in);
    EXPECT(ok);
    if (ok) {
      f.distances = grid.data();
      std::vector<int32_t> got_i(want_i.size());
      std::vector<double> got_c(want_c.size()), traj((size_t)B);
      int32_t* p = got_i.data();
      EXPECT(mtg_check_distance_field_host(N, K, D, B, coeffs.data(), times.data(), K, 1, &f, dt, max_samples, inflation, p, p + B,
                                           got_c.data(), p + 2 * B, p + 2 * B + B * K, p + 2 * B + 2 * B * K, traj.data()) == MTG_OK);
      EXPECT(got_i == want_i);
      EXPECT(std::memcmp(got_c.data(), want_c.data(), sizeof(double) * want_c.size()) == 0);
      std::printf("fixture %s: %d x %d segments, %s\n", argv[1], B, K, failures ? "FAILED" : "ok");
    }
  }
  if (failures == 0) std::printf("DISTANCE-FIELD HOST CHECK PASSED\n");
  return failures == 0 ? 0 : 1;
}
