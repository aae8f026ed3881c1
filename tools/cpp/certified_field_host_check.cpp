// Stand-alone check of the certified distance-field check's HOST translation unit under the sanitizers (host code only; nothing
// here touches a device or is loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o certified_field_host_check \
//       certified_field_host_check.cpp ../../mav_trajectory_generation_amd/csrc/mtg_certify_host.cpp \
//       ../../mav_trajectory_generation_amd/csrc/mtg_field_host.cpp
//   ./certified_field_host_check [case.txt]
// It runs the hand-computed lines of tests/test_certified_field.py (fields linear in one axis, 8 x 6 x 4 voxels, h = 1), positions
// and segment times of +-1e300 and +-infinity (where an index error would read out of bounds), the three limits at their extremes
// (where a frontier index error would write out of bounds), the Lipschitz helper, and -- with a file written by
// tools/dump_certified_field_case.py -- one of the committed fixtures, whose outputs must equal the recorded ones of the library's
// own build bit for bit.
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
  int32_t result = -9, first_segment = -9, seg_result = -9, nodes = -9, depth = -9;
  double lower = -9.0, sampled = -9.0, closest_time = -9.0, failing_time = -9.0, traj_lower = -9.0, traj_sampled = -9.0;
};

// one segment p = a + v t (N = 2) over T
static Out run_line(const mtg_distance_field& f, const double (&a)[3], const double (&v)[3], double T, double lipschitz, double inflation,
                    int min_depth = 0, int max_depth = 16, int max_frontier = 1024, int* rc_out = nullptr) {
  // exactly sized heap buffers: a read or write past either end is the sanitizer's to find
  std::vector<double> c = {a[0], v[0], a[1], v[1], a[2], v[2]}, t = {T};
  Out o;
  const int rc = mtg_certify_distance_field_host(2, 1, 3, 1, c.data(), t.data(), 1, 1, &f, lipschitz, min_depth, max_depth, max_frontier,
                                                 inflation, &o.result, &o.first_segment, &o.seg_result, &o.lower, &o.sampled, &o.closest_time,
                                                 &o.failing_time, &o.nodes, &o.depth, &o.traj_lower, &o.traj_sampled);
  if (rc_out) *rc_out = rc;
  else EXPECT(rc == MTG_OK);
  return o;
}

int main(int argc, char** argv) {
  const double inf = std::numeric_limits<double>::infinity();
  for (int axis = 0; axis < 3; ++axis) {
    std::vector<float> grid((size_t)NX * NY * NZ);   // exactly sized
    for (int z = 0; z < NZ; ++z)
      for (int y = 0; y < NY; ++y)
        for (int x = 0; x < NX; ++x) grid[((size_t)z * NY + y) * NX + x] = (float)((axis + 1) * (axis == 0 ? x : axis == 1 ? y : z));
    mtg_distance_field f;
    mtg_distance_field_init(&f);
    f.distances = grid.data();
    f.nx = NX; f.ny = NY; f.nz = NZ;
    f.voxel_size = 1.0;
    f.outside_distance = inf;
    const double k = axis + 1.0, tiny = 1e-8 * k;
    double lip = 0.0;
    EXPECT(mtg_distance_field_lipschitz_host(&f, &lip) == MTG_OK && lip >= k && lip <= k * (1.0 + 1e-12));
    double a[3] = {1.0, 1.0, 1.0}, v[3] = {0.0, 0.0, 0.0};
    a[axis] = 3.0;
    v[axis] = -0.5;
    Out o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 2.0, k, k);                       // far from zero
    EXPECT(o.result == MTG_FIELD_FREE && o.nodes == 1 && o.depth == 0 && o.sampled == 1.5 * k && o.closest_time == 1.0);
    EXPECT(o.lower < k && o.lower >= k - tiny && std::isnan(o.failing_time) && o.first_segment == -1);
    v[axis] = -1.0;
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 2.0, k, k, 0, 6);                     // grazing zero at t = T
    EXPECT(o.result == MTG_FIELD_UNDECIDED_DEPTH && o.nodes == 13 && o.depth == 6 && o.sampled == k / 64.0 && o.lower < 0.0 && o.lower >= -tiny);
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 3.0, k, k);                           // crossing zero
    EXPECT(o.result == MTG_FIELD_COLLIDES && o.nodes == 3 && o.depth == 1 && o.failing_time == 2.25 && o.sampled == -0.25 * k);
    EXPECT(o.lower < -k && o.lower >= -k - tiny && o.first_segment == 0 && o.traj_sampled == -0.25 * k);
    // the limits at their extremes: 1 + 2 * 24 nodes; a full level of 1024; a budget of 2; a budget of 1024 that is passed
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 2.0, k, k, 0, 24, 2);
    EXPECT(o.result == MTG_FIELD_UNDECIDED_DEPTH && o.nodes == 49 && o.depth == 24);
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 2.0, k, k, 10, 10, 1024);
    EXPECT(o.result == MTG_FIELD_UNDECIDED_DEPTH && o.nodes == 1024 && o.depth == 10);
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 1.0, 1e6, k, 0, 16, 2);
    EXPECT(o.result == MTG_FIELD_UNDECIDED_BUDGET && o.nodes == 3 && o.depth == 1 && o.lower == -inf);
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 1.0, 1e6, k, 10, 24, 1024);
    EXPECT(o.result == MTG_FIELD_UNDECIDED_BUDGET && o.nodes == 1024 && o.depth == 10 && o.lower == -inf);
    o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, 1.0, 1e6, k, 0, 24, 1024);            // every level full up to 1024, then the budget
    EXPECT(o.result == MTG_FIELD_UNDECIDED_BUDGET && o.nodes == 2047 && o.depth == 10);
    // huge and non-finite positions, speeds and times: no index may follow from them
    const double wild[] = {1e300, -1e300, inf, -inf, std::nan("")};
    for (double x : wild) {
      double p[3] = {1.0, 1.0, 1.0}, s[3] = {0.0, 0.0, 0.0};
      p[axis] = x;
      o = run_line(f, {p[0], p[1], p[2]}, {0.0, 0.0, 0.0}, 1.0, k, k);
      // (a finite position far outside: the outside branch certifies it; an infinite one: an infinite reach scale, the bound is NaN and
      // nothing is ever certified; a NaN one fails its sample)
      EXPECT(o.nodes >= 1 && (std::isfinite(x) ? o.result == MTG_FIELD_FREE : x != x ? o.result == MTG_FIELD_COLLIDES : o.result == MTG_FIELD_UNDECIDED_BUDGET));
      s[axis] = x;
      o = run_line(f, {3.0, 1.0, 1.0}, {s[0], s[1], s[2]}, 1.0, k, 0.0, 0, 8, 16);
      EXPECT(o.nodes >= 1 && o.result != -9);
      o = run_line(f, {a[0], a[1], a[2]}, {v[0], v[1], v[2]}, x, k, k, 0, 8, 16);                 // as the segment time
      EXPECT(o.nodes >= 1 && (x > 0.0 || o.nodes == 1));
      f.outside_distance = x == x ? x : 0.0;
      o = run_line(f, {7.5, 1.0, 1.0}, {1.0, 0.5, 0.25}, 4.0, k, 0.0, 2, 8, 64);                  // leaves the grid through a corner
      EXPECT(o.nodes >= 4);
      f.outside_distance = inf;
    }
    // refused arguments
    int rc = 0;
    f.interpolation = MTG_FIELD_NEAREST;
    run_line(f, {3.0, 1.0, 1.0}, {0.0, 0.0, 0.0}, 1.0, k, 0.0, 0, 16, 1024, &rc);
    EXPECT(rc == MTG_ERR_INVALID_ARGUMENT);
    f.interpolation = MTG_FIELD_TRILINEAR;
    const int bad[][3] = {{-1, 16, 1024}, {11, 16, 1024}, {4, 3, 1024}, {4, 25, 1024}, {4, 16, 15}, {0, 16, 1}, {4, 16, 1025}};
    for (const auto& b : bad) {
      run_line(f, {3.0, 1.0, 1.0}, {0.0, 0.0, 0.0}, 1.0, k, 0.0, b[0], b[1], b[2], &rc);
      EXPECT(rc == MTG_ERR_INVALID_ARGUMENT);
    }
    for (double l : {0.0, -1.0, inf, std::nan("")}) {
      run_line(f, {3.0, 1.0, 1.0}, {0.0, 0.0, 0.0}, 1.0, l, 0.0, 0, 16, 1024, &rc);
      EXPECT(rc == MTG_ERR_INVALID_ARGUMENT);
    }
    grid[(size_t)(1 * NY + 2) * NX + 3] = std::nanf("");
    EXPECT(mtg_distance_field_lipschitz_host(&f, &lip) == MTG_OK && std::isnan(lip));
    o = run_line(f, {5.0, 2.0, 1.0}, {-1.0, 0.0, 0.0}, 4.0, k, 0.0);                              // the root samples the NaN voxel
    EXPECT(o.result == MTG_FIELD_COLLIDES && std::isnan(o.sampled) && std::isnan(o.lower) && o.failing_time == 2.0);
  }
  std::printf("hand cases: %s\n", failures ? "FAILED" : "ok");

  if (argc > 1) {   // a fixture with recorded outputs (tools/dump_certified_field_case.py)
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int N, K, D, B, min_depth, max_depth, max_frontier;
    mtg_distance_field f;
    mtg_distance_field_init(&f);
    double lipschitz, inflation;
    char word[32];
    bool ok = std::fscanf(in, "%d %d %d %d %d %d %d %lf %lf %lf %lf %31s %la %d %d %d %lf", &N, &K, &D, &B, &f.nx, &f.ny, &f.nz, &f.origin[0],
                          &f.origin[1], &f.origin[2], &f.voxel_size, word, &lipschitz, &min_depth, &max_depth, &max_frontier, &inflation) == 17;
    f.outside_distance = std::strcmp(word, "inf") == 0 ? inf : std::atof(word);
    std::vector<double> coeffs((size_t)B * K * D * N), times((size_t)B * K);
    std::vector<float> grid((size_t)f.nx * f.ny * f.nz);
    for (double& v : coeffs) ok = ok && std::fscanf(in, "%la", &v) == 1;
    for (double& v : times) ok = ok && std::fscanf(in, "%la", &v) == 1;
    for (float& v : grid) ok = ok && std::fscanf(in, "%a", &v) == 1;
    const size_t S = (size_t)B * K;
    std::vector<int32_t> want_i((size_t)2 * B + 3 * S);
    std::vector<unsigned long long> want_r(4 * S + (size_t)2 * B);
    for (int32_t& v : want_i) ok = ok && std::fscanf(in, "%d", &v) == 1;
    for (unsigned long long& v : want_r) ok = ok && std::fscanf(in, "%llx", &v) == 1;
    std::fclose(in);
    EXPECT(ok);
    if (ok) {
      f.distances = grid.data();
      double lip = 0.0;
      EXPECT(mtg_distance_field_lipschitz_host(&f, &lip) == MTG_OK && lip == lipschitz);
      std::vector<int32_t> got_i(want_i.size());
      std::vector<double> got_r(want_r.size());
      int32_t* p = got_i.data();
      double* q = got_r.data();
      EXPECT(mtg_certify_distance_field_host(N, K, D, B, coeffs.data(), times.data(), K, 1, &f, lipschitz, min_depth, max_depth, max_frontier,
                                             inflation, p, p + B, p + 2 * B, q, q + S, q + 2 * S, q + 3 * S, p + 2 * B + S, p + 2 * B + 2 * S,
                                             q + 4 * S, q + 4 * S + B) == MTG_OK);
      EXPECT(got_i == want_i);
      EXPECT(std::memcmp(got_r.data(), want_r.data(), sizeof(double) * want_r.size()) == 0);
      std::printf("fixture %s: %d x %d segments, %s\n", argv[1], B, K, failures ? "FAILED" : "ok");
    }
  }
  if (failures == 0) std::printf("CERTIFIED-FIELD HOST CHECK PASSED\n");
  return failures == 0 ? 0 : 1;
}
