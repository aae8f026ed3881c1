// TrajectoryBatch::softConstraintCost of the compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h) against
// the library's host entry on the same trajectories and against rows of the reference's own maxima and soft cost
// (tests/golden/reference_time_objective_veneer_rows.txt: the coefficients are the reference's own).
//   test_objective_veneer <rows file> host      -- the host entry against the rows; needs no device
//   test_objective_veneer <rows file> device    -- the batch form as well
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

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: %s <rows file> host|device\n", argv[0]); return 2; }
  const bool device = std::strcmp(argv[2], "device") == 0;
  std::ifstream in(argv[1]);
  std::string line;
  std::getline(in, line);   // comment
  int N, K, D, n_rows, n_con;
  in >> N >> K >> D >> n_rows >> n_con;
  std::vector<std::pair<int, double>> constraints(n_con);
  for (auto& c : constraints) in >> c.first >> c.second;
  double weight, maximum_cost;
  in >> weight >> maximum_cost;
  std::vector<double> times((size_t)n_rows * K), coeffs((size_t)n_rows * K * D * N), ref_max((size_t)n_rows * n_con), ref_cost(n_rows);
  std::vector<Trajectory> all(n_rows);
  for (int b = 0; b < n_rows; ++b) {
    for (int k = 0; k < K; ++k) in >> times[(size_t)b * K + k];
    Segment::Vector segments(K, Segment(N, D));
    for (int k = 0; k < K; ++k) {
      segments[k].setTime(times[(size_t)b * K + k]);
      for (int d = 0; d < D; ++d) {
        Eigen::VectorXd c(N);
        for (int n = 0; n < N; ++n) {
          in >> c[n];
          coeffs[(((size_t)b * K + k) * D + d) * N + n] = c[n];
        }
        segments[k][d] = Polynomial(N, c);
      }
    }
    all[b].setSegments(segments);
    for (int q = 0; q < n_con; ++q) in >> ref_max[(size_t)b * n_con + q];
    in >> ref_cost[b];
  }
  EXPECT(!in.fail() && n_rows >= 2 && n_con >= 1 && n_con <= MTG_MAX_MAGNITUDE_CONSTRAINTS);

  mtg_time_objective_params params;
  mtg_time_objective_params_init(&params);
  EXPECT(params.time_penalty == 500.0 && params.soft_constraint_weight == 100.0 && params.maximum_cost == 1.0e12 &&
         params.use_soft_constraints == 1 && params.n_constraints == 0 && params.time_cost_kind == MTG_TIME_SQUARED_AND_CONSTRAINTS);
  params.soft_constraint_weight = weight;
  params.maximum_cost = maximum_cost;
  params.n_constraints = n_con;
  for (int q = 0; q < n_con; ++q) { params.derivative[q] = constraints[q].first; params.value[q] = constraints[q].second; }
  std::vector<double> host_cost(n_rows), host_max((size_t)n_rows * n_con);
  EXPECT(mtg_magnitude_soft_cost_host(N, K, D, n_rows, coeffs.data(), times.data(), K, 1, &params, host_cost.data(), host_max.data(),
                                      nullptr) == MTG_OK);
  // the soft cost a set of maxima gives, and how far a relative error `delta` of each maximum can move it (the exponent rule:
  // d ln(term) = weight * (max / value) * delta; capped terms do not move)
  auto cost_of = [&](const double* mx, double delta, double* slack) {
    double sum = 0.0;
    *slack = 0.0;
    for (int q = 0; q < n_con; ++q) {
      const double value = constraints[q].second;
      const double term = std::exp((mx[q] - value) / value * weight);
      if (term < maximum_cost) *slack += term * std::expm1(weight * (mx[q] / value) * delta);
      sum += std::fmin(maximum_cost, term);
    }
    *slack += 1e-14 * sum;
    return sum;
  };
  bool saw_capped = false, saw_uncapped = false;
  for (int b = 0; b < n_rows; ++b) {
    for (int q = 0; q < n_con; ++q) {
      const double ref = ref_max[(size_t)b * n_con + q];
      EXPECT(std::fabs(host_max[(size_t)b * n_con + q] - ref) <= 1e-9 * ref);
    }
    double slack;
    const double want = cost_of(&ref_max[(size_t)b * n_con], 1e-9, &slack);
    EXPECT(std::fabs(want - ref_cost[b]) <= 1e-12 * ref_cost[b]);   // the rows' own cost is this formula on the rows' maxima
    EXPECT(std::fabs(host_cost[b] - ref_cost[b]) <= slack);
    saw_capped = saw_capped || ref_cost[b] >= maximum_cost;
    saw_uncapped = saw_uncapped || ref_cost[b] < maximum_cost;
  }
  EXPECT(saw_capped && saw_uncapped);
  params.derivative[0] = N / 2;   // beyond N / 2 - 1
  EXPECT(mtg_magnitude_soft_cost_host(N, K, D, n_rows, coeffs.data(), times.data(), K, 1, &params, host_cost.data(), nullptr, nullptr) ==
         MTG_ERR_INVALID_ARGUMENT);

  if (device) {
    TrajectoryBatch batch(all);
    std::vector<double> cost, maxima;
    EXPECT(batch.softConstraintCost(constraints, weight, &cost, &maxima, maximum_cost));
    EXPECT(cost.size() == (size_t)n_rows && maxima.size() == (size_t)n_rows * n_con);
    for (int b = 0; b < n_rows && cost.size() == (size_t)n_rows; ++b) {
      for (int q = 0; q < n_con; ++q) {
        const size_t i = (size_t)b * n_con + q;
        EXPECT(std::fabs(maxima[i] - host_max[i]) <= 1e-12 * host_max[i]);   // same lane code on both sides
        EXPECT(std::fabs(maxima[i] - ref_max[i]) <= 1e-9 * ref_max[i]);
      }
      double slack;
      cost_of(&ref_max[(size_t)b * n_con], 1e-9, &slack);
      EXPECT(std::fabs(cost[b] - ref_cost[b]) <= slack);
    }
    std::vector<double> none;
    EXPECT(batch.softConstraintCost({}, weight, &none) && none.size() == (size_t)n_rows && none[0] == 0.0);
    EXPECT(!batch.softConstraintCost({{N / 2, 1.0}}, weight, &none));
    EXPECT(!batch.softConstraintCost({{1, 0.0}}, weight, &none));
    EXPECT(!batch.softConstraintCost(std::vector<std::pair<int, double>>(5, {1, 1.0}), weight, &none));
  }
  if (failures == 0) std::printf("OBJECTIVE VENEER TESTS PASSED (%s)\n", device ? "host + device" : "host");
  return failures == 0 ? 0 : 1;
}
