// TrajectoryBatch::computeAxisMinMax and boundingBoxes of the compat veneer (include/compat/mav_trajectory_generation/
// trajectory_batch.h) on the device entry mtg_minmax_axes, against the veneer's own single-object Polynomial::computeMinMax
// folded over the segments the way the batch entry folds them (first strictly smaller / larger).
//   test_axis_minmax_veneer      -- needs a device
#include <mav_trajectory_generation/trajectory_batch.h>

#include <cmath>
#include <cstdio>
#include <vector>

using namespace mav_trajectory_generation;

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static unsigned long long state = 88172645463325252ull;
static double uniform() {   // xorshift64, in (-1, 1)
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (double)(state >> 11) / 4503599627370496.0 - 1.0;
}

// S = sum_{k >= q} ff(k, q) |p_k| T^(k - q): the bound of a value comparison is 1e-9 max(1, S)
static double bound(const Polynomial& p, double T, int q) {
  const Eigen::VectorXd c = p.getCoefficients(q);
  double s = 0.0, tp = 1.0;
  for (int i = 0; i < (int)c.size(); ++i) {
    s += std::fabs(c[i]) * tp;
    tp *= T;
  }
  return 1e-9 * std::fmax(1.0, s);
}

static void run(int N, int K, int D, int B) {
  std::vector<Trajectory> trajectories(B);
  for (int b = 0; b < B; ++b) {
    Segment::Vector segments(K, Segment(N, D));
    for (int k = 0; k < K; ++k) {
      segments[k].setTime(1.25 + 0.75 * uniform());
      for (int d = 0; d < D; ++d) {
        Eigen::VectorXd c(N);
        double fact = 1.0;
        for (int n = 0; n < N; ++n) {
          c[n] = 1.5 * uniform() / fact;
          fact *= n + 1;
        }
        segments[k][d] = Polynomial(N, c);
      }
    }
    trajectories[b].setSegments(segments);
  }
  TrajectoryBatch batch(trajectories);
  EXPECT((int)batch.size() == B && batch.D() == D);
  std::vector<Extremum> mn, mx;
  for (int q = 0; q <= 4 && q <= N - 1; ++q) {
    EXPECT(batch.computeAxisMinMax(q, &mn, &mx));
    EXPECT(mn.size() == (size_t)B * D && mx.size() == (size_t)B * D);
    for (int b = 0; b < B; ++b)
      for (int d = 0; d < D; ++d) {
        const Extremum& lo = mn[(size_t)b * D + d];
        const Extremum& hi = mx[(size_t)b * D + d];
        double want_lo = 0.0, want_hi = 0.0, worst_bound = 0.0;
        for (int k = 0; k < K; ++k) {
          const Segment& s = trajectories[b].segments()[k];
          std::pair<double, double> a, c;
          EXPECT(s[d].computeMinMax(0.0, s.getTime(), q, &a, &c));
          if (k == 0 || a.second < want_lo) want_lo = a.second;
          if (k == 0 || c.second > want_hi) want_hi = c.second;
          worst_bound = std::fmax(worst_bound, bound(s[d], s.getTime(), q));
        }
        EXPECT(std::fabs(lo.value - want_lo) <= worst_bound);
        EXPECT(std::fabs(hi.value - want_hi) <= worst_bound);
        // the reported (segment, time) carries the reported value
        for (const Extremum* e : {&lo, &hi}) {
          EXPECT(e->segment_idx >= 0 && e->segment_idx < K);
          if (e->segment_idx < 0 || e->segment_idx >= K) continue;
          const Segment& s = trajectories[b].segments()[e->segment_idx];
          EXPECT(e->time >= 0.0 && e->time <= s.getTime());
          EXPECT(std::fabs(s[d].evaluate(e->time, q) - e->value) <= bound(s[d], s.getTime(), q));
        }
      }
    if (q == 0) {
      std::vector<double> box_lo, box_hi;
      EXPECT(batch.boundingBoxes(&box_lo, &box_hi));
      EXPECT(box_lo.size() == mn.size() && box_hi.size() == mx.size());
      for (size_t r = 0; r < mn.size() && r < box_lo.size(); ++r) {
        EXPECT(box_lo[r] == mn[r].value && box_hi[r] == mx[r].value && box_lo[r] <= box_hi[r]);
      }
    }
  }
  EXPECT(!batch.computeAxisMinMax(5, &mn, &mx));
  EXPECT(!batch.computeAxisMinMax(-1, &mn, &mx));
  if (N <= 4) EXPECT(!batch.computeAxisMinMax(N, &mn, &mx));
}

int main() {
  run(10, 8, 3, 9);    // 216 lanes
  run(12, 1, 6, 5);    // the reference's 6-DoF shape
  run(3, 2, 1, 1);     // parabolas: orders 0 .. 2
  run(7, 3, 4, 4);
  if (failures == 0) std::printf("AXIS MINMAX VENEER TESTS PASSED (device)\n");
  return failures == 0 ? 0 : 1;
}
