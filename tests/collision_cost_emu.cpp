// collision_cost_emu.cpp -- a stand-alone program (its own main) around the host form of the distance-field collision cost
// (csrc/mtg_collision_host.cpp, built together with it): seeded batches of every coefficient count through
// mtg_collision_cost_host with guard words around every output, in every combination of the optional outputs, and a serial
// restatement of the rule from the lane header (64 partial sums, the butterfly) that must agree bit for bit.  Built by
// tests/test_collision_cost_arguments.py with AddressSanitizer and UndefinedBehaviorSanitizer and run as a subprocess.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mtg_hip.h"
#include "../mav_trajectory_generation_amd/csrc/mtg_collision_lane.h"

namespace {

constexpr int kGuard = 4;
constexpr double kGuardWord = -7777.25;
constexpr int32_t kGuardInt = -7777;

uint64_t state = 20261021;
double next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; }

template <class T>
struct Guarded {
  std::vector<T> v;
  T word;
  Guarded(size_t n, T w) : v(n + 2 * kGuard, w), word(w) {}
  T* data() { return v.data() + kGuard; }
  bool intact() const {
    for (int i = 0; i < kGuard; ++i)
      if (std::memcmp(&v[i], &word, sizeof(T)) != 0 || std::memcmp(&v[v.size() - 1 - i], &word, sizeof(T)) != 0) return false;
    return true;
  }
};

// one segment by the rule, NC = 12 whatever N is (zero padding changes nothing: checked against the entry's own instance)
void restate(const double* c, int N, int D, double T, const mtgf::Grid& g, const mtgc::Potential& q, double dt, int max_samples,
             double* cost, double* grad, int* samples) {
  double p[3][12];
  mtgs::load_padded<12, 3>(c, N, D, p);
  const int S = mtgf::sample_count(T, dt, max_samples);
  static mtgc::Sums<12, true> P[64];
  for (int l = 0; l < 64; ++l) {
    mtgc::clear(P[l]);
    mtgc::sum_samples<12, true>(p, T, dt, S, l, 64, g, q, P[l]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    mtgc::Sums<12, true> Q[64];
    for (int l = 0; l < 64; ++l) Q[l] = P[l ^ off];
    for (int l = 0; l < 64; ++l) mtgc::add(P[l], Q[l]);
  }
  *samples = S;
  *cost = S < 0 ? NAN : P[0].cost;
  for (int a = 0; a < D; ++a)
    for (int j = 0; j < N; ++j) grad[a * N + j] = a >= 3 ? 0.0 : (S < 0 ? NAN : P[0].grad[a][j]);
}

bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main() {
  const int NX = 9, NY = 8, NZ = 7;
  std::vector<float> voxels(NX * NY * NZ);
  for (auto& v : voxels) v = (float)(1.5 * next() - 0.25);
  mtg_distance_field field;
  mtg_distance_field_init(&field);
  field.distances = voxels.data(); field.nx = NX; field.ny = NY; field.nz = NZ;
  field.origin[0] = -1.0; field.origin[1] = -0.75; field.origin[2] = -0.5;
  field.voxel_size = 0.25; field.outside_distance = 0.125;
  const double dt = 0.03, inflation = 0.1, epsilon = 0.5, speed_epsilon = 1e-3;
  const int max_samples = 150;
  int bad = 0, calls = 0, segments = 0;
  for (int N = 1; N <= 12; ++N)
    for (int D = 3; D <= 4; ++D) {
      const int B = 3, K = 4;
      std::vector<double> coeffs((size_t)B * K * D * N), times(B * K);
      for (size_t i = 0; i < coeffs.size(); ++i) {
        const int j = (int)(i % N);
        double f = 1.0;
        for (int e = 2; e <= j; ++e) f *= e;
        coeffs[i] = (j == 0 ? 0.9 * next() - 0.2 : 1.2 * (next() - 0.5)) / f;   // around the grid: inside and outside samples
      }
      for (auto& t : times) t = 0.05 + 2.5 * next();
      times[1] = 0.0; times[2] = -1.0; times[5] = NAN; times[7] = 10.0;   // T = 0, T < 0, NaN, more than max_samples
      mtgf::Grid g;
      mtgc::Potential q;
      if (!mtgc::arguments_ok(N, K, D, B, K, 1, &field, dt, max_samples, inflation, epsilon, speed_epsilon, &g, &q)) { ++bad; continue; }
      std::vector<double> want_cost(B * K), want_grad((size_t)B * K * D * N);
      std::vector<int> want_samples(B * K);
      for (int s = 0; s < B * K; ++s)
        restate(coeffs.data() + (size_t)s * D * N, N, D, times[s], g, q, dt, max_samples, &want_cost[s], &want_grad[(size_t)s * D * N], &want_samples[s]);
      segments += B * K;
      for (int mask = 0; mask < 8; ++mask) {
        Guarded<double> seg(B * K, kGuardWord), traj(B, kGuardWord), grad((size_t)B * K * D * N, kGuardWord);
        Guarded<int32_t> samples(B * K, kGuardInt);
        const int rc = mtg_collision_cost_host(N, K, D, B, coeffs.data(), times.data(), K, 1, &field, dt, max_samples, inflation, epsilon,
                                               speed_epsilon, seg.data(), mask & 1 ? traj.data() : nullptr, mask & 2 ? grad.data() : nullptr,
                                               mask & 4 ? samples.data() : nullptr);
        ++calls;
        if (rc != 0 || !seg.intact() || !traj.intact() || !grad.intact() || !samples.intact()) { ++bad; continue; }
        for (int s = 0; s < B * K; ++s) {
          bad += !same(seg.data()[s], want_cost[s]);
          if (mask & 4) bad += samples.data()[s] != want_samples[s];
          if (mask & 2)
            for (int e = 0; e < D * N; ++e) bad += !same(grad.data()[(size_t)s * D * N + e], want_grad[(size_t)s * D * N + e]);
        }
        if (mask & 1)
          for (int b = 0; b < B; ++b) {
            double total = 0.0;
            for (int k = 0; k < K; ++k) total = total + seg.data()[b * K + k];
            bad += !same(traj.data()[b], total);
          }
        if (!(mask & 1)) bad += traj.data()[0] != kGuardWord;
        if (!(mask & 2)) bad += grad.data()[0] != kGuardWord;
        if (!(mask & 4)) bad += samples.data()[0] != kGuardInt;
      }
    }
  std::printf("collision_cost_emu: %d calls, %d segments, %d mismatches\n", calls, segments, bad);
  return bad != 0;
}
