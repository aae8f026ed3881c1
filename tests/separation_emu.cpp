// separation_emu.cpp -- the lane code of the trajectory-to-trajectory separation check (csrc/mtg_separation_lane.h) for the host
// with its two test knobs exposed: pruning on or off, and the number of root searches a lane ran.  One call is one lane:
// (one trajectory of A, one of B, segment i of A).  Built by tests/test_trajectory_separation.py; with -DSEPARATION_EMU_MAIN a
// stand-alone program that runs every lane of a small seeded pair both ways and compares the results (the sanitizer build).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../mav_trajectory_generation_amd/csrc/mtg_separation_lane.h"

// out_f: separation, time; out_i: segment_b, failing_a, failing_b, pieces, invalid, searches
extern "C" int separation_emu_lane(int n_coeffs, int dimension, int ka, const double* coeffs_a, const double* times_a, double start_a,
                                   int kb, const double* coeffs_b, const double* times_b, double start_b, int i, double min_separation,
                                   int prune, double* out_f, int32_t* out_i) {
  if (n_coeffs < 1 || n_coeffs > 12 || i < 0 || i >= ka) return 1;
  const mtgp::Side A{coeffs_a, times_a, 1, ka, start_a}, B{coeffs_b, times_b, 1, kb, start_b};
  mtgs::with_instance<mtgp::kMinInstance>(n_coeffs, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    double buf[mtgp::buffer_len(NC)];
    double* r = buf;
    mtgp::Fold f;
    int searches = 0;
    mtgp::lane_check<NC, double*>(A, B, i, n_coeffs, dimension, min_separation, prune != 0, r, f, &searches);
    out_f[0] = f.separation;
    out_f[1] = f.time;
    out_i[0] = f.segment_b;
    out_i[1] = f.failing_a;
    out_i[2] = f.failing_b;
    out_i[3] = f.pieces;
    out_i[4] = f.invalid ? 1 : 0;
    out_i[5] = searches;
  });
  return 0;
}

#if defined(SEPARATION_EMU_MAIN)
#include <vector>

#include "../include/mtg_hip.h"

// A deterministic pair of small batches through the host entry point and through the lane, pruned and not.
int main() {
  const int N = 10, D = 3, KA = 5, KB = 4, BA = 3, BB = 2;
  std::vector<double> ca(BA * KA * D * N), cb(BB * KB * D * N), ta(BA * KA), tb(BB * KB), sa(BA), sb(BB);
  uint64_t state = 20261100;
  auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; };
  auto fill = [&](std::vector<double>& c, int n) {
    for (size_t k = 0; k < c.size(); ++k) {
      double f = 1.0;
      for (int e = 2; e <= (int)(k % n); ++e) f *= e;
      c[k] = 6.0 * (next() - 0.5) / f;
    }
  };
  fill(ca, N);
  fill(cb, N);
  for (auto& t : ta) t = 0.5 + 2.5 * next();
  for (auto& t : tb) t = 0.5 + 2.5 * next();
  for (auto& s : sa) s = 1.5 * next();
  for (auto& s : sb) s = 1.5 * next();
  std::vector<int32_t> pairs;
  for (int a = 0; a < BA; ++a)
    for (int b = 0; b < BB; ++b) { pairs.push_back(a); pairs.push_back(b); }
  const int P = BA * BB;
  std::vector<int32_t> feas(P), fa(P), fb(P), pa(P), pb(P), segb(P * KA), pieces(P * KA);
  std::vector<double> sep(P), time(P), seg(P * KA), segt(P * KA);
  const int rc = mtg_check_trajectory_separation_host(N, D, KA, BA, ca.data(), ta.data(), KA, 1, sa.data(), KB, BB, cb.data(), tb.data(), KB, 1,
                                                      sb.data(), P, pairs.data(), 1.5, feas.data(), fa.data(), fb.data(), sep.data(),
                                                      time.data(), pa.data(), pb.data(), seg.data(), segt.data(), segb.data(), pieces.data());
  if (rc != 0) { std::printf("host form returned %d\n", rc); return 1; }
  int bad = 0, n_pieces = 0;
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < KA; ++i) {
      double f0[2], f1[2];
      int32_t i0[6], i1[6];
      const int a = pairs[2 * p], b = pairs[2 * p + 1];
      for (int prune = 0; prune < 2; ++prune)
        separation_emu_lane(N, D, KA, ca.data() + a * KA * D * N, ta.data() + a * KA, sa[a], KB, cb.data() + b * KB * D * N, tb.data() + b * KB,
                            sb[b], i, 1.5, prune, prune ? f1 : f0, prune ? i1 : i0);
      bad += std::memcmp(f0, f1, sizeof f0) != 0 || std::memcmp(i0, i1, 5 * sizeof(int32_t)) != 0;
      bad += std::memcmp(&f1[0], &seg[p * KA + i], sizeof(double)) != 0 || i1[0] != segb[p * KA + i] || i1[3] != pieces[p * KA + i];
      n_pieces += i1[3];
    }
  std::printf("separation_emu: %d pairs, %d pieces, %d mismatches\n", P, n_pieces, bad);
  return bad != 0;
}
#endif
