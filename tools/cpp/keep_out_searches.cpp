// The keep-out zone check's optional counter for tools/bench_keep_out_zones.py: how many zones each lane SEARCHES (of n_zones
// without pruning), from the lane code itself (csrc/mtg_keepout_lane.h compiled for the host; N = 10 and 12 only).
//   g++ -O2 -std=c++17 -shared -fPIC -o libkeep_out_searches.so keep_out_searches.cpp
#include <cstdint>

#include "../../mav_trajectory_generation_amd/csrc/mtg_keepout_lane.h"

extern "C" int keep_out_searches(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                 const double* times, const double* zones, int32_t n_zones, int32_t n_planes, double inflation,
                                 int32_t* searches /* [batch][n_segments] */) {
  if (n_coeffs < 9 || n_coeffs > 12) return -1;
  for (int64_t idx = 0; idx < batch * n_segments; ++idx) {
    const double* c = coeffs + idx * (int64_t)(dimension * n_coeffs);
    mtgk::Fold f;
    int n = 0;
    if (n_coeffs <= 10) {
      double roots[mtgk::roots_len(10)];
      double* r = roots;
      mtgk::segment_check<10, double*>(c, n_coeffs, dimension, times[idx], zones, n_zones, n_planes, inflation, r, f, &n);
    } else {
      double roots[mtgk::roots_len(12)];
      double* r = roots;
      mtgk::segment_check<12, double*>(c, n_coeffs, dimension, times[idx], zones, n_zones, n_planes, inflation, r, f, &n);
    }
    searches[idx] = n;
  }
  return 0;
}
