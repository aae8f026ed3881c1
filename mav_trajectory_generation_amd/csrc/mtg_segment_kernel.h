// mtg_segment_kernel.h -- the device half of the frame the per-segment root-search kernels share (mtg_extrema.hip,
// mtg_feasibility.hip, mtg_objective.hip, mtg_halfplane.hip): one lane per (trajectory, segment) of a [B][K][D][N] batch, the
// lane's root buffers as LDS columns, the first-failure word of a trajectory, and the tail of an entry point.  HIP only; the
// host + device half is mtg_segment_lane.h.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mtg_hip.h"
#include "mtg_segment_lane.h"

extern "C" int mtg_context_stream_device(mtg_context* ctx, void** stream, int* device);
extern "C" int mtg_context_set_last_error(mtg_context* ctx, int code, const char* message);   // mtg_abi.hip

namespace mtgs {

// A lane's buffer in LDS, [slot][lane] layout: lanes in lock-step hit distinct banks.  COLS = columns per workgroup.
template <int COLS>
struct LdsColumn {
  double* p;   // element i at p[i * COLS]
  __device__ double& operator[](int i) { return p[i * COLS]; }
};

struct SegShape {
  const double* coeffs;   // [B][K][D][N]
  const double* times;    // times[b*ts_b + k*ts_k]
  long long ts_b, ts_k;
  long long B;
  int N, K, D;
};

struct SegLane {
  long long idx, b;   // (trajectory, segment) number b * K + seg, trajectory
  int seg;
  double T;           // segment time
  const double* c;    // the segment's [D][N] coefficients
  bool in_range;      // false: nothing else is set, the lane has no segment
};
__device__ __forceinline__ SegLane seg_lane(const SegShape& S, long long idx) {
  SegLane L;
  L.idx = idx;
  L.in_range = idx < S.B * S.K;
  if (!L.in_range) return L;
  L.b = idx / S.K;
  L.seg = (int)(idx - L.b * S.K);
  L.T = S.times[L.b * S.ts_b + (long long)L.seg * S.ts_k];
  L.c = S.coeffs + idx * (long long)(S.D * S.N);
  return L;
}

// lane per trajectory, ahead of the segment kernel: no failure yet; key (or null) is a second per-trajectory word to seed
template <class Key>
__global__ void first_failure_init_kernel(int* word, Key* key, Key key_seed, long long B) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  word[b] = kNoFailure;
  if (key) key[b] = key_seed;
}
// a failing lane: the atomic minimum keeps the first failure whichever lane finishes first
__device__ __forceinline__ void report_failure(int* word, int segment, int code) { atomicMin(word, failure_word(segment, code)); }

// A trajectory's minimum of a double through atomicMin on an unsigned word (the clearance checks): unsigned order = numeric
// order, and NaN below every number (-infinity maps to 0x000f.., so 0 is free)
__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  if (x != x) return 0ull;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
constexpr unsigned long long kKeyInfinity = 0xfff0000000000000ull;   // order_key(+infinity): "no clearance yet"
__device__ __forceinline__ double order_value(unsigned long long k) {
  if (k == 0ull) return NAN;
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

inline dim3 grid_for(long long lanes, int threads) { return dim3((unsigned)((lanes + threads - 1) / threads)); }

// the context's stream, with its device made current
inline int entry_stream(mtg_context* ctx, hipStream_t* stream) {
  void* s = nullptr;
  int device = 0;
  const int rc = mtg_context_stream_device(ctx, &s, &device);
  if (rc != MTG_OK) return rc;
  if (hipSetDevice(device) != hipSuccess) return MTG_ERR_DEVICE;
  *stream = (hipStream_t)s;
  return MTG_OK;
}

}  // namespace mtgs
