// mtg_entries.h -- what the kernel tables hand to the host: the launch constants, the kernel function-pointer types and the table
// entry structs of every launch form.  Plain C++ without a HIP header, so that the launch decision (mtg_launch_plan.h) and its CPU
// test build with g++; the kernel units get it through mtg_kernels.h.
#ifndef MTG_ENTRIES_H_
#define MTG_ENTRIES_H_
#include <stddef.h>

struct MtgParams;    // mtg_lane.h
struct MtgTileRef;   // mtg_kernels.h

constexpr int kWave = 64;
constexpr int kBlock = 2 * kWave;  // wave 0: direction A (forward), wave 1: direction B

// A queue of batches in ONE launch (mtg_solve_linear_sequence; mtg_solve_slab_queue_kernel in mtg_kernels.h): the pointer triples
// travel in the kernel arguments (no upload in front of the launch).
struct MtgSeqItem { const double* times; const double* dfix; double* coeffs; };
constexpr int kSeqMax = 96;    // batches per launch (kernel arguments <= 4 KB); longer queues are cut into several launches
struct MtgSeqQueue {
  int n, tiles_per_batch;
  MtgSeqItem item[kSeqMax];
};

using SolveFn = void (*)(MtgParams, int);
using UpdateFn = void (*)(MtgParams, int);
using SolveMultiFn = void (*)(const MtgParams*, const MtgTileRef*, int);
struct MtgStaticEntry {
  int h, d, k, ms, mi, me, dv;
  int heavy;       // static variant that spills: prefer a rolled variant for large launches
  SolveFn fn[5];   // [extra outputs (cost / d_free)] + 2 * [write-through stores]; [4] = cost only (OUT 9)
  void (*upd[2])(MtgParams, int);   // rolled entries: setFreeConstraints kernel [with cost]; static entries: null
  void (*upd_slab[2][2])(MtgParams, int);   // rolled entries with all plan dimensions: the same with whole-sector output, [with cost][piece not a multiple of 64 bytes]
  size_t upd_slab_lds;
  SolveMultiFn multi[4];            // rolled entries: several plans in one launch, [extra outputs] + 2 * [write-through]
};
using SolveQueueFn = void (*)(MtgParams, int, MtgSeqQueue);
struct MtgSlabEntry {
  int h, d, k, ms, mi, me, dv;
  size_t lds;
  SolveFn fn[2];   // coefficient store policy: [0] write-back, [1] nt sc1
  SolveQueueFn queue;   // the same (nt sc1) over a queue of batches: mtg_solve_linear_sequence
  SolveFn extra;        // nt sc1 with the extra outputs (OUT = 3: cost and / or d_P), round 3
};

// dimension-in-lane launch form (mtg_dimlane.h / mtg_dimlane.hip): canonical SoA inputs, coefficient output (+ status)
struct MtgDimlaneEntry {
  int h, k, ms, mi, me, dv, dl, np;
  int tpw;            // trajectories per wave (64 / dl)
  int lo_per_cu, hi_per_cu;   // default form while lo * CUs <= workgroups <= hi * CUs / 2 (hi = 0: no upper limit; hi counts HALF workgroups per CU)
  size_t lds;         // dynamic LDS per workgroup
  size_t ws_per_lane; // long-chain variants (MtgCfg::WSJ > 0): workspace bytes per resident lane (grid * np * 128 lanes), else 0
  // enqueues one launch on `stream` (a hipStream_t): grid workgroups of np * 128 threads (coefficient stores: nt sc1); aos: input
  // layout (0 canonical SoA, 1 canonical AoS, 2 padded SoA); returns 0 or -1 (attribute / launch set-up failed)
  int (*launch)(void* stream, int grid, const double* times, const double* dfix, double* coeffs, int* status,
                int* traj_status, int B, int ntiles, double* ws, int aos);
  // a queue of batches in one launch (mtg_solve_linear_sequence; main-table variants only, else null): ntiles = tiles of
  // all batches (q->n * q->tiles_per_batch)
  int (*launch_queue)(void* stream, int grid, const MtgSeqQueue* q, int* status, int B, int ntiles, double* ws, int aos);
  // solves that also return the cost and / or d_P (either pointer may be null; cost zeroed by the caller; ps_*: d_P strides
  // in doubles); main-table variants only, else null
  int (*launch_extra)(void* stream, int grid, const double* times, const double* dfix, double* coeffs, int* status,
                      int* traj_status, int B, int ntiles, double* ws, int aos, double* dfree, double* cost, long long ps_b,
                      long long ps_d, long long ps_c);
};

// table entry of the run-time-K bodies (one per polynomial order / dimension count): mtg_dimlane_rt.hip
struct MtgDimlaneRtEntry {
  int h, ms, mi, me, dv, dl;
  int tpw, r_steps, l_steps;
  size_t lds;
  size_t step_bytes_per_lane;   // workspace bytes per head step and resident lane
  int (*launch)(void* stream, int grid, const double* times, const double* dfix, double* coeffs, int* status, int* traj_status,
                int B, int K, int ntiles, double* ws, int aos);
};

#endif  // MTG_ENTRIES_H_
