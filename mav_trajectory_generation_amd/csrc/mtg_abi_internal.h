// mtg_abi_internal.h -- what the translation units behind the C ABI of include/mtg_hip.h share (host only, no kernels):
//   mtg_abi.hip (context, device memory, layouts), mtg_plan.hip (rank decision, plans), mtg_dispatch.hip (launcher of mtg_launch_plan.h's decision,
//   sequence / Mellinger / update / objective entries), mtg_shadow.hip (basic solution, refinement), mtg_multi.hip (mixed requests).
#ifndef MTG_ABI_INTERNAL_H_
#define MTG_ABI_INTERNAL_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mtg_hip.h"
#include "mtg_kernels.h"
#include "mtg_dimlane_rt.h"
#include "mtg_launch_plan.h"

int mtg_host_run(const MtgParams& P, int H, bool update);   // mtg_host.cpp: host build of the lane code
// mtg_coop.hip: the row-cooperative kernel (0 launched, 1 shape / size not covered, 2 runtime error) and its LDS need
int mtg_coop_launch(void* stream, int H, int D, int K, int deriv, long long B, const double* times, long long ts_b, long long ts_k,
                    const double* dfix, long long fs_b, long long fs_d, long long fs_c, double* coeffs, int* status, int* tstatus);
size_t mtg_coop_lds_bytes(int H, int D, int K);
extern "C" int mtg_basic_solution_one(int H, int K, int D, int deriv, const int* mask, const int* offF, const int* offP,
                                      const double* times, const double* dfix, double* dfree);   // mtg_basic.cpp (internal; exported for the CPU tests)

struct mtg_context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int* d_status = nullptr;
  int* h_status = nullptr;  // pinned
  // small host-pointer calls (the single-trajectory drop-in path): one page-locked bounce buffer, so that a call is one
  // H2D DMA, the kernel, one D2H DMA and one synchronisation instead of five staged pageable copies
  double* h_bounce = nullptr;
  size_t h_bounce_bytes = 0;
  int n_cu = 256;
  MtgKnobs knobs;                    // the form-related measurement knobs (mtg_launch_plan.h), set through mtg_context_set_option
  // the other knobs (same rules: include/mtg_hip_lab.h, never read from the environment by the library)
  bool knob_dl_any_rr = false;       // MTG_DL_ANY_SCHED=rr: round 2's unit schedule of the cross-structure launch
  bool knob_sample_generic = false;  // MTG_SAMPLE_GENERIC: mtg_sample_range never through its LDS-staged kernel
  int knob_sample_max_blocks = 0;    // MTG_SAMPLE_MAX_BLOCKS: >= 1 caps the persistent grid of mtg_sample_range (0: occupancy x CUs, the shipped grid)
  int knob_extrema_split = -1;       // MTG_EXTREMA_SPLIT: lanes per root search of the extrema kernels (include/mtg_hip_lab.h; -1: default)
  int knob_field_lanes = 0;          // MTG_FIELD_LANES: lanes that share one segment of the distance-field check (1 / 4 / 16 / 64; 0: default)
  // MTG_FLAG_CONCURRENT_ITEMS requests: side streams (created on first use) + fork / join events
  std::vector<hipStream_t> side_streams;
  hipEvent_t fork_event = nullptr;
  std::vector<hipEvent_t> join_events;
  // Cross-structure requests (mtg_multi_create -> mtg_solve_dl_any_kernel) are typically rebuilt with the SAME structure and new
  // buffers (a planner's mixed request per cycle; bench.py --config 4 rebuilds its 240-item request per timed region): the
  // per-workgroup unit lists depend only on the (chain length, order, tile count) sequence of the items, so they are computed and
  // uploaded once per structure and shared read-only by every request of that structure; the workspace is one buffer per
  // context (requests of one context run in stream order), the small per-request item tables come from a free list.
  struct DlAnySchedule {
    std::vector<long long> key;        // mtg_dl_any_schedule_key: grid, schedule kind, then (K, H, tiles) per item in launch order
    int grid = 0, nunits = 0;
    void* d_units = nullptr;           // MtgDlAnyUnit [nunits]
    int* d_wg_begin = nullptr;         // [grid + 1]
  };
  std::vector<DlAnySchedule> dl_any_schedules;      // never evicted while the context lives (bounded: kMaxDlAnySchedules)
  double* dl_any_ws = nullptr;
  size_t dl_any_ws_bytes = 0;
  std::vector<std::pair<void*, size_t>> dl_any_item_pool;   // free item tables (device)
  std::string last_error;
  std::mutex mu;
};

// one enqueued launch of the last solve: what mtg_launch_plan decided, the kernel parameters it ran with (params.ws: its workspace)
struct LaunchRecord {
  MtgLaunch launch;
  MtgParams params;
};

struct mtg_plan {
  mtg_context* ctx = nullptr;
  int N = 0, H = 0, D = 0, K = 0, deriv = 0;
  std::vector<int> mask;            // [K+1]
  std::vector<int> offF, offP;      // [K+2]
  int n_fixed = 0, n_free = 0;
  int null_dim = 0;                 // STRUCTURAL rank deficiency of the free system R_PP (mtg_plan.hip: structural_null_dim)
  int* d_tables = nullptr;          // vmask | offF | offP
  MtgPlanForms forms;               // the table entries of the shape, resolved once (mtg_launch_plan.h)
  bool lds_attr_set[4] = {false, false, false, false};   // [MtgLdsAttr]: LDS attribute of the slab-output kernels set
  double* ws = nullptr;
  size_t ws_bytes = 0;
  double* pert_cost = nullptr;      // [(K + 1)][batch] costs of mtg_mellinger_cost_gradient's virtual problems
  size_t pert_cost_bytes = 0;
  double* objective_ws = nullptr;   // mtg_time_objective: cost [batch] | maxima slots [batch][4] | per-trajectory status int32 [batch]
  size_t objective_ws_bytes = 0;
  double* user_ws = nullptr;       // caller-owned workspace (mtg_plan_set_workspace)
  size_t user_ws_bytes = 0;
  // staging for MTG_FLAG_HOST_POINTERS
  double* stage = nullptr;
  size_t stage_bytes = 0;
  // MTG_FLAG_BASIC_SOLUTION with device pointers: [status word (8 bytes) | per-trajectory status int32 [batch]] of the call itself
  double* basic_status = nullptr;
  size_t basic_status_bytes = 0;
  // Structurally rank-deficient plans: the SHADOW plan = this pattern with null_dim additional slots fixed (to zero), chosen so
  // that the fixed functionals span the cost's null space -- a regular system whose solution is a basic solution of this one
  // (MTG_FLAG_BASIC_SOLUTION).  shadow_fixed_src[j]: column of this plan's d_fixed behind the shadow's fixed column j (-1: a
  // pinned slot, value 0); free_in_shadow[j]: the shadow's free column of this plan's free column j (-1: pinned, value 0).
  mtg_plan* shadow = nullptr;
  std::vector<int> shadow_fixed_src, free_in_shadow;
  int* d_shadow_maps = nullptr;      // device copy: shadow_fixed_src | free_in_shadow
  double* shadow_buf = nullptr;      // [batch][D][n_fixed of the shadow] | [batch][D][n_free of the shadow]
  size_t shadow_buf_bytes = 0;
  double* refine_buf = nullptr;      // MTG_FLAG_REFINE: x | residual | delta ([batch][D][n_free] each) | zeros ([batch][D][n_fixed])
  size_t refine_buf_bytes = 0;
  std::vector<LaunchRecord> last;
};

inline int set_err(mtg_context* ctx, int code, const std::string& msg) {
  if (ctx) ctx->last_error = msg;
  return code;
}
#define MTG_HIP_TRY(ctx, expr)                                                                 \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return set_err(ctx, MTG_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

inline int ensure_buffer(mtg_context* ctx, double** buf, size_t* cur, size_t need) {
  if (*cur >= need) return MTG_OK;
  if (*buf) MTG_HIP_TRY(ctx, hipFree(*buf));
  *buf = nullptr;
  *cur = 0;
  MTG_HIP_TRY(ctx, hipMalloc((void**)buf, need));
  *cur = need;
  return MTG_OK;
}

inline void fill_common(const mtg_plan* p, MtgParams& P, int64_t batch, const mtg_layout* L) {
  std::memset(&P, 0, sizeof(P));
  P.ts_b = L->times_stride_b; P.ts_k = L->times_stride_k;
  P.fs_b = L->fixed_stride_b; P.fs_d = L->fixed_stride_d; P.fs_c = L->fixed_stride_c;
  P.ps_b = L->free_stride_b; P.ps_d = L->free_stride_d; P.ps_c = L->free_stride_c;
  P.status = p->ctx->d_status;
  P.vmask = p->d_tables;
  P.offF = p->d_tables + (p->K + 1);
  P.offP = p->d_tables + (p->K + 1) + (p->K + 2);
  P.B = batch;
  P.K = p->K;
  P.Dtot = p->D;
  P.deriv = p->deriv;
  // host copies of the table offsets (same values as the __constant__ ones)
  const int ainv_off[7] = {0, 0, 2, 10, 28, 60, 110};
  P.ainvoff = ainv_off[p->H];
  int off = 0;
  for (int n = 2; n < p->N; n += 2) off += (n / 2) * n * n;
  P.h1off = off + p->deriv * p->N * p->N;
}

struct PerturbedTimes { double h, lower_bound; };   // mtg_mellinger_cost_gradient: (K + 1) virtual problems per trajectory

// contiguous [B][D][n] strides of a layout's fixed / free values
inline void mtg_fixed_contiguous(mtg_layout* L, int D, int n) { L->fixed_stride_b = (int64_t)D * n; L->fixed_stride_d = n; L->fixed_stride_c = 1; }
inline void mtg_free_contiguous(mtg_layout* L, int D, int n) { L->free_stride_b = (int64_t)D * n; L->free_stride_d = n; L->free_stride_c = 1; }

// ---- functions that cross the translation units -------------------------------------------------------------------------------
int mtg_status_code(mtg_context* ctx, int status_word);                                   // mtg_abi.hip: flags -> error code + text
// mtg_dispatch.hip: one solve / update call.  own_status_dev: a device status word of the CALL (zeroed here) instead of the
// context's -- flags of earlier asynchronous launches stay where the next mtg_context_sync finds them; explicit_rhs
// (MTG_FLAG_REFINE's correction solve; with MTG_FLAG_GENERIC_KERNEL): [batch][D][n_free], added to the right-hand side
int mtg_solve_impl(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed, double* coeffs, double* d_free,
                   double* cost, uint32_t flags, bool update_only, int32_t* traj_status = nullptr, const PerturbedTimes* pert = nullptr,
                   hipStream_t on_stream = nullptr, int* own_status_dev = nullptr, const double* explicit_rhs = nullptr);
// mtg_shadow.hip (see there)
void mtg_flag_structurally_singular(const mtg_plan* p, hipStream_t st, int* status, int* tstatus, int64_t batch);
bool mtg_shadow_layout(const mtg_plan* p, int64_t batch, const mtg_layout* L, mtg_layout* SL);
size_t mtg_shadow_fixed_elems(const mtg_plan* p, int64_t batch);
void mtg_shadow_gather_async(const mtg_plan* p, int64_t batch, const mtg_layout* L, const double* d_fixed, double* dst, mtg_layout* SL, hipStream_t st);
void mtg_launch_pin_scatter(const mtg_plan* p, int64_t batch, const mtg_layout* L, const double* sfr, double* d_free, hipStream_t st);

#endif  // MTG_ABI_INTERNAL_H_
