// mtg_launch_plan.h -- the launch decision: plan, batch, layout, flags and knobs -> kernel form, grid, LDS and workspace sizes, as
// pure functions.  No HIP header, plain C++, nothing allocated, no device touched: mtg_dispatch.hip launches, reports
// (mtg_plan_launch_form) and replays (mtg_time_last_solve) what mtg_launch_plan() returns, the queue takes mtg_queue_plan(),
// mtg_multi.hip the shared rules at the end; the CPU tests reach all of it (tests/launch_plan_emu.cpp, tests/test_launch_plan.py).
#ifndef MTG_LAUNCH_PLAN_H_
#define MTG_LAUNCH_PLAN_H_
#include <stdint.h>

#include <algorithm>

#include "../../include/mtg_hip.h"
#include "mtg_entries.h"

// The form-related measurement knobs of a context (mtg_context_set_option, include/mtg_hip_lab.h; never read from the environment by
// the library); defaults = the shipped behaviour.  In the comments: the environment variables the PYTHON layer forwards.
struct MtgKnobs {
  int force_dg = 0;             // MTG_FORCE_DG: dimension-group size of the specialised kernels
  bool prefer_rolled = false;   // MTG_PREFER_ROLLED: rolled variant even where a static one exists
  bool no_dimlane = false;      // MTG_NO_DIMLANE: never pick the dimension-in-lane form
  int dl_max_units_per_cu = -1; // MTG_DL_MAX_UNITS: overrides the variants' upper limit (workgroups <= this x CUs; 0: none)
  bool no_slab = false;         // MTG_NO_SLAB: fused form without the slab-output kernel
  bool no_slab_extra = false;   // MTG_NO_SLAB_EXTRA: extra outputs (cost / d_P) through the older fused kernel
  bool no_dl_extra = false;     // MTG_NO_DL_EXTRA: extra outputs never through the dimension-in-lane kernels
  bool no_queue = false;        // MTG_NO_QUEUE: mtg_solve_linear_sequence as one launch per batch
  int dl_grid_per_cu = 8;       // MTG_DL_GRID_PER_CU: workgroups per CU of a (non-workspace) dimension-in-lane launch
  int dl_rt = -1;               // MTG_DL_RT: 1 = the run-time-K body even where a static variant exists, 0 = never (default: where none exists)
  bool no_balance = false;      // MTG_NO_BALANCE: persistent grids are not evened out over their rounds
  int slab_policy = -1;         // MTG_SLAB_POLICY: 0 write-back, 1 nt sc1
  int rolled_wg_per_cu = 4;     // MTG_ROLLED_WG_PER_CU: persistent workgroups per CU of the rolled (workspace) kernels
  int coop = -1;                // MTG_COOP: 1 always / 0 never take the row-cooperative form where eligible (default: by size)
};

// Everything of the decision that depends on the plan alone, resolved once by mtg_plan_create: no table search per call.
struct MtgPlanForms {
  int H = 0, D = 0, K = 0, n_fixed = 0;
  int free_mid = 0;                            // free slots of the middle vertex (K + 1) / 2: the exchange buffers' size
  const MtgStaticEntry* fast = nullptr;        // all dimensions in one workgroup
  const MtgStaticEntry* fast_split = nullptr;  // smallest dimension group that divides D
  const MtgStaticEntry* rolled = nullptr;      // the rolled (run-time K) entry of all dimensions
  const MtgStaticEntry* group[5] = {};         // [dg]: entry of dimension-group size dg = 1 .. 4 (option "force_dg")
  const MtgSlabEntry* slab = nullptr;          // slab-output kernels of the shape (whole-sector stores)
  const MtgDimlaneEntry* dimlane = nullptr;    // dimension-in-lane form, one unrolled body per chain length
  const MtgDimlaneRtEntry* dimlane_rt = nullptr;   // run-time-K dimension-in-lane body: any chain length of the standard shapes
  bool coop_shape = false;                     // end vertices fully fixed, position-only interior vertices (row-cooperative form)
  size_t coop_lds = 0;                         // mtg_coop_lds_bytes(H, D, K)
  SolveFn generic_solve[5][3] = {};            // [dimensions 1 .. 4][0 plain, 1 extra outputs, 2 cost only]
  UpdateFn generic_update[5][2] = {};          // [dimensions 1 .. 4][with cost]
};

// What a call asks for.  extra: cost and / or d_P output next to the coefficients (an update call: the cost); cost_only:
// MTG_FLAG_COST_ONLY; pert: the (K + 1) x batch virtual problems of mtg_mellinger_cost_gradient (always cost only).
struct MtgCall { int64_t batch = 0; const mtg_layout* L = nullptr; uint32_t flags = 0; bool update = false, extra = false, cost_only = false, pert = false; };

// The form codes of mtg_plan_launch_form, plus the update-from-free path.
enum class MtgForm : int { kGeneric = 0, kFused = 1, kSplit = 2, kRolled = 3, kSlab = 4, kDimlane = 5, kDimlaneRt = 6, kCoop = 7, kUpdate = 8 };
// which "LDS attribute already set" flag of the plan covers a launch's kernel (hipFuncSetAttribute once per plan and kernel)
enum class MtgLdsAttr : int { kNone = -1, kSlabWriteBack = 0, kSlabNt = 1, kSlabExtra = 2, kSlabQueue = 3 };

// One launch.  Exactly one of fn / dl / rt / coop names what runs: a kernel launched here with (params, ntiles) over grid x gridy
// workgroups of `block` threads and `lds` bytes; a table entry's own launch function, which takes grid, ntiles, workspace and input
// kind and knows its block and LDS sizes itself; or mtg_coop_launch, which derives all of them from the batch.
struct MtgLaunch {
  SolveFn fn = nullptr;
  const MtgDimlaneEntry* dl = nullptr;
  const MtgDimlaneRtEntry* rt = nullptr;
  bool coop = false;
  int grid = 0, gridy = 1, block = kBlock;
  size_t lds = 0;
  int dim0 = 0, ntiles = 0;
  size_t ws_bytes = 0;          // workspace this launch needs (0: none); sized per launch, never summed
  long long ws_stride = 0;      // MtgParams::ws_stride of the workspace kernels
  int input_kind = -1;          // mtg_input_kind of the layout (the dimension-in-lane launch functions' `aos`)
  MtgLdsAttr attr = MtgLdsAttr::kNone;
  bool user_ws_param = false;   // static kernels: MtgParams::ws = the caller's workspace (unused; measurement builds park timestamps there)
};

// The decision for one call: the form and its launches.  More than one launch only for generic kernels (or the generic update) with
// D > 4: dimensions in groups of four, n - 1 launches of launch[0] at dim0 = 0, 4, ... and the remaining dimensions as launch[1].
struct MtgLaunchPlan {
  MtgForm form = MtgForm::kGeneric;
  int n = 0;
  MtgLaunch launch[2];
  const char* error = nullptr;  // no kernel for the call (MTG_ERR_UNSUPPORTED)
  MtgLaunch at(int i) const {
    MtgLaunch l = launch[(n > 1 && i == n - 1) ? 1 : 0];
    l.dim0 = 4 * i;
    return l;
  }
};

inline int64_t mtg_tiles(int64_t n, int64_t per) { return (n + per - 1) / per; }   // tiles of `per` trajectories
// rows of a SoA buffer padded to the next multiple of 16 trajectories (mtg_layout_soa_padded)
inline int64_t mtg_padded16(int64_t batch) { return (batch + 15) & ~(int64_t)15; }
// The static dimension-in-lane kernels address their inputs with 32-bit byte offsets.  padded: over the padded row stride (single
// and queue launches, which also read padded SoA); the mixed request, canonical layouts only, checks the batch as it is.
inline bool mtg_dl_offsets_fit(const MtgPlanForms& f, int64_t batch, bool padded) {
  return (padded ? mtg_padded16(batch) : batch) * 8 * (int64_t)std::max(f.K, f.n_fixed * f.D) < (1ll << 32);
}
// "All workgroups resident at once at <= 2 waves per SIMD": the dimension-split form's default range and, the same count, where
// every workgroup finishes at about the same time so that write-through stores avoid the serial end-of-kernel L2 write-back.
inline bool mtg_all_resident(long long tiles, int groups, int n_cu) { return tiles * groups <= 4ll * n_cu; }
// LDS of the LDS-staged output: one coefficient staging buffer per wave (64 rows x an odd number of 16-byte chunks) ...
inline size_t mtg_stage_lds_bytes(int dims, int N) { return (size_t)64 * ((size_t)(dims * N / 2) | 1) * 2 * sizeof(double); }
// ... and of the fused family's solve kernels: two of them + the two directions' exchange buffers
inline size_t mtg_solve_lds_bytes(int dims, int N, int free_mid) {
  return 2 * mtg_stage_lds_bytes(dims, N) + (size_t)2 * (free_mid * (free_mid + 1) / 2 + dims * free_mid) * kWave * sizeof(double);
}
// Persistent grid over equal-cost tiles: with `cap` resident workgroups the launch takes ceil(ntiles / cap) rounds whatever
// the grid; spreading the tiles evenly over those rounds (grid = ceil(ntiles / rounds) <= cap) keeps the rounds, and
// every round runs with fewer workgroups competing for HBM (a 20 x 10k queue: 3140 tiles = 6.13 rounds of 512 -> 7 rounds
// of 449 instead of 6 full rounds and a 13 %-full one).  MTG_NO_BALANCE: the full grid (A/B runs).
inline int mtg_balanced_grid(const MtgKnobs& kn, int ntiles, int cap) {
  if (ntiles <= cap || kn.no_balance) return std::min(ntiles, cap);
  const long long rounds = ((long long)ntiles + cap - 1) / cap;   // (64-bit: a queue's tile count may be just below 2^31)
  return (int)((ntiles + rounds - 1) / rounds);
}
// Input layout kinds the dimension-in-lane kernels read: 0 = canonical SoA (times[K][B], d_fixed[D][n_fixed][B]), 1 = canonical
// AoS (times[B][K], d_fixed[B][D][n_fixed]: the reference's natural order), 2 = SoA with the row stride padded to the next
// multiple of 16 trajectories (mtg_layout_soa_padded; the static variants' single and queue launches only), -1 = anything else
// (fused / generic kernels).
inline int mtg_input_kind(const MtgPlanForms& f, const mtg_layout* L, int64_t batch) {
  if (L->times_stride_b == 1 && L->times_stride_k == batch && L->fixed_stride_b == 1 && L->fixed_stride_c == batch &&
      L->fixed_stride_d == (int64_t)f.n_fixed * batch)
    return 0;
  const int64_t bs = mtg_padded16(batch);
  if (bs != batch && L->times_stride_b == 1 && L->times_stride_k == bs && L->fixed_stride_b == 1 && L->fixed_stride_c == bs &&
      L->fixed_stride_d == (int64_t)f.n_fixed * bs)
    return 2;
  if (L->times_stride_b == f.K && L->times_stride_k == 1 && L->fixed_stride_b == (int64_t)f.D * f.n_fixed &&
      L->fixed_stride_c == 1 && L->fixed_stride_d == f.n_fixed)
    return 1;
  return -1;
}

// default range of the dimension-in-lane form (mtg_dimlane_variants.inc): LO * CUs <= workgroups <= HI * CUs / 2
// (HI = 0: no upper limit; HI = 3 = 1.5 workgroups per CU, the measured cross-over against the slab-output fused kernel)
inline bool mtg_dimlane_is_default(const MtgKnobs& kn, int n_cu, const MtgDimlaneEntry* dl, int64_t trajectories) {
  const int64_t units = ((trajectories + dl->tpw - 1) / dl->tpw + dl->np - 1) / dl->np, cus = n_cu;
  const int hi = kn.dl_max_units_per_cu >= 0 ? 2 * kn.dl_max_units_per_cu : dl->hi_per_cu;
  if (units < (int64_t)dl->lo_per_cu * cus) return false;
  return hi == 0 || 2 * units <= (int64_t)hi * cus;
}

// The dimension-in-lane form applies to: a plan with a matching variant, canonical inputs (kinds 0 - 2), sizes whose 32-bit byte
// offsets cannot overflow.  Chosen by default while the launch is at most a few workgroups per CU (measured cross-over against
// the fused form: DESIGN.md section 4); MTG_FLAG_DIMLANE forces it, MTG_FLAG_FUSED_DIMS / MTG_FLAG_SPLIT_DIMS /
// MTG_FLAG_GENERIC_KERNEL exclude it.
inline const MtgDimlaneEntry* mtg_pick_dimlane(const MtgPlanForms& f, const MtgKnobs& kn, int n_cu, const MtgCall& c) {
  const MtgDimlaneEntry* dl = f.dimlane;
  if (!dl || kn.no_dimlane || c.cost_only) return nullptr;
  // extra outputs (cost / d_P): the main-table variants have a kernel for them (round 3; MTG_NO_DL_EXTRA: as before, through
  // the fused kernels)
  if (c.extra && (!dl->launch_extra || kn.no_dl_extra)) return nullptr;
  // (N = 12 / K = 32 with extra outputs spills 544 registers: 110 vs 128 us at 10k, but 542 vs 443 us at 50k against the
  // rolled fused kernel -- profiles/r03r_k32_extra_outputs.jsonl)
  if (c.extra && dl->h == 6 && dl->k == 32 && c.batch > 20000 && !(c.flags & MTG_FLAG_DIMLANE)) return nullptr;
  if (c.flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS)) return nullptr;
  if (mtg_input_kind(f, c.L, c.batch) < 0) return nullptr;
  if (!mtg_dl_offsets_fit(f, c.batch, true)) return nullptr;
  if (c.flags & MTG_FLAG_DIMLANE) return dl;
  return mtg_dimlane_is_default(kn, n_cu, dl, c.batch) ? dl : nullptr;
}

// The run-time-K dimension-in-lane body (mtg_dimlane_rt.h): same eligibility as the static dimension-in-lane variants
// (canonical SoA / AoS inputs, coefficient output only); taken where the plan has no static variant (K > 32, ...) -- or always /
// never with MTG_DL_RT=1 / 0.
inline const MtgDimlaneRtEntry* mtg_pick_dimlane_rt(const MtgPlanForms& f, const MtgKnobs& kn, const MtgCall& c) {
  const MtgDimlaneRtEntry* rt = f.dimlane_rt;
  if (!rt || kn.dl_rt == 0 || kn.no_dimlane || c.cost_only || c.extra) return nullptr;
  if (f.dimlane && kn.dl_rt != 1) return nullptr;
  if (c.flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS)) return nullptr;
  { const int kind = mtg_input_kind(f, c.L, c.batch); if (kind < 0 || kind > 1) return nullptr; }
  // the body keeps the batch size and its tile count in 32-bit integers (its input addresses are 64-bit, unlike the static
  // variants' 32-bit byte offsets)
  if (c.batch + rt->tpw >= (1ll << 31)) return nullptr;
  return rt;
}

// fused static form, coefficient output only: the slab-output kernel (whole-sector stores, mtg_solve_slab_kernel)
inline const MtgSlabEntry* mtg_pick_slab(const MtgPlanForms& f, const MtgKnobs& kn, const MtgStaticEntry* var) {
  if (!var || var->k <= 0 || var->d != f.D || kn.no_slab) return nullptr;
  return f.slab;
}

// Variant choice of the fused / dimension-split forms: specialised kernels when the plan matches one; with few tiles (small
// batch) the dimension-split form puts Dtot/D times as many (lighter, 2-per-SIMD) waves on the machine.  nullptr: generic.
inline const MtgStaticEntry* mtg_pick_static(const MtgPlanForms& f, const MtgKnobs& kn, int n_cu, int ntiles, uint32_t flags,
                                             bool coeffs_only) {
  if (flags & MTG_FLAG_GENERIC_KERNEL) return nullptr;
  // Coefficient output only and a slab-output fused kernel for the shape: never the dimension-split form by default.  Its
  // 80-byte pieces complete sectors from different workgroups (1.21x write amplification, read-modify-write at the memory
  // side once the output is not cache-resident): with rotating buffers 15.4 / 25.7 us at B = 10k / 20k against 10.4 / 14.3 us
  // (profiles/r02_sweep_forms.txt).  Round 2 still sent SoA batches between 1.5 workgroups per CU of the dimension-in-lane
  // form (~16k) and 4 x CUs split-form workgroups (~21.8k) to the split form (found with mtg_plan_launch_form).
  if (coeffs_only && !(flags & MTG_FLAG_SPLIT_DIMS) && kn.force_dg <= 0 && !kn.prefer_rolled && mtg_pick_slab(f, kn, f.fast))
    return f.fast;
  // Dimension-split form while ALL its workgroups (tiles x dimension groups) are resident at once at <= 2 waves per
  // SIMD (4 x CUs workgroups); beyond that it runs in rounds and the fused form -- no repeated factorisation, one
  // round up to 2 x CUs tiles -- wins (measured, N = 10 / K = 8 / D = 3: B = 20k 15.0 vs 15.4 us, B = 30k 25.5 vs
  // 18.3 us, B = 60k 44.1 vs 34.3 us).  Plans whose fused kernel spills ("heavy") keep the split form longer.
  bool auto_split = ntiles < 4 * n_cu;
  if (f.fast && f.fast_split && !f.fast->heavy) auto_split = mtg_all_resident(ntiles, f.D / f.fast_split->d, n_cu);
  const bool want_split = (flags & MTG_FLAG_SPLIT_DIMS) || (!(flags & MTG_FLAG_FUSED_DIMS) && auto_split);
  const MtgStaticEntry* var = (want_split && f.fast_split) ? f.fast_split : (f.fast ? f.fast : f.fast_split);
  if (var && var->heavy && !want_split && f.rolled) var = f.rolled;   // large launch, spilling static kernel: the rolled form is faster
  if (kn.prefer_rolled && f.rolled) var = f.rolled;
  // (the kernel tables hold dimension groups of 1 .. 4 only -- a lane keeps a group's rows in registers -- so group[] is all
  // that "force_dg" can find)
  if (kn.force_dg > 0 && kn.force_dg <= 4 && f.D % kn.force_dg == 0 && f.group[kn.force_dg]) var = f.group[kn.force_dg];
  return var;
}

// The row-cooperative form (mtg_coop.hip): standard shapes (end vertices fully fixed, position-only interior vertices), D = 3,
// coefficient output only, non-negative strides, 32-bit input / output offsets, the step storage of the chain within one CU's LDS.
// Default range = where it was measured faster than the lane-per-half forms (profiles/r04d_coop_vs_default.jsonl: 0.54-0.87 of
// their time): LONG chains in launches of at most one 2-wave workgroup per CU -- a chain step costs ~2.4x the lane-instructions
// here, but its latency is ~1.2 us against 1.8-2.6 us, and four trajectory-halves share a wavefront instead of 21-64.
//   N = 12: K >= 16 (K >= 32: up to two workgroups per CU);  N = 10: K >= 64;  N = 8: K >= 80;
//   workgroups (four trajectories each) <= CUs x that factor, and all of them resident at once (LDS).
// MTG_FLAG_COOPERATIVE forces the form wherever it is eligible; option "coop" = 0 takes it out of the default choice, 1 makes
// it the choice wherever eligible.
inline bool mtg_pick_coop(const MtgPlanForms& f, const MtgKnobs& kn, int n_cu, const MtgCall& c) {
  if (f.D != 3 || f.H < 4 || f.H > 6 || f.K < 2 || c.cost_only || c.extra || c.pert || !f.coop_shape) return false;
  if (f.coop_lds == 0 || f.coop_lds > 160 * 1024) return false;
  const mtg_layout* L = c.L;
  if (L->times_stride_b < 0 || L->times_stride_k < 0 || L->fixed_stride_b < 0 || L->fixed_stride_d < 0 || L->fixed_stride_c < 0) return false;
  const int64_t tmax = (c.batch - 1) * L->times_stride_b + (int64_t)(f.K - 1) * L->times_stride_k;
  const int64_t fmax = (c.batch - 1) * L->fixed_stride_b + (int64_t)(f.D - 1) * L->fixed_stride_d + (int64_t)(f.n_fixed - 1) * L->fixed_stride_c;
  if (tmax * 8 >= (1ll << 32) || fmax * 8 >= (1ll << 32) || c.batch * f.K * f.D * (2 * f.H) * 8 >= (1ll << 32)) return false;
  if (c.flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_DIMLANE)) return false;
  if ((c.flags & MTG_FLAG_COOPERATIVE) || kn.coop == 1) return true;
  if (kn.coop == 0 || kn.dl_rt == 1) return false;   // (option "dl_rt" = 1 asks for the run-time-K body)
  const int kmin = f.H == 6 ? 16 : (f.H == 5 ? 64 : 80);
  if (f.K < kmin) return false;
  const int64_t wgs = (c.batch + 3) / 4;
  const int64_t resident = (int64_t)(160 * 1024 / f.coop_lds);   // workgroups per CU the LDS holds
  const int64_t per_cu = std::min<int64_t>((f.H == 6 && f.K >= 32) ? 2 : 1, resident);
  return wgs <= per_cu * n_cu;
}

// Grid and workspace of a static dimension-in-lane launch over ntiles tiles.  grid_per_cu: workgroups per CU of the variants
// without a workspace.  Long chains: part of the back-substitution data goes through the workspace; persistent workgroups only
// (two 2-wave workgroups per CU, one wave per SIMD), so the workspace stays small enough to live in the Infinity Cache.
inline MtgLaunch mtg_dimlane_launch(const MtgDimlaneEntry* dl, int n_cu, int grid_per_cu, int ntiles, int input_kind) {
  MtgLaunch l;
  l.dl = dl;
  l.ntiles = ntiles;
  const int units = (ntiles + dl->np - 1) / dl->np;
  l.grid = std::min(units, n_cu * grid_per_cu);
  if (dl->ws_per_lane) {
    l.grid = std::min(units, n_cu * 4 / (2 * dl->np));
    l.ws_bytes = dl->ws_per_lane * (size_t)l.grid * dl->np * 2 * kWave;
  }
  l.input_kind = input_kind;
  return l;
}

// Which form a call takes and how it is launched: the update-from-free kernels; the row-cooperative form in its range; the
// run-time-K dimension-in-lane body where the plan has no static variant; the static dimension-in-lane variants inside their
// default range (or forced); else the fused family -- slab-output kernel (whole-sector stores) where the shape has one, else
// static (fused / dimension-split), rolled (run-time K, workspace) or generic (run-time masks) kernels.
inline MtgLaunchPlan mtg_launch_plan(const MtgPlanForms& f, const MtgKnobs& kn, int n_cu, const MtgCall& c) {
  MtgLaunchPlan lp;
  const int N = 2 * f.H;
  // 64-trajectory tiles (x (K + 1) virtual problems for perturbed-time launches)
  const int ntiles = (int)mtg_tiles(c.batch, kWave) * (c.pert ? f.K + 1 : 1);
  const int ngen = (f.D + 3) / 4;                                  // launches of the generic kernels: four dimensions each
  const int gen_dims[2] = {std::min(4, f.D), f.D - 4 * (ngen - 1)};
  lp.n = 1;
  if (c.update) {
    // setFreeConstraints path (LIN:500-508): compile-time-mask ("rolled") update kernel when the plan has one (all D dimensions
    // in one launch), else generic
    lp.form = MtgForm::kUpdate;
    const MtgStaticEntry* uv = (c.flags & MTG_FLAG_GENERIC_KERNEL) ? nullptr : f.rolled;
    if (!uv) lp.n = ngen;
    for (int i = 0; i < std::min(lp.n, 2); ++i) {
      MtgLaunch& l = lp.launch[i];
      const int dc = uv ? f.D : gen_dims[i];
      l.fn = uv ? uv->upd[c.extra ? 1 : 0] : f.generic_update[dc][c.extra ? 1 : 0];
      if (!l.fn) lp.error = "no update kernel";
      l.ntiles = ntiles;
      l.grid = std::min(ntiles, n_cu * 16);
      l.block = kWave;
      l.lds = mtg_stage_lds_bytes(dc, N);
      // whole-sector output (mtg_update_slab_kernel) for the rolled form; "no_slab" keeps the per-segment staging
      const int phase = ((size_t)f.K * f.D * N * 8) % 64 != 0 ? 1 : 0;
      if (uv && !kn.no_slab && uv->upd_slab[c.extra ? 1 : 0][phase] && uv->upd_slab_lds <= 64 * 1024) {
        l.fn = uv->upd_slab[c.extra ? 1 : 0][phase];
        l.lds = uv->upd_slab_lds;
      }
    }
    return lp;
  }
  if (mtg_pick_coop(f, kn, n_cu, c)) {
    // one 2-wave workgroup per four trajectories, step storage in LDS
    lp.form = MtgForm::kCoop;
    lp.launch[0].coop = true;
    return lp;
  }
  if (const MtgDimlaneRtEntry* rt = mtg_pick_dimlane_rt(f, kn, c)) {
    // persistent 2-wave workgroups, two per CU; the head steps beyond the register tail and the LDS step area go through a
    // lane-coalesced workspace (slots j - 1 of all head steps)
    lp.form = MtgForm::kDimlaneRt;
    MtgLaunch& l = lp.launch[0];
    l.rt = rt;
    l.ntiles = (int)mtg_tiles(c.batch, rt->tpw);
    l.grid = std::min(l.ntiles, n_cu * 2);
    const int kc_max = (f.K + 1) / 2;
    if (kc_max - 1 - rt->r_steps - rt->l_steps > 0)
      l.ws_bytes = rt->step_bytes_per_lane * (size_t)(kc_max - 1 - rt->r_steps) * (size_t)l.grid * 2 * kWave;
    l.input_kind = mtg_input_kind(f, c.L, c.batch);
    return lp;
  }
  if (const MtgDimlaneEntry* dl = mtg_pick_dimlane(f, kn, n_cu, c)) {
    // all dimensions of a trajectory in one wave, whole-sector coefficient stores
    lp.form = MtgForm::kDimlane;
    lp.launch[0] = mtg_dimlane_launch(dl, n_cu, kn.dl_grid_per_cu, (int)mtg_tiles(c.batch, dl->tpw), mtg_input_kind(f, c.L, c.batch));
    return lp;
  }
  const MtgStaticEntry* var = mtg_pick_static(f, kn, n_cu, ntiles, c.flags, !c.extra && !c.cost_only && !c.pert);
  const MtgSlabEntry* slab = (c.cost_only || c.pert) ? nullptr : mtg_pick_slab(f, kn, var);
  if (slab && c.extra && (!slab->extra || kn.no_slab_extra)) slab = nullptr;
  if (slab) {
    // (extra outputs -- cost / d_P -- through the slab-output kernel as well: the older fused kernel's 240-byte pieces
    // complete most sectors from two store instructions, 80-83 us at B = 125k with rotating buffers)
    lp.form = MtgForm::kSlab;
    MtgLaunch& l = lp.launch[0];
    const int pol = kn.slab_policy >= 0 ? kn.slab_policy : 1;
    l.fn = c.extra ? slab->extra : slab->fn[pol];
    l.attr = c.extra ? MtgLdsAttr::kSlabExtra : (pol ? MtgLdsAttr::kSlabNt : MtgLdsAttr::kSlabWriteBack);
    l.ntiles = ntiles;
    l.grid = mtg_balanced_grid(kn, ntiles, n_cu * 2);   // 63.5 KB of LDS per workgroup: two per CU, one wave per SIMD
    l.lds = slab->lds;
    return lp;
  }
  const int kc = (f.K + 1) / 2;
  if (var) {
    lp.form = var->k < 0 ? MtgForm::kRolled : (var->d == f.D ? MtgForm::kFused : MtgForm::kSplit);
    MtgLaunch& l = lp.launch[0];
    const int ngroups = f.D / var->d;
    // few tiles => every workgroup finishes at about the same time: write-through stores avoid the serial
    // end-of-kernel L2 write-back; many tiles => plain write-back stores are faster
    const bool write_through = mtg_all_resident(ntiles, ngroups, n_cu);
    l.fn = c.cost_only ? var->fn[4] : var->fn[(c.extra ? 1 : 0) + (write_through ? 2 : 0)];
    l.ntiles = ntiles;
    l.grid = std::min(ntiles, std::max(1, n_cu * 8 / ngroups));
    l.gridy = ngroups;
    l.user_ws_param = true;
    if (var->k < 0) {   // rolled kernels stream (G, g) through the workspace
      l.grid = std::min(ntiles, std::max(1, n_cu * kn.rolled_wg_per_cu / ngroups));
      l.ws_stride = (long long)l.grid * ngroups * kBlock;
      l.ws_bytes = (size_t)kc * ((size_t)f.H * f.H + (size_t)var->d * f.H) * (size_t)l.ws_stride * sizeof(double);
    }
    l.lds = mtg_solve_lds_bytes(var->d, N, f.free_mid);
    return lp;
  }
  lp.form = MtgForm::kGeneric;
  lp.n = ngen;
  for (int i = 0; i < std::min(lp.n, 2); ++i) {
    MtgLaunch& l = lp.launch[i];
    const int dc = gen_dims[i];
    l.fn = f.generic_solve[dc][c.cost_only ? 2 : (c.extra ? 1 : 0)];
    if (!l.fn) lp.error = "no generic kernel";
    l.ntiles = ntiles;
    l.grid = std::min(ntiles, n_cu * 4);
    l.ws_stride = (long long)l.grid * kBlock;   // generic kernels stream (G, g) through the workspace as well
    l.ws_bytes = (size_t)kc * ((size_t)f.H * f.H + (size_t)dc * f.H) * (size_t)l.ws_stride * sizeof(double);
    l.lds = mtg_solve_lds_bytes(dc, N, f.free_mid);
  }
  return lp;
}

// mtg_solve_linear_sequence as persistent launches of up to kSeqMax batches, coefficient output only: the slab-output fused
// kernel or the dimension-in-lane kernel, chosen by the TOTAL number of trajectories of a launch the way single launches choose
// by their batch.  Neither set: the call does not qualify (one launch per batch).
struct MtgQueuePlan {
  const MtgSlabEntry* slab = nullptr;
  const MtgDimlaneEntry* dl = nullptr;   // wins where both are set
  int tiles_per_batch = 0, input_kind = -1;
};
inline MtgQueuePlan mtg_queue_plan(const MtgPlanForms& f, const MtgKnobs& kn, int n_cu, int32_t n, int64_t batch, const mtg_layout* L,
                                   uint32_t flags) {
  MtgQueuePlan q;
  if (n < 2 || batch <= 0 || kn.no_queue) return q;
  if (flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH)) return q;
  const int32_t n_launch = std::min<int32_t>(n, kSeqMax);       // batches per launch
  q.slab = (flags & MTG_FLAG_DIMLANE) ? nullptr : mtg_pick_slab(f, kn, f.fast);
  if (q.slab && (!q.slab->queue || mtg_tiles(batch, kWave) * (int64_t)n_launch >= (1ll << 31))) q.slab = nullptr;
  q.dl = f.dimlane;
  if (q.dl && (!q.dl->launch_queue || kn.no_dimlane || (flags & MTG_FLAG_FUSED_DIMS))) q.dl = nullptr;
  q.input_kind = mtg_input_kind(f, L, batch);
  if (q.dl && (q.input_kind < 0 || !mtg_dl_offsets_fit(f, batch, true) || mtg_tiles(batch, q.dl->tpw) * (int64_t)n_launch >= (1ll << 31)))
    q.dl = nullptr;
  if (q.slab && q.dl && !(flags & MTG_FLAG_DIMLANE) && !mtg_dimlane_is_default(kn, n_cu, q.dl, batch * (int64_t)n_launch)) q.dl = nullptr;
  q.tiles_per_batch = (int)mtg_tiles(batch, q.dl ? q.dl->tpw : kWave);
  return q;
}
// One launch of the queue over n_batches (<= kSeqMax) batches.  The dimension-in-lane grid without a workspace is 8 x CUs here,
// whatever option "dl_grid_per_cu" says: a recorded difference from the single launch, kept as it is.
inline MtgLaunch mtg_queue_launch(const MtgQueuePlan& q, const MtgKnobs& kn, int n_cu, int n_batches) {
  const int ntiles = n_batches * q.tiles_per_batch;
  if (q.dl) return mtg_dimlane_launch(q.dl, n_cu, 8, ntiles, q.input_kind);
  MtgLaunch l;
  l.ntiles = ntiles;
  l.grid = mtg_balanced_grid(kn, ntiles, n_cu * 2);   // two workgroups per CU, one wave per SIMD (as the single-batch launch)
  l.lds = q.slab->lds;
  l.attr = MtgLdsAttr::kSlabQueue;
  return l;
}

#endif  // MTG_LAUNCH_PLAN_H_
