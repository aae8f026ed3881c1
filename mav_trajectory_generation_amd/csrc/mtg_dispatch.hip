// mtg_dispatch.hip -- the C ABI of include/mtg_hip.h, part 3: form choice (pick_*), launchers, host-pointer staging and the one
// solve / update call behind every entry (mtg_solve_impl); sequence, Mellinger, update and objective-solve entries; launch reports.
#include "mtg_abi_internal.h"

#define MTG_DECL(H) SolveFn mtg_pick_generic_solve_h##H(int, int); UpdateFn mtg_pick_generic_update_h##H(int, bool);
MTG_DECL(1) MTG_DECL(2) MTG_DECL(3) MTG_DECL(4) MTG_DECL(5) MTG_DECL(6)
#undef MTG_DECL

SolveFn mtg_pick_generic_solve(int h, int d, int extra) {
  static SolveFn (*const pick[6])(int, int) = {mtg_pick_generic_solve_h1, mtg_pick_generic_solve_h2, mtg_pick_generic_solve_h3,
                                               mtg_pick_generic_solve_h4, mtg_pick_generic_solve_h5, mtg_pick_generic_solve_h6};
  return h >= 1 && h <= 6 ? pick[h - 1](d, extra) : nullptr;
}
UpdateFn mtg_pick_generic_update(int h, int d, bool wc) {
  static UpdateFn (*const pick[6])(int, bool) = {mtg_pick_generic_update_h1, mtg_pick_generic_update_h2, mtg_pick_generic_update_h3,
                                                 mtg_pick_generic_update_h4, mtg_pick_generic_update_h5, mtg_pick_generic_update_h6};
  return h >= 1 && h <= 6 ? pick[h - 1](d, wc) : nullptr;
}

static int64_t span(int64_t batch, int64_t sb, int64_t n1, int64_t s1, int64_t n2, int64_t s2) {
  return (batch - 1) * sb + (n1 - 1) * s1 + (n2 - 1) * s2 + 1;
}

// The dimension-in-lane form applies to: a plan with a matching variant, canonical SoA inputs (times[K][B],
// d_fixed[D][n_fixed][B]), coefficient output only, sizes whose 32-bit byte offsets cannot overflow.  Chosen by default
// while the launch is at most a few workgroups per CU (measured cross-over against the fused form: DESIGN.md section 4);
// MTG_FLAG_DIMLANE forces it, MTG_FLAG_FUSED_DIMS / MTG_FLAG_SPLIT_DIMS / MTG_FLAG_GENERIC_KERNEL exclude it.
// Persistent grid over equal-cost tiles: with `cap` resident workgroups the launch takes ceil(ntiles / cap) rounds whatever
// the grid; spreading the tiles evenly over those rounds (grid = ceil(ntiles / rounds) <= cap) keeps the rounds, and
// every round runs with fewer workgroups competing for HBM (a 20 x 10k queue: 3140 tiles = 6.13 rounds of 512 -> 7 rounds
// of 449 instead of 6 full rounds and a 13 %-full one).  MTG_NO_BALANCE: the full grid (A/B runs).
static int balanced_grid(const mtg_context* ctx, int ntiles, int cap) {
  if (ntiles <= cap || ctx->knob_no_balance) return std::min(ntiles, cap);
  const int rounds = (ntiles + cap - 1) / cap;
  return (ntiles + rounds - 1) / rounds;
}

// default range of the dimension-in-lane form (mtg_dimlane_variants.inc): LO * CUs <= workgroups <= HI * CUs / 2
// (HI = 0: no upper limit; HI = 3 = 1.5 workgroups per CU, the measured cross-over against the slab-output fused kernel)
static bool dimlane_is_default(const mtg_plan* p, const MtgDimlaneEntry* dl, int64_t trajectories) {
  const int64_t units = ((trajectories + dl->tpw - 1) / dl->tpw + dl->np - 1) / dl->np;
  const int64_t cus = p->ctx->n_cu;
  const int hi = p->ctx->dl_max_units_per_cu >= 0 ? 2 * p->ctx->dl_max_units_per_cu : dl->hi_per_cu;
  if (units < (int64_t)dl->lo_per_cu * cus) return false;
  return hi == 0 || 2 * units <= (int64_t)hi * cus;
}

// Input layout kinds the dimension-in-lane kernels read: 0 = canonical SoA (times[K][B], d_fixed[D][n_fixed][B]), 1 = canonical
// AoS (times[B][K], d_fixed[B][D][n_fixed]: the reference's natural order), 2 = SoA with the row stride padded to the next
// multiple of 16 trajectories (mtg_layout_soa_padded; the static variants' single and queue launches only), -1 = anything else
// (fused / generic kernels).
int mtg_dimlane_input_kind(const mtg_plan* p, const mtg_layout* L, int64_t batch) {
  if (L->times_stride_b == 1 && L->times_stride_k == batch && L->fixed_stride_b == 1 && L->fixed_stride_c == batch &&
      L->fixed_stride_d == (int64_t)p->n_fixed * batch)
    return 0;
  const int64_t bs = mtg_padded16(batch);
  if (bs != batch && L->times_stride_b == 1 && L->times_stride_k == bs && L->fixed_stride_b == 1 && L->fixed_stride_c == bs &&
      L->fixed_stride_d == (int64_t)p->n_fixed * bs)
    return 2;
  if (L->times_stride_b == p->K && L->times_stride_k == 1 && L->fixed_stride_b == (int64_t)p->D * p->n_fixed &&
      L->fixed_stride_c == 1 && L->fixed_stride_d == p->n_fixed)
    return 1;
  return -1;
}

static const MtgDimlaneEntry* pick_dimlane(const mtg_plan* p, int64_t batch, const mtg_layout* L, const MtgParams& P,
                                           uint32_t flags, bool cost_only) {
  const MtgDimlaneEntry* dl = p->dimlane;
  if (!dl || p->ctx->knob_no_dimlane || cost_only) return nullptr;
  // extra outputs (cost / d_P): the main-table variants have a kernel for them (round 3; MTG_NO_DL_EXTRA: as before, through
  // the fused kernels)
  if ((P.dfree || P.cost) && (!dl->launch_extra || p->ctx->knob_no_dl_extra)) return nullptr;
  // (N = 12 / K = 32 with extra outputs spills 544 registers: 110 vs 128 us at 10k, but 542 vs 443 us at 50k against the
  // rolled fused kernel -- profiles/r03r_k32_extra_outputs.jsonl)
  if ((P.dfree || P.cost) && dl->h == 6 && dl->k == 32 && batch > 20000 && !(flags & MTG_FLAG_DIMLANE)) return nullptr;
  if (flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS)) return nullptr;
  if (mtg_dimlane_input_kind(p, L, batch) < 0) return nullptr;
  if (mtg_padded16(batch) * 8 * (int64_t)std::max(p->K, p->n_fixed * p->D) >= (1ll << 32)) return nullptr;
  if (flags & MTG_FLAG_DIMLANE) return dl;
  return dimlane_is_default(p, dl, batch) ? dl : nullptr;
}

// The run-time-K dimension-in-lane body (mtg_dimlane_rt.h): same eligibility as the static dimension-in-lane variants
// (canonical SoA inputs, coefficient output only); taken where the plan has no static variant (K > 32, ...) -- or always /
// never with MTG_DL_RT=1 / 0.
static const MtgDimlaneRtEntry* pick_dimlane_rt(const mtg_plan* p, int64_t batch, const mtg_layout* L, const MtgParams& P,
                                                uint32_t flags, bool cost_only) {
  const MtgDimlaneRtEntry* rt = p->dimlane_rt;
  if (!rt || p->ctx->knob_dl_rt == 0 || p->ctx->knob_no_dimlane || cost_only || P.dfree || P.cost) return nullptr;
  if (p->dimlane && p->ctx->knob_dl_rt != 1) return nullptr;
  if (flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS)) return nullptr;
  { const int kind = mtg_dimlane_input_kind(p, L, batch); if (kind < 0 || kind > 1) return nullptr; }
  // the body keeps the batch size and its tile count in 32-bit integers (its input addresses are 64-bit, unlike the static
  // variants' 32-bit byte offsets)
  if (batch + rt->tpw >= (1ll << 31)) return nullptr;
  return rt;
}

// fused static form, coefficient output only: the slab-output kernel (whole-sector stores, mtg_solve_slab_kernel)
static const MtgSlabEntry* pick_slab(const mtg_plan* p, const MtgStaticEntry* var) {
  if (!var || var->k <= 0 || var->d != p->D || p->ctx->knob_no_slab) return nullptr;
  return mtg_find_slab(p->H, p->D, p->K, p->deriv, p->mask.data());
}

// Variant choice of the fused / dimension-split forms: specialised kernels when the plan matches one; with few tiles (small
// batch) the dimension-split form puts Dtot/D times as many (lighter, 2-per-SIMD) waves on the machine.  nullptr: generic.
static const MtgStaticEntry* pick_static(const mtg_plan* p, int ntiles, uint32_t flags, bool coeffs_only) {
  const mtg_context* ctx = p->ctx;
  const MtgStaticEntry* var = nullptr;
  if (flags & MTG_FLAG_GENERIC_KERNEL) return nullptr;
  // Coefficient output only and a slab-output fused kernel for the shape: never the dimension-split form by default.  Its
  // 80-byte pieces complete sectors from different workgroups (1.21x write amplification, read-modify-write at the memory
  // side once the output is not cache-resident): with rotating buffers 15.4 / 25.7 us at B = 10k / 20k against 10.4 / 14.3 us
  // (profiles/r02_sweep_forms.txt).  Round 2 still sent SoA batches between 1.5 workgroups per CU of the dimension-in-lane
  // form (~16k) and 4 x CUs split-form workgroups (~21.8k) to the split form (found with mtg_plan_launch_form).
  if (coeffs_only && !(flags & MTG_FLAG_SPLIT_DIMS) && ctx->knob_force_dg <= 0 && !ctx->knob_prefer_rolled && pick_slab(p, p->fast))
    return p->fast;
  // Dimension-split form while ALL its workgroups (tiles x dimension groups) are resident at once at <= 2 waves per
  // SIMD (4 x CUs workgroups); beyond that it runs in rounds and the fused form -- no repeated factorisation, one
  // round up to 2 x CUs tiles -- wins (measured, N = 10 / K = 8 / D = 3: B = 20k 15.0 vs 15.4 us, B = 30k 25.5 vs
  // 18.3 us, B = 60k 44.1 vs 34.3 us).  Plans whose fused kernel spills ("heavy") keep the split form longer.
  bool auto_split = ntiles < 4 * ctx->n_cu;
  if (p->fast && p->fast_split && !p->fast->heavy)
    auto_split = (long long)ntiles * (p->D / p->fast_split->d) <= 4ll * ctx->n_cu;
  const bool want_split = (flags & MTG_FLAG_SPLIT_DIMS) || (!(flags & MTG_FLAG_FUSED_DIMS) && auto_split);
  var = (want_split && p->fast_split) ? p->fast_split : (p->fast ? p->fast : p->fast_split);
  if (var && var->heavy && !want_split) {   // large launch, spilling static kernel: the rolled form is faster
    const MtgStaticEntry* v = mtg_find_static(p->H, p->D, p->K, p->deriv, p->mask.data(), true);
    if (v) var = v;
  }
  if (ctx->knob_prefer_rolled) {
    const MtgStaticEntry* v = mtg_find_static(p->H, p->D, p->K, p->deriv, p->mask.data(), true);
    if (v) var = v;
  }
  if (ctx->knob_force_dg > 0) {
    const int dg = ctx->knob_force_dg;
    if (p->D % dg == 0) {
      const MtgStaticEntry* v = mtg_find_static(p->H, dg, p->K, p->deriv, p->mask.data());
      if (v) var = v;
    }
  }
  return var;
}

static int workspace(mtg_plan* p, size_t need, double** out) {
  mtg_context* ctx = p->ctx;
  if (p->user_ws) {
    if (p->user_ws_bytes < need) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "user workspace too small");
    *out = p->user_ws;
    return MTG_OK;
  }
  const int rc = ensure_buffer(ctx, &p->ws, &p->ws_bytes, need);
  if (rc == MTG_OK) *out = p->ws;
  return rc;
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
static bool coop_eligible(const mtg_plan* p, int64_t batch, const mtg_layout* L, const MtgParams& P, bool cost_only) {
  if (p->D != 3 || p->H < 4 || p->H > 6 || p->K < 2 || cost_only || P.dfree || P.cost || P.pert_on) return false;
  const int full = (1 << p->H) - 1;
  if (p->mask[0] != full || p->mask[p->K] != full) return false;
  for (int v = 1; v < p->K; ++v) if (p->mask[v] != 1) return false;
  const size_t lds = mtg_coop_lds_bytes(p->H, p->D, p->K);
  if (lds == 0 || lds > 160 * 1024) return false;
  if (L->times_stride_b < 0 || L->times_stride_k < 0 || L->fixed_stride_b < 0 || L->fixed_stride_d < 0 || L->fixed_stride_c < 0) return false;
  const int64_t tmax = (batch - 1) * L->times_stride_b + (int64_t)(p->K - 1) * L->times_stride_k;
  const int64_t fmax = (batch - 1) * L->fixed_stride_b + (int64_t)(p->D - 1) * L->fixed_stride_d + (int64_t)(p->n_fixed - 1) * L->fixed_stride_c;
  return tmax * 8 < (1ll << 32) && fmax * 8 < (1ll << 32) && batch * p->K * p->D * p->N * 8 < (1ll << 32);
}
static bool pick_coop(const mtg_plan* p, int64_t batch, const mtg_layout* L, const MtgParams& P, uint32_t flags, bool cost_only) {
  if (!coop_eligible(p, batch, L, P, cost_only)) return false;
  if (flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_DIMLANE)) return false;
  if ((flags & MTG_FLAG_COOPERATIVE) || p->ctx->knob_coop == 1) return true;
  if (p->ctx->knob_coop == 0 || p->ctx->knob_dl_rt == 1) return false;   // (option "dl_rt" = 1 asks for the run-time-K body)
  const int kmin = p->H == 6 ? 16 : (p->H == 5 ? 64 : 80);
  if (p->K < kmin) return false;
  const int64_t wgs = (batch + 3) / 4;
  const int64_t resident = (int64_t)(160 * 1024 / mtg_coop_lds_bytes(p->H, p->D, p->K));   // workgroups per CU the LDS holds
  const int64_t per_cu = std::min<int64_t>((p->H == 6 && p->K >= 32) ? 2 : 1, resident);
  return wgs <= per_cu * p->ctx->n_cu;
}

// Which form a call takes: the run-time-K dimension-in-lane body where the plan has no static variant, the static
// dimension-in-lane variants inside their default range (or forced), else the fused family.  Same order as
// mtg_plan_launch_form reports.
static SolveForm pick_form(SolveCall& c, bool update_only) {
  if (update_only) return SolveForm::kUpdate;
  if (pick_coop(c.p, c.batch, c.L, c.P, c.flags, c.cost_only)) return SolveForm::kCoop;
  if ((c.rt = pick_dimlane_rt(c.p, c.batch, c.L, c.P, c.flags, c.cost_only))) return SolveForm::kDimlaneRt;
  if ((c.dl = pick_dimlane(c.p, c.batch, c.L, c.P, c.flags, c.cost_only))) return SolveForm::kDimlane;
  return SolveForm::kFused;
}

// setFreeConstraints path (LIN:500-508): compile-time-mask ("rolled") update kernel when the plan has one (all D dimensions in
// one launch), else generic
static int launch_update(SolveCall& c) {
  mtg_plan* p = c.p;
  mtg_context* ctx = p->ctx;
  const MtgStaticEntry* uv = (c.flags & MTG_FLAG_GENERIC_KERNEL) ? nullptr : mtg_find_static(p->H, p->D, p->K, p->deriv, p->mask.data(), true);
  for (int dim0 = 0; dim0 < p->D; dim0 += 4) {
    const int dc = uv ? p->D : std::min(4, p->D - dim0);
    UpdateFn fn = uv ? uv->upd[c.wc ? 1 : 0] : mtg_pick_generic_update(p->H, dc, c.wc);
    if (!fn) return set_err(ctx, MTG_ERR_UNSUPPORTED, "no update kernel");
    MtgParams Q = c.P;
    Q.dim0 = dim0;
    const int grid = std::min(c.ntiles, ctx->n_cu * 16);
    size_t lds = (size_t)64 * ((size_t)(dc * p->N / 2) | 1) * 2 * sizeof(double);
    // whole-sector output (mtg_update_slab_kernel) for the rolled form; "no_slab" keeps the per-segment staging
    const int phase = ((size_t)p->K * p->D * p->N * 8) % 64 != 0 ? 1 : 0;
    if (uv && !ctx->knob_no_slab && uv->upd_slab[c.wc ? 1 : 0][phase] && uv->upd_slab_lds <= 64 * 1024) {
      fn = uv->upd_slab[c.wc ? 1 : 0][phase];
      lds = uv->upd_slab_lds;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kWave), lds, c.st, Q, c.ntiles);
    if (uv) break;
  }
  return MTG_OK;
}

// row-cooperative form (mtg_coop.hip): one 2-wave workgroup per four trajectories, step storage in LDS
static int launch_coop(SolveCall& c) {
  mtg_plan* p = c.p;
  const MtgParams& P = c.P;
  const int rc = mtg_coop_launch((void*)c.st, p->H, p->D, p->K, p->deriv, c.batch, P.times, P.ts_b, P.ts_k, P.dfix, P.fs_b, P.fs_d, P.fs_c,
                                 P.coeffs, P.status, c.dts);
  if (rc != 0) return set_err(p->ctx, rc == 1 ? MTG_ERR_UNSUPPORTED : MTG_ERR_DEVICE, "row-cooperative launch failed");
  LaunchRecord r;
  r.valid = true; r.params = P; r.coop = true;
  p->last.push_back(r);
  return MTG_OK;
}

// run-time-K dimension-in-lane body: persistent 2-wave workgroups, two per CU; the head steps beyond the register tail and the
// LDS step area go through a lane-coalesced workspace
static int launch_dimlane_rt(SolveCall& c) {
  mtg_plan* p = c.p;
  mtg_context* ctx = p->ctx;
  const MtgDimlaneRtEntry* rt = c.rt;
  const int nt = (int)((c.batch + rt->tpw - 1) / rt->tpw);
  const int grid = std::min(nt, ctx->n_cu * 2);
  const int kc_max = (p->K + 1) / 2;
  double* rt_ws = nullptr;
  if (kc_max - 1 - rt->r_steps - rt->l_steps > 0) {      // head steps beyond the register tail and the LDS step area
    const size_t need = rt->step_bytes_per_lane * (size_t)(kc_max - 1 - rt->r_steps) * (size_t)grid * 2 * kWave;   // slots j - 1 of all head steps
    const int rc = workspace(p, need, &rt_ws);
    if (rc != MTG_OK) return rc;
  }
  const int aos = mtg_dimlane_input_kind(p, c.L, c.batch);
  if (rt->launch((void*)c.st, grid, c.P.times, c.P.dfix, c.P.coeffs, c.P.status, c.dts, (int)c.batch, p->K, nt, rt_ws, aos) != 0)
    return set_err(ctx, MTG_ERR_DEVICE, "run-time-K dimension-in-lane launch set-up failed");
  LaunchRecord r;
  r.valid = true; r.params = c.P; r.ntiles = nt; r.grid = grid; r.rt = rt; r.dl_ws = rt_ws; r.dl_aos = aos;
  p->last.push_back(r);
  return MTG_OK;
}

// the launch call of a static dimension-in-lane variant (launch_dimlane, and its replay by mtg_time_last_solve)
static int run_dimlane(const MtgDimlaneEntry* dl, hipStream_t st, int grid, const MtgParams& P, int nt, double* ws, int aos) {
  if (!P.dfree && !P.cost) return dl->launch((void*)st, grid, P.times, P.dfix, P.coeffs, P.status, P.tstatus, (int)P.B, nt, ws, aos);
  return dl->launch_extra((void*)st, grid, P.times, P.dfix, P.coeffs, P.status, P.tstatus, (int)P.B, nt, ws, aos, P.dfree, P.cost, P.ps_b, P.ps_d, P.ps_c);
}

// dimension-in-lane form (mtg_dimlane.h): all dimensions of a trajectory in one wave, whole-sector coefficient stores
static int launch_dimlane(SolveCall& c) {
  mtg_plan* p = c.p;
  mtg_context* ctx = p->ctx;
  const MtgDimlaneEntry* dl = c.dl;
  const MtgParams& P = c.P;
  const int nt = (int)((c.batch + dl->tpw - 1) / dl->tpw);
  const int units = (nt + dl->np - 1) / dl->np;
  int grid = std::min(units, ctx->n_cu * ctx->knob_dl_grid_per_cu);
  double* dl_ws = nullptr;
  if (dl->ws_per_lane) {
    // long chains: part of the back-substitution data goes through the workspace; persistent workgroups only (two
    // 2-wave workgroups per CU, one wave per SIMD), so the workspace stays small enough to live in the Infinity Cache
    grid = std::min(units, ctx->n_cu * 4 / (2 * dl->np));
    const int rc = workspace(p, dl->ws_per_lane * (size_t)grid * dl->np * 2 * kWave, &dl_ws);
    if (rc != MTG_OK) return rc;
  }
  const int aos = mtg_dimlane_input_kind(p, c.L, c.batch);
  if (run_dimlane(dl, c.st, grid, P, nt, dl_ws, aos) != 0) return set_err(ctx, MTG_ERR_DEVICE, "dimension-in-lane launch set-up failed");
  LaunchRecord r;
  r.valid = true; r.params = P; r.ntiles = nt; r.grid = grid; r.dl = dl; r.dl_ws = dl_ws; r.dl_aos = aos;
  p->last.push_back(r);
  return MTG_OK;
}

// the fused family: slab-output kernel (whole-sector stores) where the shape has one, else static (fused / dimension-split),
// rolled (run-time K, workspace) or generic (run-time masks) kernels
static int launch_fused(SolveCall& c) {
  mtg_plan* p = c.p;
  mtg_context* ctx = p->ctx;
  const bool wc = c.wc, cost_only = c.cost_only;
  const int ntiles = c.ntiles;
  hipStream_t st = c.st;
  const MtgStaticEntry* var = pick_static(p, ntiles, c.flags, !wc && !cost_only && !c.pert);
  const int vm = (p->K + 1) / 2;
  const int fm = p->H - __builtin_popcount((unsigned)p->mask[vm]);
  for (int dim0 = 0; dim0 < p->D; dim0 += 4) {
    const int dc = var ? var->d : std::min(4, p->D - dim0);
    const int ngroups = var ? p->D / var->d : 1;
    MtgParams Q = c.P;
    Q.dim0 = dim0;
    SolveFn fn;
    int grid;
    const bool needs_ws = !var || var->k < 0;   // generic and rolled kernels stream (G, g) through the workspace
    const MtgSlabEntry* slab = nullptr;
    if (!cost_only && !c.pert) slab = pick_slab(p, var);
    if (slab && wc && (!slab->extra || ctx->knob_no_slab_extra)) slab = nullptr;
    if (slab) {
      // (extra outputs -- cost / d_P -- through the slab-output kernel as well: the older fused kernel's 240-byte pieces
      // complete most sectors from two store instructions, 80-83 us at B = 125k with rotating buffers)
      const int pol = ctx->knob_slab_policy >= 0 ? ctx->knob_slab_policy : 1;
      SolveFn sfn = wc ? slab->extra : slab->fn[pol];
      bool& attr_set = wc ? p->slab_extra_attr_set : p->slab_attr_set[pol];
      const int sgrid = balanced_grid(ctx, ntiles, ctx->n_cu * 2);   // 63.5 KB of LDS per workgroup: two per CU, one wave per SIMD
      if (!attr_set) {
        MTG_HIP_TRY(ctx, hipFuncSetAttribute((const void*)sfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slab->lds));
        attr_set = true;
      }
      hipLaunchKernelGGL(sfn, dim3(sgrid), dim3(kBlock), slab->lds, st, Q, ntiles);
      LaunchRecord r;
      r.valid = true; r.fn = sfn; r.params = Q; r.ntiles = ntiles; r.grid = sgrid; r.gridy = 1; r.lds = slab->lds;
      p->last.push_back(r);
      break;
    }
    if (var) {
      Q.ws = p->user_ws;   // unused by the static kernels (measurement builds park timestamps here)
      // few tiles => every workgroup finishes at about the same time: write-through stores avoid the serial
      // end-of-kernel L2 write-back; many tiles => plain write-back stores are faster
      const bool write_through = (long long)ntiles * ngroups <= 4ll * ctx->n_cu;
      fn = cost_only ? var->fn[4] : var->fn[(wc ? 1 : 0) + (write_through ? 2 : 0)];
      grid = std::min(ntiles, std::max(1, ctx->n_cu * 8 / ngroups));
    } else {
      fn = mtg_pick_generic_solve(p->H, dc, cost_only ? 2 : (wc ? 1 : 0));
      if (!fn) return set_err(ctx, MTG_ERR_UNSUPPORTED, "no generic kernel");
      grid = std::min(ntiles, ctx->n_cu * 4);
    }
    if (needs_ws) {
      if (var) grid = std::min(ntiles, std::max(1, ctx->n_cu * ctx->rolled_wg_per_cu / ngroups));
      const int kc = (p->K + 1) / 2;
      const size_t E = (size_t)p->H * p->H + (size_t)dc * p->H;
      const int rc = workspace(p, (size_t)kc * E * (size_t)grid * ngroups * kBlock * sizeof(double), &Q.ws);
      if (rc != MTG_OK) return rc;
      Q.ws_stride = (long long)grid * ngroups * kBlock;
    }
    // LDS: two coefficient staging buffers (64 rows x odd number of 16-byte chunks) + two exchange buffers
    const size_t stage = (size_t)64 * ((size_t)(dc * p->N / 2) | 1) * 2 * sizeof(double);
    const size_t lds = 2 * stage + (size_t)2 * (fm * (fm + 1) / 2 + dc * fm) * kWave * sizeof(double);
    hipLaunchKernelGGL(fn, dim3(grid, ngroups), dim3(kBlock), lds, st, Q, ntiles);
    LaunchRecord r;
    r.valid = true; r.fn = fn; r.params = Q; r.ntiles = ntiles; r.grid = grid; r.gridy = ngroups; r.lds = lds;
    p->last.push_back(r);
    if (var) break;
  }
  return MTG_OK;
}

// Host-pointer calls: inputs staged into the plan's device area ([times | d_fixed | d_free | coeffs | cost | per-trajectory
// status | status word]; small calls through ONE page-locked bounce buffer = one H2D DMA, the kernel, one D2H DMA), outputs and
// the call's OWN status word fetched back synchronously.
struct HostStaging {
  bool bounce = false;
  int64_t n_times = 0, n_fix = 0, n_fre = 0, n_coef = 0, n_ts = 0;
  int* status_dev = nullptr;        // this call's own status word (a host-pointer call reports its status itself; it must neither
                                    // collect nor clear the flags earlier asynchronous launches left in the context's word)
  const double *dt = nullptr, *dfx = nullptr;
  double *dco = nullptr, *dfr = nullptr, *dcs = nullptr;
  int32_t* dts = nullptr;
};

static int stage_host_inputs(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed,
                             const double* d_free, bool want_cost, bool want_ts, bool update_only, hipStream_t st, HostStaging& h) {
  mtg_context* ctx = p->ctx;
  constexpr size_t kBounceLimit = 1u << 20;
  h.n_times = span(batch, L->times_stride_b, p->K, L->times_stride_k, 1, 0);
  h.n_fix = p->n_fixed ? span(batch, L->fixed_stride_b, p->D, L->fixed_stride_d, p->n_fixed, L->fixed_stride_c) : 0;
  h.n_fre = p->n_free ? span(batch, L->free_stride_b, p->D, L->free_stride_d, p->n_free, L->free_stride_c) : 0;
  h.n_coef = batch * p->K * p->D * p->N;
  h.n_ts = want_ts ? (batch + 1) / 2 : 0;   // doubles that hold `batch` int32
  const size_t need = (size_t)(h.n_times + h.n_fix + h.n_fre + h.n_coef + batch + h.n_ts + 1) * sizeof(double);
  int rc = ensure_buffer(ctx, &p->stage, &p->stage_bytes, need);
  if (rc != MTG_OK) return rc;
  double* s = p->stage;
  double* s_t = s; s += h.n_times;
  double* s_f = s; s += h.n_fix;
  double* s_p = s; s += h.n_fre;
  double* s_c = s; s += h.n_coef;
  double* s_j = s; s += batch;
  if (want_ts) h.dts = reinterpret_cast<int32_t*>(s);
  s += h.n_ts;
  h.status_dev = reinterpret_cast<int*>(s);
  const size_t n_in = (size_t)(h.n_times + h.n_fix + (update_only ? h.n_fre : 0));
  h.bounce = need <= kBounceLimit;
  if (h.bounce) {
    if (ctx->h_bounce_bytes < need) {
      if (ctx->h_bounce) hipHostFree(ctx->h_bounce);
      ctx->h_bounce = nullptr;
      ctx->h_bounce_bytes = 0;
      MTG_HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_bounce, kBounceLimit, hipHostMallocDefault));
      ctx->h_bounce_bytes = kBounceLimit;
    }
    std::memcpy(ctx->h_bounce, times, h.n_times * sizeof(double));
    if (h.n_fix) std::memcpy(ctx->h_bounce + h.n_times, d_fixed, h.n_fix * sizeof(double));
    if (update_only && h.n_fre) std::memcpy(ctx->h_bounce + h.n_times + h.n_fix, d_free, h.n_fre * sizeof(double));
    MTG_HIP_TRY(ctx, hipMemcpyAsync(s_t, ctx->h_bounce, n_in * sizeof(double), hipMemcpyHostToDevice, st));
  } else {
    MTG_HIP_TRY(ctx, hipMemcpyAsync(s_t, times, h.n_times * sizeof(double), hipMemcpyHostToDevice, st));
    if (h.n_fix) MTG_HIP_TRY(ctx, hipMemcpyAsync(s_f, d_fixed, h.n_fix * sizeof(double), hipMemcpyHostToDevice, st));
    if (update_only && h.n_fre) MTG_HIP_TRY(ctx, hipMemcpyAsync(s_p, d_free, h.n_fre * sizeof(double), hipMemcpyHostToDevice, st));
  }
  h.dt = s_t; h.dfx = s_f; h.dco = s_c;
  h.dfr = (d_free && h.n_fre) ? s_p : nullptr;
  h.dcs = want_cost ? s_j : nullptr;
  return MTG_OK;
}

static int fetch_host_outputs(mtg_plan* p, int64_t batch, double* coeffs, double* d_free, double* cost, int32_t* traj_status,
                              bool update_only, hipStream_t st, const HostStaging& h, int* host_status) {
  mtg_context* ctx = p->ctx;
  const int64_t n_times = h.n_times, n_fix = h.n_fix, n_fre = h.n_fre, n_coef = h.n_coef, n_ts = h.n_ts;
  if (h.bounce) {
    // [d_free | coeffs | cost | per-trajectory status | status word] sit back to back in the device staging area: one D2H DMA
    double* s_p = p->stage + n_times + n_fix;
    const size_t n_out = (size_t)(n_fre + n_coef + batch + n_ts + 1);
    MTG_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_bounce, s_p, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(host_status, ctx->h_bounce + n_fre + n_coef + batch + n_ts, sizeof(int));
    if (!update_only && d_free && n_fre) std::memcpy(d_free, ctx->h_bounce, n_fre * sizeof(double));
    std::memcpy(coeffs, ctx->h_bounce + n_fre, n_coef * sizeof(double));
    if (cost) std::memcpy(cost, ctx->h_bounce + n_fre + n_coef, batch * sizeof(double));
    if (traj_status) std::memcpy(traj_status, ctx->h_bounce + n_fre + n_coef + batch, batch * sizeof(int32_t));
  } else {
    MTG_HIP_TRY(ctx, hipMemcpyAsync(coeffs, h.dco, n_coef * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!update_only && d_free && n_fre) MTG_HIP_TRY(ctx, hipMemcpyAsync(d_free, h.dfr, n_fre * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cost) MTG_HIP_TRY(ctx, hipMemcpyAsync(cost, h.dcs, batch * sizeof(double), hipMemcpyDeviceToHost, st));
    if (traj_status) MTG_HIP_TRY(ctx, hipMemcpyAsync(traj_status, h.dts, batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    // (h_status is the context's pinned word; the context lock is held, and mtg_context_sync overwrites it under the same lock)
    MTG_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status, h.status_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    MTG_HIP_TRY(ctx, hipStreamSynchronize(st));
    *host_status = *ctx->h_status;
  }
  return MTG_OK;
}

// latency path of single-trajectory host callers: the lane code's host build on the calling thread (mtg_host.cpp); no device
// work, no lock
static int solve_on_host_backend(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed,
                                 double* coeffs, double* d_free, double* cost, bool update_only, int32_t* traj_status) {
  MtgParams P;
  fill_common(p, P, batch, L);
  P.times = times; P.dfix = d_fixed; P.coeffs = coeffs; P.dfree = p->n_free ? d_free : nullptr; P.cost = cost;
  int st_word = 0;
  P.status = &st_word;
  P.tstatus = traj_status;
  P.vmask = p->mask.data(); P.offF = p->offF.data(); P.offP = p->offP.data();
  if (traj_status) std::memset(traj_status, 0, (size_t)batch * sizeof(int32_t));
  if (mtg_host_run(P, p->H, update_only) != 0) return MTG_ERR_UNSUPPORTED;
  if (!update_only && p->null_dim > 0 && p->n_free > 0) {      // structurally rank-deficient free system: every trajectory
    st_word |= MTG_FLAG_SINGULAR;
    if (traj_status) for (int64_t b = 0; b < batch; ++b) traj_status[b] |= MTG_FLAG_SINGULAR;
  }
  return mtg_status_code(nullptr, st_word);
}

int mtg_solve_impl(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed, double* coeffs,
                   double* d_free, double* cost, uint32_t flags, bool update_only, int32_t* traj_status, const PerturbedTimes* pert,
                   hipStream_t on_stream, int* own_status_dev, const double* explicit_rhs) {
  const bool cost_only = !update_only && (flags & MTG_FLAG_COST_ONLY) != 0;
  if (!p || !L || !times || (!coeffs && !cost_only) || batch < 0) return MTG_ERR_INVALID_ARGUMENT;
  if (cost_only && (!cost || (flags & MTG_FLAG_HOST_POINTERS))) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = p->ctx;
  if (!cost_only && !(flags & MTG_FLAG_HOST_POINTERS) && (reinterpret_cast<uintptr_t>(coeffs) & 15))
    return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs must be 16-byte aligned");
  if (p->n_fixed > 0 && !d_fixed) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "d_fixed is null");
  if (update_only && p->n_free > 0 && !d_free) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "d_free is null");
  if (batch == 0) return MTG_OK;
  const bool host = (flags & MTG_FLAG_HOST_POINTERS) != 0;
  if (host && (flags & MTG_FLAG_HOST_BACKEND) && batch <= MTG_HOST_BACKEND_MAX_BATCH)
    return solve_on_host_backend(p, batch, L, times, d_fixed, coeffs, d_free, cost, update_only, traj_status);
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));

  SolveCall c;
  c.p = p; c.batch = batch; c.L = L; c.flags = flags; c.cost_only = cost_only; c.pert = pert;
  c.st = on_stream ? on_stream : ctx->stream;   // on_stream: a side stream of a concurrent mixed request
  c.dts = traj_status;
  const double* dt = times; const double* dfx = d_fixed; double* dco = coeffs; double* dfr = d_free; double* dcs = cost;
  HostStaging h;
  if (host) {
    const int rc = stage_host_inputs(p, batch, L, times, d_fixed, d_free, cost != nullptr, traj_status != nullptr, update_only, c.st, h);
    if (rc != MTG_OK) return rc;
    dt = h.dt; dfx = h.dfx; dco = h.dco; dfr = h.dfr; dcs = h.dcs; c.dts = h.dts;
  }
  if (dcs) MTG_HIP_TRY(ctx, hipMemsetAsync(dcs, 0, (pert ? (size_t)(p->K + 1) : (size_t)1) * batch * sizeof(double), c.st));
  if (c.dts) MTG_HIP_TRY(ctx, hipMemsetAsync(c.dts, 0, batch * sizeof(int32_t), c.st));
  if (h.status_dev) MTG_HIP_TRY(ctx, hipMemsetAsync(h.status_dev, 0, sizeof(double), c.st));
  if (own_status_dev && !host) MTG_HIP_TRY(ctx, hipMemsetAsync(own_status_dev, 0, sizeof(double), c.st));

  fill_common(p, c.P, batch, L);
  if (h.status_dev) c.P.status = h.status_dev;
  else if (own_status_dev) c.P.status = own_status_dev;
  c.P.times = dt; c.P.dfix = dfx; c.P.coeffs = dco; c.P.dfree = (p->n_free ? dfr : nullptr); c.P.cost = dcs;
  c.P.tstatus = c.dts;
  if (explicit_rhs) { c.P.rhs = explicit_rhs; c.P.rh_b = (long long)p->D * p->n_free; c.P.rh_d = p->n_free; c.P.rh_c = 1; }
  c.wc = dcs != nullptr || (!update_only && c.P.dfree != nullptr);
  c.ntiles = (int)((batch + kWave - 1) / kWave);
  if (pert) {   // cost-only launch over (K + 1) x batch virtual problems; cost = [(K + 1)][batch]
    c.P.pert_on = 1; c.P.pert_seg = -1; c.P.pert_tpv = c.ntiles;
    c.P.pert_h = pert->h; c.P.pert_corr = pert->h / (p->K - 1.0); c.P.pert_lo = pert->lower_bound;
    c.ntiles *= p->K + 1;
  }
  p->last.clear();

  int rc = MTG_OK;
  switch (pick_form(c, update_only)) {
    case SolveForm::kUpdate: rc = launch_update(c); break;
    case SolveForm::kCoop: rc = launch_coop(c); break;
    case SolveForm::kDimlaneRt: rc = launch_dimlane_rt(c); break;
    case SolveForm::kDimlane: rc = launch_dimlane(c); break;
    case SolveForm::kFused: rc = launch_fused(c); break;
  }
  if (rc != MTG_OK) return rc;
  if (!update_only) mtg_flag_structurally_singular(p, c.st, c.P.status, c.P.tstatus, batch);
  MTG_HIP_TRY(ctx, hipGetLastError());

  if (host) {
    // A host-pointer call synchronises anyway: the status word (and the per-trajectory status) come back with the
    // results, and the call itself returns MTG_ERR_BAD_SEGMENT_TIME / MTG_ERR_SINGULAR -- no mtg_context_sync needed.
    int host_status = 0;
    rc = fetch_host_outputs(p, batch, coeffs, d_free, cost, traj_status, update_only, c.st, h, &host_status);
    if (rc != MTG_OK) return rc;
    return mtg_status_code(ctx, host_status);
  }
  return MTG_OK;
}

extern "C" {
int mtg_plan_launch_form(const mtg_plan* p, int64_t batch, const mtg_layout* L, uint32_t flags) {
  if (!p || !L || batch <= 0 || (flags & (MTG_FLAG_HOST_POINTERS | MTG_FLAG_COST_ONLY))) return MTG_ERR_INVALID_ARGUMENT;
  MtgParams P;
  fill_common(p, P, batch, L);   // (no d_free / cost output: coefficient output only ...
  const bool extra = (flags & MTG_FLAG_QUERY_EXTRA_OUTPUTS) != 0;
  static double cost_stands_for_any_extra_output = 0.0;
  if (extra) P.cost = &cost_stands_for_any_extra_output;   // ... unless asked for the form of a call with extra outputs; never dereferenced)
  flags &= ~(uint32_t)MTG_FLAG_QUERY_EXTRA_OUTPUTS;
  if (pick_coop(p, batch, L, P, flags, false)) return 7;
  if (pick_dimlane_rt(p, batch, L, P, flags, false)) return 6;
  if (pick_dimlane(p, batch, L, P, flags, false)) return 5;
  const MtgStaticEntry* var = pick_static(p, (int)((batch + kWave - 1) / kWave), flags, !extra);
  if (!var) return 0;
  if (const MtgSlabEntry* slab = pick_slab(p, var)) {
    if (!extra || (slab->extra && !p->ctx->knob_no_slab_extra)) return 4;
  }
  if (var->k < 0) return 3;
  return var->d == p->D ? 1 : 2;
}

int mtg_plan_set_workspace(mtg_plan* p, void* device_ptr, size_t bytes) {
  if (!p) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(p->ctx->mu);
  p->user_ws = bytes ? static_cast<double*>(device_ptr) : nullptr;
  p->user_ws_bytes = bytes;
  return MTG_OK;
}

// The queue as ONE persistent launch (several when n > kSeqMax), coefficient output only: the slab-output fused kernel
// (mtg_solve_slab_queue_kernel) or the dimension-in-lane kernel (mtg_solve_dl_queue_kernel; canonical SoA inputs), chosen
// by the TOTAL number of trajectories the way single launches choose by their batch.  Returns 1 when the call does not
// qualify (the caller then enqueues one launch per batch), MTG_OK or an error otherwise.
static int sequence_as_queue(mtg_plan* p, int32_t n, int64_t batch, const mtg_layout* L, const double* const* times,
                             const double* const* d_fixed, double* const* coeffs, uint32_t flags) {
  mtg_context* ctx = p->ctx;
  if (n < 2 || batch <= 0 || ctx->knob_no_queue || p->null_dim > 0) return 1;
  if (flags & (MTG_FLAG_GENERIC_KERNEL | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH)) return 1;
  const int32_t n_launch = std::min<int32_t>(n, kSeqMax);       // batches per launch
  const MtgSlabEntry* slab = nullptr;
  if (!(flags & MTG_FLAG_DIMLANE) && !ctx->knob_no_slab && p->fast && p->fast->k > 0 && p->fast->d == p->D)
    slab = mtg_find_slab(p->H, p->D, p->K, p->deriv, p->mask.data());
  if (slab && (!slab->queue || ((batch + kWave - 1) / kWave) * (int64_t)n_launch >= (1ll << 31))) slab = nullptr;
  const MtgDimlaneEntry* dl = p->dimlane;
  if (dl && (!dl->launch_queue || ctx->knob_no_dimlane || (flags & MTG_FLAG_FUSED_DIMS))) dl = nullptr;
  if (dl && (mtg_dimlane_input_kind(p, L, batch) < 0 || mtg_padded16(batch) * 8 * (int64_t)std::max(p->K, p->n_fixed * p->D) >= (1ll << 32) ||
             ((batch + dl->tpw - 1) / dl->tpw) * (int64_t)n_launch >= (1ll << 31)))
    dl = nullptr;
  if (slab && dl && !(flags & MTG_FLAG_DIMLANE) && !dimlane_is_default(p, dl, batch * (int64_t)n_launch)) dl = nullptr;
  if (!slab && !dl) return 1;
  for (int32_t i = 0; i < n; ++i) {
    if (!times[i] || !coeffs[i] || (p->n_fixed > 0 && !d_fixed[i])) return MTG_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(coeffs[i]) & 15) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs must be 16-byte aligned");
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  p->last.clear();
  const int64_t tpb = dl ? (batch + dl->tpw - 1) / dl->tpw : (batch + kWave - 1) / kWave;
  MtgParams P;
  fill_common(p, P, batch, L);
  P.times = times[0]; P.dfix = d_fixed ? d_fixed[0] : nullptr; P.coeffs = coeffs[0];
  if (!dl && !p->slab_queue_attr_set) {
    MTG_HIP_TRY(ctx, hipFuncSetAttribute((const void*)slab->queue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slab->lds));
    p->slab_queue_attr_set = true;
  }
  for (int32_t i0 = 0; i0 < n; i0 += kSeqMax) {
    MtgSeqQueue q;
    q.n = std::min<int32_t>(kSeqMax, n - i0);
    q.tiles_per_batch = (int)tpb;
    for (int i = 0; i < q.n; ++i) q.item[i] = MtgSeqItem{times[i0 + i], d_fixed ? d_fixed[i0 + i] : nullptr, coeffs[i0 + i]};
    for (int i = q.n; i < kSeqMax; ++i) q.item[i] = MtgSeqItem{nullptr, nullptr, nullptr};
    const int ntiles = q.n * (int)tpb;
    if (dl) {
      const int units = (ntiles + dl->np - 1) / dl->np;
      int grid = std::min(units, ctx->n_cu * 8);
      double* dl_ws = nullptr;
      if (dl->ws_per_lane) {   // long chains: persistent workgroups only, as in single launches
        grid = std::min(units, ctx->n_cu * 4 / (2 * dl->np));
        const int rc = workspace(p, dl->ws_per_lane * (size_t)grid * dl->np * 2 * kWave, &dl_ws);
        if (rc != MTG_OK) return rc;
      }
      if (dl->launch_queue((void*)ctx->stream, grid, &q, ctx->d_status, (int)batch, ntiles, dl_ws, mtg_dimlane_input_kind(p, L, batch)) != 0)
        return set_err(ctx, MTG_ERR_DEVICE, "dimension-in-lane queue launch set-up failed");
    } else {
      const int grid = balanced_grid(ctx, ntiles, ctx->n_cu * 2);   // two workgroups per CU, one wave per SIMD (as the single-batch launch)
      hipLaunchKernelGGL(slab->queue, dim3(grid), dim3(kBlock), slab->lds, ctx->stream, P, ntiles, q);
    }
  }
  MTG_HIP_TRY(ctx, hipGetLastError());
  return MTG_OK;
}

int mtg_solve_linear_sequence_events(mtg_plan* plan, int32_t n, int64_t batch, const mtg_layout* layout,
                                     const double* const* times, const double* const* d_fixed, double* const* coeffs,
                                     uint32_t flags, void* start_event, void* stop_event) {
  if (!plan || !layout || n < 0 || !times || !coeffs || (plan->n_fixed > 0 && !d_fixed)) return MTG_ERR_INVALID_ARGUMENT;
  if (flags & (MTG_FLAG_HOST_POINTERS | MTG_FLAG_COST_ONLY)) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = plan->ctx;
  if (flags & MTG_FLAG_BASIC_SOLUTION) {
    // A queue stays asynchronous: a structurally rank-deficient plan runs the whole queue on its shadow (the pinned, regular
    // system -- the shadow's d_fixed of every batch gathered on the device first); on a regular plan the flag changes nothing.
    flags &= ~(uint32_t)MTG_FLAG_BASIC_SOLUTION;
    if (plan->null_dim > 0 && plan->n_free > 0 && n > 0 && batch > 0) {
      if (!plan->shadow) return set_err(ctx, MTG_ERR_UNSUPPORTED, "MTG_FLAG_BASIC_SOLUTION: this rank-deficient plan has no shadow plan");
      const size_t per = mtg_shadow_fixed_elems(plan, batch);
      mtg_layout SL;
      std::vector<const double*> sfx((size_t)n);
      {
        std::lock_guard<std::mutex> lock(ctx->mu);
        MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int rs = ensure_buffer(ctx, &plan->shadow_buf, &plan->shadow_buf_bytes, per * (size_t)n * sizeof(double));
        if (rs != MTG_OK) return rs;
        for (int32_t i = 0; i < n; ++i) {
          if (!d_fixed[i]) return MTG_ERR_INVALID_ARGUMENT;
          mtg_shadow_gather_async(plan, batch, layout, d_fixed[i], plan->shadow_buf + per * (size_t)i, &SL, ctx->stream);
          sfx[(size_t)i] = plan->shadow_buf + per * (size_t)i;
        }
        MTG_HIP_TRY(ctx, hipGetLastError());
      }
      return mtg_solve_linear_sequence_events(plan->shadow, n, batch, &SL, times, sfx.data(), coeffs, flags, start_event, stop_event);
    }
  }
  if (start_event) {
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    MTG_HIP_TRY(ctx, hipEventRecord((hipEvent_t)start_event, ctx->stream));
  }
  int rc = sequence_as_queue(plan, n, batch, layout, times, d_fixed, coeffs, flags);
  if (rc == 1) {
    rc = MTG_OK;
    for (int32_t i = 0; i < n && rc == MTG_OK; ++i)
      rc = mtg_solve_impl(plan, batch, layout, times[i], d_fixed ? d_fixed[i] : nullptr, coeffs[i], nullptr, nullptr,
                      flags & ~(uint32_t)MTG_FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH, false);
  }
  if (stop_event) MTG_HIP_TRY(ctx, hipEventRecord((hipEvent_t)stop_event, ctx->stream));
  return rc;
}

int mtg_solve_linear_sequence(mtg_plan* plan, int32_t n, int64_t batch, const mtg_layout* layout,
                              const double* const* times, const double* const* d_fixed, double* const* coeffs, uint32_t flags) {
  return mtg_solve_linear_sequence_events(plan, n, batch, layout, times, d_fixed, coeffs, flags, nullptr, nullptr);
}

namespace {
// J[b] = cost of the unperturbed problem; gradient[b][n] = (cost of variant n + 1 - J[b]) / h, written with the times' strides
__global__ void mtg_mellinger_grad_kernel(const double* __restrict__ cost_all, long long B, int K, double inv_h,
                                          double* __restrict__ J, double* __restrict__ grad, long long gs_b, long long gs_k) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (cost_all == nullptr) {   // one segment: zero gradient
    for (int n = 0; n < K; ++n) grad[b * gs_b + n * gs_k] = 0.0;
    return;
  }
  const double j0 = cost_all[b];
  if (J) J[b] = j0;
  for (int n = 0; n < K; ++n) grad[b * gs_b + n * gs_k] = (cost_all[(long long)(n + 1) * B + b] - j0) * inv_h;
}
}  // namespace

int mtg_mellinger_cost_gradient(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                const double* d_fixed, double increment_time, double time_lower_bound, double* cost, double* gradient) {
  if (!plan || !layout || !times || !gradient || batch < 0 || !(increment_time > 0.0)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  mtg_context* ctx = plan->ctx;
  const int K = plan->K;
  if (K == 1) {   // polynomial_optimization_nonlinear_impl.h:295-302: one segment -> zero gradient
    int rc = MTG_OK;
    if (cost) rc = mtg_solve_impl(plan, batch, layout, times, d_fixed, nullptr, nullptr, cost, MTG_FLAG_COST_ONLY, false);
    if (rc != MTG_OK) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(mtg_mellinger_grad_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const double*)nullptr, (long long)batch, 1, 0.0, (double*)nullptr, gradient,
                       (long long)layout->times_stride_b, (long long)layout->times_stride_k);
    MTG_HIP_TRY(ctx, hipGetLastError());
    return MTG_OK;
  }
  double* all = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_buffer(ctx, &plan->pert_cost, &plan->pert_cost_bytes, (size_t)(K + 1) * batch * sizeof(double));
    if (rc != MTG_OK) return rc;
    all = plan->pert_cost;
  }
  const PerturbedTimes pt{increment_time, time_lower_bound};
  const int rc = mtg_solve_impl(plan, batch, layout, times, d_fixed, nullptr, nullptr, all, MTG_FLAG_COST_ONLY, false, nullptr, &pt);
  if (rc != MTG_OK) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  hipLaunchKernelGGL(mtg_mellinger_grad_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const double*)all, (long long)batch, K, 1.0 / increment_time, cost, gradient,
                     (long long)layout->times_stride_b, (long long)layout->times_stride_k);
  MTG_HIP_TRY(ctx, hipGetLastError());
  return MTG_OK;
}

int mtg_update_segments_from_free(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                  const double* d_fixed, const double* d_free, double* coeffs, double* cost, uint32_t flags) {
  return mtg_solve_impl(plan, batch, layout, times, d_fixed, coeffs, const_cast<double*>(d_free), cost, flags, true);
}

// used by mtg_objective.hip: the solve stage of mtg_time_objective -- the plan's ordinary launch forms (coefficients + cost; with
// d_free_in the update-from-free path) into the caller's coefficient buffer, cost and per-trajectory status into the plan's
// workspace, whose three parts are returned
int mtg_plan_objective_solve(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times, const double* d_fixed,
                             const double* d_free_in, double* coeffs, double** cost, double** slots, int32_t** tstatus) {
  if (!plan || !cost || !slots || !tstatus || batch <= 0) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = plan->ctx;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_buffer(ctx, &plan->objective_ws, &plan->objective_ws_bytes, (size_t)batch * 48);
    if (rc != MTG_OK) return rc;
  }
  *cost = plan->objective_ws;
  *slots = plan->objective_ws + batch;
  *tstatus = reinterpret_cast<int32_t*>(plan->objective_ws + 5 * batch);
  return mtg_solve_impl(plan, batch, layout, times, d_fixed, coeffs, const_cast<double*>(d_free_in), *cost, 0, d_free_in != nullptr, *tstatus);
}

int mtg_time_last_solve(mtg_plan* p, int iters, double* mean_us) {
  if (!p || !mean_us || iters < 1) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = p->ctx;
  if (p->last.empty()) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "no recorded solve launch");
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipEvent_t e0, e1;
  MTG_HIP_TRY(ctx, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return set_err(ctx, MTG_ERR_DEVICE, "hipEventCreate"); }
  struct EventGuard { hipEvent_t a, b; ~EventGuard() { hipEventDestroy(a); hipEventDestroy(b); } } guard{e0, e1};
  MTG_HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < iters; ++i) {
    for (const LaunchRecord& r : p->last) {
      if (r.coop) {
        mtg_coop_launch((void*)ctx->stream, p->H, p->D, p->K, p->deriv, r.params.B, r.params.times, r.params.ts_b, r.params.ts_k,
                        r.params.dfix, r.params.fs_b, r.params.fs_d, r.params.fs_c, r.params.coeffs, r.params.status, r.params.tstatus);
        continue;
      }
      if (r.rt) {
        r.rt->launch((void*)ctx->stream, r.grid, r.params.times, r.params.dfix, r.params.coeffs, r.params.status, r.params.tstatus,
                     (int)r.params.B, r.params.K, r.ntiles, r.dl_ws, r.dl_aos);
        continue;
      }
      if (r.dl) {
        run_dimlane(r.dl, ctx->stream, r.grid, r.params, r.ntiles, r.dl_ws, r.dl_aos);
        continue;
      }
      // (the cost accumulators are not re-zeroed between the timed launches: values are irrelevant here, and a memset
      // node per iteration would be timed as part of the kernel)
      hipLaunchKernelGGL(r.fn, dim3(r.grid, r.gridy), dim3(kBlock), r.lds, ctx->stream, r.params, r.ntiles);
    }
  }
  MTG_HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
  MTG_HIP_TRY(ctx, hipEventSynchronize(e1));
  float ms = 0.f;
  MTG_HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
  *mean_us = (double)ms * 1000.0 / iters;
  return MTG_OK;
}
}  // extern "C"
