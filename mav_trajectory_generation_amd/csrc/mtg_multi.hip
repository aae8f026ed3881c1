// mtg_multi.hip -- the C ABI of include/mtg_hip.h, part 5: mixed requests (mtg_multi_*) as few launches -- one cross-structure
// dimension-in-lane launch, merged rolled groups, singles (optionally over side streams); schedules: mtg_multi_schedule.h.
#include "mtg_abi_internal.h"
#include "mtg_multi_schedule.h"

extern "C" {
struct MtgMultiGroup {
  const MtgStaticEntry* entry = nullptr;   // rolled configuration shared by the group's items
  std::vector<int> items;
  MtgParams* d_table = nullptr;
  MtgTileRef* d_tiles = nullptr;
  double* d_ws = nullptr;
  int ntiles = 0, grid = 0, ngroups = 1;    // ngroups: dimension groups (grid.y) of the launch
  size_t lds = 0;
  bool extra = false;                       // any item wants d_free / cost
  bool any = false;                         // cross-structure launch (mtg_solve_multi_any_kernel): items of several configurations
  int dg = 0;                               // dimensions per workgroup of the launch
  bool attr_set[4] = {false, false, false, false};
  int any_units = 1;                        // cross-structure launch: dimension groups per tile (units = ntiles * any_units)
};
struct MtgDlAnyGroup {                      // cross-structure dimension-in-lane launch (mtg_solve_dl_any_kernel)
  std::vector<int> items;
  MtgDlAnyItem* d_items = nullptr;
  MtgDlAnyUnit* d_units = nullptr;
  int* d_wg_begin = nullptr;                // [grid + 1]: workgroup w runs d_units[d_wg_begin[w] .. d_wg_begin[w + 1])
  double* d_ws = nullptr;
  int nunits = 0, grid = 0;
  bool shared_schedule = false;             // d_units / d_wg_begin belong to the context's schedule cache
  size_t d_items_bytes = 0;                 // d_items comes from (and returns to) the context's free list
  std::vector<MtgDlAnyItem> h_items;        // source of the asynchronous upload
};
struct mtg_multi {
  mtg_context* ctx = nullptr;
  MtgDlAnyGroup dl_any;
  std::vector<mtg_multi_item> items;
  std::vector<MtgMultiGroup> groups;
  std::vector<int> singles;                 // items launched through the ordinary path
  bool concurrent = false;                  // MTG_FLAG_CONCURRENT_ITEMS: singles spread over the context's side streams
  std::vector<int> lane_of;                 // [singles.size()] side stream of each single (longest-processing-time first)
  int n_lanes = 0;
  // MTG_FLAG_BASIC_SOLUTION: items of structurally rank-deficient plans run on the plan's shadow; their shadow d_fixed is gathered
  // from the caller's buffer in front of every solve, their d_free (when asked for) scattered back behind it
  struct ShadowFix { const mtg_plan* plan; int64_t batch; mtg_layout layout; const double* d_fixed; double* sfx; double* d_free; double* sfr; };
  std::vector<ShadowFix> shadow_fix;
  double* shadow_mem = nullptr;
};

static void multi_free(mtg_multi* m, bool context_locked) {
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  if (m->dl_any.d_items) {
    std::unique_lock<std::mutex> lock(m->ctx->mu, std::defer_lock);
    if (!context_locked) lock.lock();
    m->ctx->dl_any_item_pool.push_back({(void*)m->dl_any.d_items, m->dl_any.d_items_bytes});
  }
  if (!m->dl_any.shared_schedule && m->dl_any.d_units) hipFree(m->dl_any.d_units);
  if (!m->dl_any.shared_schedule && m->dl_any.d_wg_begin) hipFree(m->dl_any.d_wg_begin);     // (dl_any.d_ws is the context's)
  for (MtgMultiGroup& g : m->groups) {
    if (g.d_table) hipFree(g.d_table);
    if (g.d_tiles) hipFree(g.d_tiles);
    if (g.d_ws) hipFree(g.d_ws);
  }
  if (m->shadow_mem) hipFree(m->shadow_mem);
  delete m;
}
int mtg_multi_destroy(mtg_multi* m) {
  if (m) multi_free(m, false);
  return MTG_OK;
}

static long long item_work(const mtg_multi_item& it) { return mtg_work_estimate(it.plan->K, it.plan->N); }
static bool runs_on_shadow(const mtg_multi_item& it) { return it.plan->null_dim > 0 && it.plan->n_free > 0 && it.batch != 0; }

// step 1: every item usable (the MTG_FLAG_BASIC_SOLUTION conditions first, as the items are patched before the others are looked at)
static int multi_validate(mtg_context* ctx, int32_t n_items, const mtg_multi_item* items, uint32_t flags) {
  for (int i = 0; i < n_items && (flags & MTG_FLAG_BASIC_SOLUTION); ++i) {
    const mtg_multi_item& it = items[i];
    if (!it.plan || it.plan->ctx != ctx || it.batch < 0) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "mtg_multi_create: bad item");
    if (!runs_on_shadow(it)) continue;
    if (!it.plan->shadow) return set_err(ctx, MTG_ERR_UNSUPPORTED, "MTG_FLAG_BASIC_SOLUTION: a rank-deficient plan of the request has no shadow plan");
    if (!it.d_fixed) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "mtg_multi_create: bad item");
  }
  for (int i = 0; i < n_items; ++i) {
    const mtg_multi_item& it = items[i];
    if (!it.plan || it.plan->ctx != ctx || it.batch < 0 || !it.times || !it.coeffs || (it.plan->n_fixed > 0 && !it.d_fixed))
      return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "mtg_multi_create: bad item");
    if (reinterpret_cast<uintptr_t>(it.coeffs) & 15) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs must be 16-byte aligned");
  }
  return MTG_OK;
}

// step 2 (MTG_FLAG_BASIC_SOLUTION): the request stays asynchronous -- an item of a structurally rank-deficient plan becomes an
// item of that plan's SHADOW (the pinned, regular system: just another plan of the request); regular plans' items are unchanged
static int multi_patch_shadow_items(mtg_multi* m) {
  mtg_context* ctx = m->ctx;
  size_t total = 0;
  for (const mtg_multi_item& it : m->items)
    if (runs_on_shadow(it))
      total += mtg_shadow_fixed_elems(it.plan, it.batch) + (it.d_free ? (size_t)it.batch * it.plan->D * std::max(it.plan->shadow->n_free, 1) : 0);
  if (total == 0) return MTG_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MTG_HIP_TRY(ctx, hipMalloc((void**)&m->shadow_mem, total * sizeof(double)));
  double* cur = m->shadow_mem;
  for (mtg_multi_item& it : m->items) {
    if (!runs_on_shadow(it)) continue;
    const mtg_plan* p = it.plan;
    mtg_multi::ShadowFix fx{p, it.batch, it.layout, it.d_fixed, cur, it.d_free, nullptr};
    cur += mtg_shadow_fixed_elems(p, it.batch);
    mtg_shadow_layout(p, it.batch, &fx.layout, &it.layout);     // the item's layout with the shadow buffer's fixed-value strides ...
    if (it.d_free) {     // ... and d_P through a contiguous [B][D][n_free of the shadow] buffer, scattered back after the solve
      fx.sfr = cur;
      cur += (size_t)it.batch * p->D * std::max(p->shadow->n_free, 1);
      mtg_free_contiguous(&it.layout, p->D, p->shadow->n_free);
      it.d_free = fx.sfr;
    }
    it.plan = p->shadow;
    it.d_fixed = fx.sfx;
    m->shadow_fix.push_back(fx);
  }
  return MTG_OK;
}

// step 3 (MTG_FLAG_CONCURRENT_ITEMS): one launch per item, each through the ordinary variant choice, on up to kSideStreams side
// streams (the HIP runtime maps a process's streams onto 4 hardware queues: more streams add no overlap).  The work estimate
// of mtg_lpt_lanes is chain length x N^2 x rounds of tiles.
static int multi_plan_lanes(mtg_multi* m) {
  constexpr int kSideStreams = 4;
  mtg_context* ctx = m->ctx;
  m->concurrent = true;
  std::vector<int> idx, plan_id;
  std::vector<double> est;
  for (int i = 0; i < (int)m->items.size(); ++i) {
    const mtg_multi_item& it = m->items[(size_t)i];
    if (it.batch <= 0) continue;
    int id = i;      // plan id: the request index of the plan's first item
    for (int r : idx) if (m->items[(size_t)r].plan == it.plan) { id = r; break; }
    const double rounds = std::max(1.0, (double)it.batch * it.plan->D / (64.0 * 4.0 * ctx->n_cu));
    idx.push_back(i);
    plan_id.push_back(id);
    est.push_back((double)item_work(it) * rounds);
  }
  std::vector<int> order(idx.size());
  m->lane_of.resize(idx.size());
  m->n_lanes = mtg_lpt_lanes(est.data(), plan_id.data(), (int)idx.size(), kSideStreams, order.data(), m->lane_of.data());
  for (int s : order) m->singles.push_back(idx[(size_t)s]);
  while ((int)ctx->side_streams.size() < m->n_lanes) {
    hipStream_t q = nullptr;
    hipEvent_t e = nullptr;
    if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      if (q) hipStreamDestroy(q);
      return set_err(ctx, MTG_ERR_DEVICE, "mtg_multi_create: side stream creation failed");
    }
    ctx->side_streams.push_back(q);
    ctx->join_events.push_back(e);
  }
  if (!ctx->fork_event && hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming) != hipSuccess)
    return set_err(ctx, MTG_ERR_DEVICE, "mtg_multi_create: event creation failed");
  return MTG_OK;
}

// The per-workgroup unit lists of a cross-structure launch on the device: from the context's cache (see
// mtg_context::DlAnySchedule), else computed (mtg_multi_schedule.h), uploaded and -- while there is room -- cached.
static bool dl_any_schedule_on_device(mtg_context* ctx, MtgDlAnyGroup& g, const std::vector<MtgScheduleItem>& sched) {
  constexpr size_t kMaxDlAnySchedules = 64;
  std::vector<long long> key = mtg_dl_any_schedule_key(sched.data(), (int)sched.size(), g.grid, ctx->knob_dl_any_rr);
  for (const auto& sc : ctx->dl_any_schedules)
    if (sc.key == key) {
      g.d_units = (MtgDlAnyUnit*)sc.d_units; g.d_wg_begin = sc.d_wg_begin; g.shared_schedule = true;
      return true;
    }
  std::vector<MtgDlAnyUnit> units;
  std::vector<int> wg_begin;
  mtg_dl_any_schedule(sched.data(), (int)sched.size(), g.grid, ctx->knob_dl_any_rr, units, wg_begin);
  if (hipMalloc((void**)&g.d_units, units.size() * sizeof(MtgDlAnyUnit)) != hipSuccess ||
      hipMalloc((void**)&g.d_wg_begin, wg_begin.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(g.d_wg_begin, wg_begin.data(), wg_begin.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(g.d_units, units.data(), units.size() * sizeof(MtgDlAnyUnit), hipMemcpyHostToDevice) != hipSuccess)
    return false;
  if (ctx->dl_any_schedules.size() < kMaxDlAnySchedules) {
    mtg_context::DlAnySchedule sc;
    sc.key = std::move(key); sc.grid = g.grid; sc.nunits = g.nunits; sc.d_units = g.d_units; sc.d_wg_begin = g.d_wg_begin;
    ctx->dl_any_schedules.push_back(std::move(sc));
    g.shared_schedule = true;
  }
  return true;
}

// step 4: items that can run their static dimension-in-lane configuration (canonical SoA inputs, coefficient output only) join
// ONE cross-structure launch (mtg_solve_dl_any_kernel), whatever their N and K: back-substitution data in registers instead of
// the rolled kernels' workspace traffic.  taken[i]: item i is part of it.
static int multi_plan_dl_any(mtg_multi* m, uint32_t flags, std::vector<char>& taken) {
  mtg_context* ctx = m->ctx;
  const std::vector<mtg_multi_item>& items = m->items;
  if ((flags & (MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_GENERIC_KERNEL)) || ctx->knobs.no_dimlane) return MTG_OK;
  std::vector<int> cand;
  for (int i = 0; i < (int)items.size(); ++i) {
    const mtg_multi_item& it = items[(size_t)i];
    const mtg_plan* p = it.plan;
    if (it.batch <= 0 || it.cost || (it.d_free && p->n_free > 0) || mtg_dl_any_index(p->forms.dimlane) < 0) continue;
    { const int kind = mtg_input_kind(p->forms, &it.layout, it.batch); if (kind < 0 || kind > 1) continue; }   // (padded SoA: single / queue launches only)
    // (the batch as it is, not its padded row stride: a recorded difference from the single launch's check, kept as it is)
    if (!mtg_dl_offsets_fit(p->forms, it.batch, false)) continue;
    cand.push_back(i);
  }
  if (cand.size() < 2) return MTG_OK;
  MtgDlAnyGroup& g = m->dl_any;
  std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return item_work(items[(size_t)a]) > item_work(items[(size_t)b]); });
  g.items = cand;
  g.h_items.resize(cand.size());
  std::vector<MtgScheduleItem> sched(cand.size());
  for (size_t bi = 0; bi < cand.size(); ++bi) {
    const mtg_multi_item& it = items[(size_t)cand[bi]];
    taken[(size_t)cand[bi]] = 1;
    g.h_items[bi] = MtgDlAnyItem{it.times, it.d_fixed, it.coeffs, (int)it.batch, mtg_dl_any_index(it.plan->forms.dimlane),
                                 mtg_input_kind(it.plan->forms, &it.layout, it.batch), 0};
    sched[bi] = MtgScheduleItem{it.plan->K, it.plan->H, (int)mtg_tiles(it.batch, it.plan->forms.dimlane->tpw)};
    g.nunits += sched[bi].tiles;
  }
  g.grid = std::min(g.nunits, ctx->n_cu * 2);      // two 2-wave workgroups per CU: one wave per SIMD
  bool ok = dl_any_schedule_on_device(ctx, g, sched);
  // workspace: one buffer per context, sized for the largest grid (requests of a context run in stream order)
  const size_t ws_bytes = std::max<size_t>(16, mtg_dl_any_ws_per_lane() * (size_t)(ctx->n_cu * 2) * 2 * kWave);
  if (ok && ctx->dl_any_ws_bytes < ws_bytes) {
    if (ctx->dl_any_ws) { hipStreamSynchronize(ctx->stream); hipFree(ctx->dl_any_ws); ctx->dl_any_ws = nullptr; ctx->dl_any_ws_bytes = 0; }
    ok = hipMalloc((void**)&ctx->dl_any_ws, ws_bytes) == hipSuccess;
    if (ok) ctx->dl_any_ws_bytes = ws_bytes;
  }
  g.d_ws = ctx->dl_any_ws;
  // item table: a buffer of the free list (or a new one), filled by an asynchronous copy on the context's stream -- the
  // launch that reads it is enqueued behind it
  const size_t ib = g.h_items.size() * sizeof(MtgDlAnyItem);
  if (ok) {
    for (size_t k2 = 0; k2 < ctx->dl_any_item_pool.size(); ++k2)
      if (ctx->dl_any_item_pool[k2].second >= ib) {
        g.d_items = (MtgDlAnyItem*)ctx->dl_any_item_pool[k2].first;
        g.d_items_bytes = ctx->dl_any_item_pool[k2].second;
        ctx->dl_any_item_pool.erase(ctx->dl_any_item_pool.begin() + (long)k2);
        break;
      }
    if (!g.d_items) {
      g.d_items_bytes = std::max<size_t>(ib, 4096);
      ok = hipMalloc((void**)&g.d_items, g.d_items_bytes) == hipSuccess;
    }
  }
  if (ok) ok = hipMemcpyAsync(g.d_items, g.h_items.data(), ib, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
  return ok ? MTG_OK : set_err(ctx, MTG_ERR_DEVICE, "mtg_multi_create: device allocation failed");
}

// step 5: the other items grouped by rolled configuration, groups merged across structures, groups of one dissolved
static void multi_group_rolled(mtg_multi* m, const std::vector<char>& taken) {
  const std::vector<mtg_multi_item>& items = m->items;
  for (int i = 0; i < (int)items.size(); ++i) {
    if (taken[(size_t)i]) continue;
    mtg_plan* p = items[(size_t)i].plan;
    const MtgStaticEntry* e = (items[(size_t)i].batch > 0 && p->K >= 2) ? p->forms.rolled : nullptr;
    if (!e || !e->multi[0]) {
      if (items[(size_t)i].batch > 0) m->singles.push_back(i);
      continue;
    }
    MtgMultiGroup* g = nullptr;
    for (MtgMultiGroup& c : m->groups) if (c.entry == e) g = &c;
    if (!g) {
      m->groups.emplace_back();
      g = &m->groups.back();
      g->entry = e;
    }
    g->items.push_back(i);
  }
  // Cross-structure merge: groups whose (3-dimensional) rolled configurations are all covered by mtg_solve_multi_any_kernel
  // become ONE launch (config 4: N = 8, 10 and 12 buckets together) -- streams would not overlap them (see the kernel).
  std::vector<size_t> anyable;
  for (size_t gi = 0; gi < m->groups.size(); ++gi)
    if (m->groups[gi].entry->d == 3 && mtg_any_cfg_index(m->groups[gi].entry) >= 0) anyable.push_back(gi);
  if (anyable.size() >= 2) {
    MtgMultiGroup merged;
    merged.any = true;
    merged.entry = m->groups[anyable[0]].entry;
    for (size_t gi : anyable) merged.items.insert(merged.items.end(), m->groups[gi].items.begin(), m->groups[gi].items.end());
    for (size_t r = anyable.size(); r-- > 0;) m->groups.erase(m->groups.begin() + anyable[r]);
    m->groups.push_back(merged);
  }
  // a group of one gains nothing from the merged form: leave it to the ordinary path (static variants, heuristics)
  for (size_t gi = 0; gi < m->groups.size();) {
    if (m->groups[gi].items.size() >= 2) { ++gi; continue; }
    m->singles.push_back(m->groups[gi].items[0]);
    m->groups.erase(m->groups.begin() + gi);
  }
}

// step 6, per rolled group: fused or dimension-split form, tile list, LDS and workspace sizes, tables on the device
static int multi_upload_group(mtg_multi* m, MtgMultiGroup& g, uint32_t flags, long long total_tiles) {
  mtg_context* ctx = m->ctx;
  const std::vector<mtg_multi_item>& items = m->items;
  const int D = g.entry->d;
  // tiles, longest chain first (work per tile ~ K N^2)
  std::vector<int> order(g.items.begin(), g.items.end());
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return item_work(items[(size_t)a]) > item_work(items[(size_t)b]); });
  // few tiles: the one-dimension-per-workgroup form of the same configurations (D x the workgroups, lighter waves)
  // while all of them are resident at once -- the rule of single-plan launches (flags override)
  const bool want_split = D > 1 && ((flags & MTG_FLAG_SPLIT_DIMS) || (!(flags & MTG_FLAG_FUSED_DIMS) && mtg_all_resident(total_tiles, D, ctx->n_cu)));
  std::vector<const MtgStaticEntry*> ent(order.size());
  bool split_ok = want_split;
  for (size_t bi = 0; bi < order.size(); ++bi) {
    const mtg_plan* p = items[order[bi]].plan;
    ent[bi] = p->forms.rolled;
    const MtgStaticEntry* es = want_split ? mtg_find_static(p->H, 1, p->K, p->deriv, p->mask.data(), true) : nullptr;
    if (!es || !es->multi[0] || (g.any && mtg_any_cfg_index(es) < 0)) split_ok = false;
  }
  int Dw = D;
  if (split_ok) {
    for (size_t bi = 0; bi < order.size(); ++bi) {
      const mtg_plan* p = items[order[bi]].plan;
      ent[bi] = mtg_find_static(p->H, 1, p->K, p->deriv, p->mask.data(), true);
    }
    g.entry = ent[0];
    g.ngroups = D;
    Dw = 1;
  }
  g.dg = Dw;
  std::vector<MtgTileRef> tiles;
  std::vector<MtgParams> table(order.size());
  int kc_max = 1;
  size_t E = 0;
  g.lds = 0;
  for (size_t bi = 0; bi < order.size(); ++bi) {
    const mtg_multi_item& it = items[order[bi]];
    const int H = it.plan->H;
    const int nt = (int)mtg_tiles(it.batch, kWave);
    const int cfg = g.any ? mtg_any_cfg_index(ent[bi]) : 0;
    for (int t = 0; t < nt; ++t) tiles.push_back(MtgTileRef{(int)bi, t, cfg});
    kc_max = std::max(kc_max, (it.plan->K + 1) / 2);
    g.extra = g.extra || it.cost != nullptr || (it.d_free != nullptr && it.plan->n_free > 0);
    E = std::max(E, (size_t)H * H + (size_t)Dw * H);
    const int fm = H - __builtin_popcount((unsigned)ent[bi]->mi);
    g.lds = std::max(g.lds, mtg_solve_lds_bytes(Dw, 2 * H, fm));
  }
  g.ntiles = (int)tiles.size();
  g.grid = std::min(g.ntiles, std::max(1, ctx->n_cu * 4 / g.ngroups));
  if (g.any) {   // one-dimensional grid over (tile, dimension group) units: as many workgroups as are resident at once
    g.grid = std::min(g.ntiles * g.ngroups, ctx->n_cu * 2);
    g.any_units = g.ngroups;
    g.ngroups = 1;
  }
  const size_t ws_bytes = (size_t)kc_max * E * (size_t)g.grid * g.ngroups * kBlock * sizeof(double);
  if (hipMalloc((void**)&g.d_ws, ws_bytes) != hipSuccess ||
      hipMalloc((void**)&g.d_table, table.size() * sizeof(MtgParams)) != hipSuccess ||
      hipMalloc((void**)&g.d_tiles, tiles.size() * sizeof(MtgTileRef)) != hipSuccess)
    return set_err(ctx, MTG_ERR_DEVICE, "mtg_multi_create: device allocation failed");
  for (size_t bi = 0; bi < order.size(); ++bi) {
    const mtg_multi_item& it = items[order[bi]];
    MtgParams& P = table[bi];
    fill_common(it.plan, P, it.batch, &it.layout);
    P.times = it.times; P.dfix = it.d_fixed; P.coeffs = it.coeffs;
    P.dfree = it.plan->n_free ? it.d_free : nullptr;
    P.cost = it.cost;
    P.ws = g.d_ws;
    P.ws_stride = (long long)g.grid * g.ngroups * kBlock;
  }
  if (hipMemcpy(g.d_table, table.data(), table.size() * sizeof(MtgParams), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(g.d_tiles, tiles.data(), tiles.size() * sizeof(MtgTileRef), hipMemcpyHostToDevice) != hipSuccess)
    return set_err(ctx, MTG_ERR_DEVICE, "mtg_multi_create: table upload failed");
  return MTG_OK;
}

int mtg_multi_create(mtg_context* ctx, int32_t n_items, const mtg_multi_item* items, uint32_t flags, mtg_multi** out) {
  if (!ctx || !items || !out || n_items < 1) return MTG_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int rc = multi_validate(ctx, n_items, items, flags);
  if (rc != MTG_OK) return rc;
  mtg_multi* m = new (std::nothrow) mtg_multi();
  if (!m) return MTG_ERR_DEVICE;
  m->ctx = ctx;
  m->items.assign(items, items + n_items);
  if (flags & MTG_FLAG_BASIC_SOLUTION) rc = multi_patch_shadow_items(m);     // (its own lock scope)
  std::unique_lock<std::mutex> lock(ctx->mu, std::defer_lock);
  if (rc == MTG_OK) {
    lock.lock();
    if (hipSetDevice(ctx->device) != hipSuccess) rc = set_err(ctx, MTG_ERR_DEVICE, "hipSetDevice failed");
  }
  if (rc == MTG_OK && (flags & MTG_FLAG_CONCURRENT_ITEMS)) {
    rc = multi_plan_lanes(m);
  } else if (rc == MTG_OK) {
    std::vector<char> taken((size_t)n_items, 0);
    rc = multi_plan_dl_any(m, flags, taken);
    if (rc == MTG_OK) multi_group_rolled(m, taken);
    long long total_tiles = 0;
    for (const MtgMultiGroup& g : m->groups)
      for (int i : g.items) total_tiles += mtg_tiles(m->items[(size_t)i].batch, kWave);
    for (size_t gi = 0; gi < m->groups.size() && rc == MTG_OK; ++gi) rc = multi_upload_group(m, m->groups[gi], flags, total_tiles);
  }
  if (rc != MTG_OK) {      // the one cleanup path: everything allocated so far belongs to m
    multi_free(m, lock.owns_lock());
    return rc;
  }
  *out = m;
  return MTG_OK;
}

int mtg_multi_launch_count(const mtg_multi* m) {
  return m ? (int)(m->groups.size() + m->singles.size() + (m->dl_any.nunits > 0 ? 1 : 0)) : 0;
}

static int multi_solve_body(mtg_multi* m) {
  mtg_context* ctx = m->ctx;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (m->dl_any.nunits > 0) {
      const MtgDlAnyGroup& g = m->dl_any;
      if (mtg_dl_any_launch((void*)ctx->stream, g.grid, g.d_items, g.d_units, g.d_wg_begin, ctx->d_status, g.d_ws) != 0)
        return set_err(ctx, MTG_ERR_DEVICE, "cross-structure dimension-in-lane launch set-up failed");
    }
    for (MtgMultiGroup& g : m->groups) {
      for (int i : g.items) {
        const mtg_multi_item& it = m->items[i];
        if (it.cost) MTG_HIP_TRY(ctx, hipMemsetAsync(it.cost, 0, it.batch * sizeof(double), ctx->stream));
      }
      // few tiles: write-through stores (no serial end-of-kernel L2 write-back), as for single-plan launches
      const bool write_through = mtg_all_resident(g.ntiles, g.ngroups * g.any_units, ctx->n_cu);
      const int variant = (g.extra ? 1 : 0) + (write_through ? 2 : 0);
      SolveMultiFn fn = g.any ? mtg_multi_any_fn(g.dg, variant) : g.entry->multi[variant];
      if (g.any && g.lds > 64 * 1024 && !g.attr_set[variant]) {
        MTG_HIP_TRY(ctx, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
        g.attr_set[variant] = true;
      }
      hipLaunchKernelGGL(fn, dim3(g.grid, g.ngroups), dim3(kBlock), g.lds, ctx->stream, (const MtgParams*)g.d_table,
                         (const MtgTileRef*)g.d_tiles, g.ntiles);
      for (int i : g.items)   // (merged groups are compile-time-mask shapes with fully fixed ends: never rank-deficient; kept for symmetry)
        mtg_flag_structurally_singular(m->items[i].plan, ctx->stream, ctx->d_status, nullptr, m->items[i].batch);
    }
    MTG_HIP_TRY(ctx, hipGetLastError());
  }
  if (m->concurrent) {
    // fork: the side streams start behind the work already queued on the context's stream
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    MTG_HIP_TRY(ctx, hipEventRecord(ctx->fork_event, ctx->stream));
    for (int l = 0; l < m->n_lanes; ++l) MTG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->side_streams[l], ctx->fork_event, 0));
    int rc_all = MTG_OK;
    for (size_t s = 0; s < m->singles.size() && rc_all == MTG_OK; ++s) {
      const mtg_multi_item& it = m->items[m->singles[s]];
      rc_all = mtg_solve_impl(it.plan, it.batch, &it.layout, it.times, it.d_fixed, it.coeffs, it.d_free, it.cost, 0, false,
                          nullptr, nullptr, ctx->side_streams[m->lane_of[s]]);
    }
    // join (also after a failed enqueue: the context's stream must not run ahead of what was launched)
    for (int l = 0; l < m->n_lanes; ++l) {
      MTG_HIP_TRY(ctx, hipEventRecord(ctx->join_events[l], ctx->side_streams[l]));
      MTG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->join_events[l], 0));
    }
    return rc_all;
  }
  for (int i : m->singles) {
    const mtg_multi_item& it = m->items[i];
    const int rc = mtg_solve_impl(it.plan, it.batch, &it.layout, it.times, it.d_fixed, it.coeffs, it.d_free, it.cost, 0, false);
    if (rc != MTG_OK) return rc;
  }
  return MTG_OK;
}

int mtg_multi_solve(mtg_multi* m) {
  if (!m) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = m->ctx;
  if (!m->shadow_fix.empty()) {      // MTG_FLAG_BASIC_SOLUTION items: the shadows' d_fixed from the callers' current values
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    mtg_layout unused;
    for (const mtg_multi::ShadowFix& fx : m->shadow_fix) mtg_shadow_gather_async(fx.plan, fx.batch, &fx.layout, fx.d_fixed, fx.sfx, &unused, ctx->stream);
    MTG_HIP_TRY(ctx, hipGetLastError());
  }
  const int rc = multi_solve_body(m);
  if (rc != MTG_OK) return rc;
  if (!m->shadow_fix.empty()) {      // ... and their d_P back into the callers' layout, exact zeros at the pinned slots
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (const mtg_multi::ShadowFix& fx : m->shadow_fix)
      if (fx.d_free) mtg_launch_pin_scatter(fx.plan, fx.batch, &fx.layout, fx.sfr, fx.d_free, ctx->stream);
    MTG_HIP_TRY(ctx, hipGetLastError());
  }
  return MTG_OK;
}
}  // extern "C"
