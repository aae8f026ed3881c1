// mtg_dispatch.hip -- the C ABI of include/mtg_hip.h, part 3: the one launcher of what mtg_launch_plan.h decides (solve, report and
// replay share it), host-pointer staging and the one solve / update call behind every entry (mtg_solve_impl); sequence, Mellinger,
// update and objective-solve entries.
#include "mtg_abi_internal.h"

static int64_t span(int64_t batch, int64_t sb, int64_t n1, int64_t s1, int64_t n2, int64_t s2) {
  return (batch - 1) * sb + (n1 - 1) * s1 + (n2 - 1) * s2 + 1;
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

// The launch call of one decided launch with its parameters (P.ws: the workspace, whatever the form): the solve's launches and their
// replay by mtg_time_last_solve.  0, or what the form's own launch function returned.
static int enqueue(const mtg_plan* p, const MtgLaunch& l, const MtgParams& P, hipStream_t st) {
  if (l.coop)
    return mtg_coop_launch((void*)st, p->H, p->D, p->K, p->deriv, P.B, P.times, P.ts_b, P.ts_k, P.dfix, P.fs_b, P.fs_d, P.fs_c, P.coeffs,
                           P.status, P.tstatus);
  if (l.rt) return l.rt->launch((void*)st, l.grid, P.times, P.dfix, P.coeffs, P.status, P.tstatus, (int)P.B, P.K, l.ntiles, P.ws, l.input_kind);
  if (l.dl && !P.dfree && !P.cost)
    return l.dl->launch((void*)st, l.grid, P.times, P.dfix, P.coeffs, P.status, P.tstatus, (int)P.B, l.ntiles, P.ws, l.input_kind);
  if (l.dl)
    return l.dl->launch_extra((void*)st, l.grid, P.times, P.dfix, P.coeffs, P.status, P.tstatus, (int)P.B, l.ntiles, P.ws, l.input_kind, P.dfree,
                              P.cost, P.ps_b, P.ps_d, P.ps_c);
  hipLaunchKernelGGL(l.fn, dim3(l.grid, l.gridy), dim3(l.block), l.lds, st, P, l.ntiles);
  return 0;
}

// The one launcher: every launch of the decision gets its workspace (sized per launch) and, once per plan and kernel, its LDS
// attribute, is enqueued and recorded for mtg_time_last_solve.
static int launch(mtg_plan* p, const MtgLaunchPlan& lp, const MtgParams& P, hipStream_t st) {
  mtg_context* ctx = p->ctx;
  for (int i = 0; i < lp.n; ++i) {
    LaunchRecord r{lp.at(i), P};
    const MtgLaunch& l = r.launch;
    if (!l.fn && !l.dl && !l.rt && !l.coop) return set_err(ctx, MTG_ERR_UNSUPPORTED, lp.error);   // (the groups before it have run)
    r.params.dim0 = l.dim0;
    if (l.user_ws_param) r.params.ws = p->user_ws;
    if (l.ws_bytes) {
      const int rc = workspace(p, l.ws_bytes, &r.params.ws);
      if (rc != MTG_OK) return rc;
      r.params.ws_stride = l.ws_stride;
    }
    if (l.attr != MtgLdsAttr::kNone && !p->lds_attr_set[(int)l.attr]) {
      MTG_HIP_TRY(ctx, hipFuncSetAttribute((const void*)l.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
      p->lds_attr_set[(int)l.attr] = true;
    }
    const int rc = enqueue(p, l, r.params, st);
    if (rc != 0)
      return set_err(ctx, l.coop && rc == 1 ? MTG_ERR_UNSUPPORTED : MTG_ERR_DEVICE,
                     l.coop ? "row-cooperative launch failed" : l.rt ? "run-time-K dimension-in-lane launch set-up failed"
                                                                     : "dimension-in-lane launch set-up failed");
    if (lp.form != MtgForm::kUpdate) p->last.push_back(r);   // (mtg_time_last_solve times solves)
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

  hipStream_t st = on_stream ? on_stream : ctx->stream;   // on_stream: a side stream of a concurrent mixed request
  int32_t* dts = traj_status;                             // per-trajectory status on the device (or null)
  const double* dt = times; const double* dfx = d_fixed; double* dco = coeffs; double* dfr = d_free; double* dcs = cost;
  HostStaging h;
  if (host) {
    const int rc = stage_host_inputs(p, batch, L, times, d_fixed, d_free, cost != nullptr, traj_status != nullptr, update_only, st, h);
    if (rc != MTG_OK) return rc;
    dt = h.dt; dfx = h.dfx; dco = h.dco; dfr = h.dfr; dcs = h.dcs; dts = h.dts;
  }
  if (dcs) MTG_HIP_TRY(ctx, hipMemsetAsync(dcs, 0, (pert ? (size_t)(p->K + 1) : (size_t)1) * batch * sizeof(double), st));
  if (dts) MTG_HIP_TRY(ctx, hipMemsetAsync(dts, 0, batch * sizeof(int32_t), st));
  if (h.status_dev) MTG_HIP_TRY(ctx, hipMemsetAsync(h.status_dev, 0, sizeof(double), st));
  if (own_status_dev && !host) MTG_HIP_TRY(ctx, hipMemsetAsync(own_status_dev, 0, sizeof(double), st));

  MtgParams P;                      // device pointers, strides, tables
  fill_common(p, P, batch, L);
  if (h.status_dev) P.status = h.status_dev;
  else if (own_status_dev) P.status = own_status_dev;
  P.times = dt; P.dfix = dfx; P.coeffs = dco; P.dfree = (p->n_free ? dfr : nullptr); P.cost = dcs;
  P.tstatus = dts;
  if (explicit_rhs) { P.rhs = explicit_rhs; P.rh_b = (long long)p->D * p->n_free; P.rh_d = p->n_free; P.rh_c = 1; }
  if (pert) {   // cost-only launch over (K + 1) x batch virtual problems; cost = [(K + 1)][batch]
    P.pert_on = 1; P.pert_seg = -1; P.pert_tpv = (int)mtg_tiles(batch, kWave);
    P.pert_h = pert->h; P.pert_corr = pert->h / (p->K - 1.0); P.pert_lo = pert->lower_bound;
  }
  MtgCall call;
  call.batch = batch; call.L = L; call.flags = flags; call.update = update_only; call.cost_only = cost_only; call.pert = pert != nullptr;
  call.extra = dcs != nullptr || (!update_only && P.dfree != nullptr);   // extra outputs (cost and / or d_P) requested
  p->last.clear();

  int rc = launch(p, mtg_launch_plan(p->forms, ctx->knobs, ctx->n_cu, call), P, st);
  if (rc != MTG_OK) return rc;
  if (!update_only) mtg_flag_structurally_singular(p, st, P.status, P.tstatus, batch);
  MTG_HIP_TRY(ctx, hipGetLastError());

  if (host) {
    // A host-pointer call synchronises anyway: the status word (and the per-trajectory status) come back with the
    // results, and the call itself returns MTG_ERR_BAD_SEGMENT_TIME / MTG_ERR_SINGULAR -- no mtg_context_sync needed.
    int host_status = 0;
    rc = fetch_host_outputs(p, batch, coeffs, d_free, cost, traj_status, update_only, st, h, &host_status);
    if (rc != MTG_OK) return rc;
    return mtg_status_code(ctx, host_status);
  }
  return MTG_OK;
}

extern "C" {
int mtg_plan_launch_form(const mtg_plan* p, int64_t batch, const mtg_layout* L, uint32_t flags) {
  if (!p || !L || batch <= 0 || (flags & (MTG_FLAG_HOST_POINTERS | MTG_FLAG_COST_ONLY))) return MTG_ERR_INVALID_ARGUMENT;
  MtgCall call;     // coefficient output only, unless asked for the form of a call with extra outputs
  call.batch = batch; call.L = L; call.flags = flags & ~(uint32_t)MTG_FLAG_QUERY_EXTRA_OUTPUTS;
  call.extra = (flags & MTG_FLAG_QUERY_EXTRA_OUTPUTS) != 0;
  return (int)mtg_launch_plan(p->forms, p->ctx->knobs, p->ctx->n_cu, call).form;   // the launcher's own decision
}

int mtg_plan_set_workspace(mtg_plan* p, void* device_ptr, size_t bytes) {
  if (!p) return MTG_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(p->ctx->mu);
  p->user_ws = bytes ? static_cast<double*>(device_ptr) : nullptr;
  p->user_ws_bytes = bytes;
  return MTG_OK;
}

// The queue as persistent launches of up to kSeqMax batches (mtg_queue_plan: slab-output fused kernel or dimension-in-lane
// kernel).  Returns 1 when the call does not qualify (the caller then enqueues one launch per batch), MTG_OK or an error otherwise.
static int sequence_as_queue(mtg_plan* p, int32_t n, int64_t batch, const mtg_layout* L, const double* const* times,
                             const double* const* d_fixed, double* const* coeffs, uint32_t flags) {
  mtg_context* ctx = p->ctx;
  if (p->null_dim > 0) return 1;
  const MtgQueuePlan qp = mtg_queue_plan(p->forms, ctx->knobs, ctx->n_cu, n, batch, L, flags);
  if (!qp.slab && !qp.dl) return 1;
  for (int32_t i = 0; i < n; ++i) {
    if (!times[i] || !coeffs[i] || (p->n_fixed > 0 && !d_fixed[i])) return MTG_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(coeffs[i]) & 15) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "coeffs must be 16-byte aligned");
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  p->last.clear();
  MtgParams P;
  fill_common(p, P, batch, L);
  P.times = times[0]; P.dfix = d_fixed ? d_fixed[0] : nullptr; P.coeffs = coeffs[0];
  if (!qp.dl && !p->lds_attr_set[(int)MtgLdsAttr::kSlabQueue]) {
    MTG_HIP_TRY(ctx, hipFuncSetAttribute((const void*)qp.slab->queue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)qp.slab->lds));
    p->lds_attr_set[(int)MtgLdsAttr::kSlabQueue] = true;
  }
  for (int32_t i0 = 0; i0 < n; i0 += kSeqMax) {
    MtgSeqQueue q;
    q.n = std::min<int32_t>(kSeqMax, n - i0);
    q.tiles_per_batch = qp.tiles_per_batch;
    for (int i = 0; i < q.n; ++i) q.item[i] = MtgSeqItem{times[i0 + i], d_fixed ? d_fixed[i0 + i] : nullptr, coeffs[i0 + i]};
    for (int i = q.n; i < kSeqMax; ++i) q.item[i] = MtgSeqItem{nullptr, nullptr, nullptr};
    const MtgLaunch l = mtg_queue_launch(qp, ctx->knobs, ctx->n_cu, q.n);
    if (qp.dl) {
      double* dl_ws = nullptr;
      if (l.ws_bytes) {   // long chains: persistent workgroups only, as in single launches
        const int rc = workspace(p, l.ws_bytes, &dl_ws);
        if (rc != MTG_OK) return rc;
      }
      if (qp.dl->launch_queue((void*)ctx->stream, l.grid, &q, ctx->d_status, (int)batch, l.ntiles, dl_ws, l.input_kind) != 0)
        return set_err(ctx, MTG_ERR_DEVICE, "dimension-in-lane queue launch set-up failed");
    } else {
      hipLaunchKernelGGL(qp.slab->queue, dim3(l.grid), dim3(kBlock), l.lds, ctx->stream, P, l.ntiles, q);
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
    // (the cost accumulators are not re-zeroed between the timed launches: values are irrelevant here, and a memset
    // node per iteration would be timed as part of the kernel)
    for (const LaunchRecord& r : p->last) enqueue(p, r.launch, r.params, ctx->stream);
  }
  MTG_HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
  MTG_HIP_TRY(ctx, hipEventSynchronize(e1));
  float ms = 0.f;
  MTG_HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
  *mean_us = (double)ms * 1000.0 / iters;
  return MTG_OK;
}
}  // extern "C"
