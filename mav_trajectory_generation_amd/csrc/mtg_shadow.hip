// mtg_shadow.hip -- the C ABI of include/mtg_hip.h, part 4: the structural-singularity flag, the shadow plan's gather / scatter
// kernels (each here and nowhere else), MTG_FLAG_BASIC_SOLUTION, MTG_FLAG_REFINE and mtg_solve_linear*, which choose among them.
#include "mtg_abi_internal.h"

extern "C" { namespace {      // (C names: what profiles and traces show for these kernels)
// Plans whose free system is structurally rank-deficient: every trajectory of a solve is flagged (context word and, when the
// caller asked for it, the per-trajectory status), whatever the sweep's pivots looked like.
__global__ void mtg_flag_all_kernel(int* status, int* tstatus, long long B, int flag) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0 && status) atomicOr(status, flag);
  if (tstatus && b < B) atomicOr(tstatus + b, flag);
}
// shadow d_fixed [B][D][nfs] from the caller's (any strides): column j <- source column src[j], or 0 for a pinned slot
__global__ void mtg_pin_gather_kernel(const double* __restrict__ src, long long fs_b, long long fs_d, long long fs_c, const int* __restrict__ map,
                                      double* __restrict__ dst, long long B, int D, int nfs) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D * nfs) return;
  const int j = (int)(i % nfs);
  const int dm = (int)((i / nfs) % D);
  const long long b = i / ((long long)nfs * D);
  const int c = map[j];
  dst[i] = c >= 0 ? src[b * fs_b + dm * fs_d + c * fs_c] : 0.0;
}
// the same into a canonical SoA destination [D][nfs][Bs] (b fastest; Bs: the row stride) -- the asynchronous shadow solves of the
// queue / merged entries keep the caller's layout KIND so that the shadow takes the same launch forms
__global__ void mtg_pin_gather_soa_kernel(const double* __restrict__ src, long long fs_b, long long fs_d, long long fs_c, const int* __restrict__ map,
                                          double* __restrict__ dst, long long B, long long Bs, int D, int nfs) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D * nfs) return;
  const long long b = i % B;
  const int j = (int)((i / B) % nfs);
  const int dm = (int)(i / (B * nfs));
  const int c = map[j];
  dst[((long long)dm * nfs + j) * Bs + b] = c >= 0 ? src[b * fs_b + dm * fs_d + c * fs_c] : 0.0;
}
// the caller's d_free (any strides) from the shadow's [B][D][nps]: free column j <- shadow column map[j], or 0 for a pinned slot
__global__ void mtg_pin_scatter_kernel(const double* __restrict__ src, const int* __restrict__ map, double* __restrict__ dst, long long ps_b,
                                       long long ps_d, long long ps_c, long long B, int D, int np, int nps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D * np) return;
  const int j = (int)(i % np);
  const int dm = (int)((i / np) % D);
  const long long b = i / ((long long)np * D);
  const int c = map[j];
  dst[b * ps_b + dm * ps_d + j * ps_c] = c >= 0 ? src[(b * D + dm) * (long long)nps + c] : 0.0;
}
} }  // namespace, extern "C"
void mtg_flag_structurally_singular(const mtg_plan* p, hipStream_t st, int* status, int* tstatus, int64_t batch) {
  if (p->null_dim <= 0 || p->n_free == 0) return;
  const int64_t n = tstatus ? batch : 1;
  hipLaunchKernelGGL(mtg_flag_all_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, status, tstatus, (long long)batch, (int)MTG_FLAG_SINGULAR);
}

// the shadow's d_fixed [batch][D][n_fixed of the shadow] from the caller's (layout L), zeros at the pinned slots
static void launch_pin_gather(const mtg_plan* p, int64_t batch, const mtg_layout* L, const double* d_fixed, double* dst, hipStream_t st) {
  const int nfs = p->shadow->n_fixed;
  const long long n = (long long)batch * p->D * nfs;
  if (n > 0)
    hipLaunchKernelGGL(mtg_pin_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_fixed, (long long)L->fixed_stride_b,
                       (long long)L->fixed_stride_d, (long long)L->fixed_stride_c, (const int*)p->d_shadow_maps, dst, (long long)batch, p->D, nfs);
}
// the caller's d_free (layout L) from the shadow's contiguous [batch][D][n_free of the shadow], exact zeros at the pinned slots
void mtg_launch_pin_scatter(const mtg_plan* p, int64_t batch, const mtg_layout* L, const double* sfr, double* d_free, hipStream_t st) {
  const long long n = (long long)batch * p->D * p->n_free;
  if (n > 0)
    hipLaunchKernelGGL(mtg_pin_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, sfr, (const int*)(p->d_shadow_maps + p->shadow->n_fixed),
                       d_free, (long long)L->free_stride_b, (long long)L->free_stride_d, (long long)L->free_stride_c, (long long)batch, p->D, p->n_free,
                       p->shadow->n_free);
}

// MTG_FLAG_BASIC_SOLUTION in the asynchronous batched entries (mtg_solve_linear_sequence*, mtg_multi_*): a structurally
// rank-deficient plan is replaced by its SHADOW (a regular plan like any other); what the shadow needs that the caller does not
// hold is its d_fixed -- the caller's columns plus zeros at the pinned slots -- gathered on the device into `dst` in the caller's
// layout KIND (SoA stays SoA: same launch forms).  SL: the caller's layout with the fixed-value strides of that buffer.
// Nothing synchronises: the per-trajectory host fall-back of the synchronous entries (a trajectory on which the shadow's own
// factorisation breaks down) does not exist here -- such a trajectory stays flagged in the context's status word.
size_t mtg_shadow_fixed_elems(const mtg_plan* p, int64_t batch) { return (size_t)mtg_padded16(batch) * p->D * std::max(p->shadow->n_fixed, 1); }
// THE layout rule of that buffer; true: canonical / padded SoA inputs (the caller's row stride: batch, or its padded value)
bool mtg_shadow_layout(const mtg_plan* p, int64_t batch, const mtg_layout* L, mtg_layout* SL) {
  const int nfs = p->shadow->n_fixed;
  const int64_t Bs = L->times_stride_k;
  const bool soa = L->fixed_stride_b == 1 && L->times_stride_b == 1 && Bs >= batch && Bs <= mtg_padded16(batch);
  *SL = *L;
  if (soa) { SL->fixed_stride_b = 1; SL->fixed_stride_c = Bs; SL->fixed_stride_d = (int64_t)nfs * Bs; }
  else mtg_fixed_contiguous(SL, p->D, nfs);
  return soa;
}
void mtg_shadow_gather_async(const mtg_plan* p, int64_t batch, const mtg_layout* L, const double* d_fixed, double* dst, mtg_layout* SL, hipStream_t st) {
  const int Dd = p->D, nfs = p->shadow->n_fixed;
  const long long n = (long long)batch * Dd * nfs, Bs = L->times_stride_k;
  if (!mtg_shadow_layout(p, batch, L, SL)) return launch_pin_gather(p, batch, L, d_fixed, dst, st);
  if (n > 0)
    hipLaunchKernelGGL(mtg_pin_gather_soa_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_fixed, (long long)L->fixed_stride_b,
                       (long long)L->fixed_stride_d, (long long)L->fixed_stride_c, (const int*)p->d_shadow_maps, dst, (long long)batch, Bs, Dd, nfs);
}

// MTG_FLAG_BASIC_SOLUTION: the ordinary solve, then -- synchronously -- the trajectories the LDL^T sweep flagged singular are
// solved again on the host (mtg_basic.cpp: column-pivoted QR of the dense R_PP, LIN:365-378), their coefficients recovered
// with the host build of the update path (LIN:263-283), and their rows of the outputs replaced.
static int solve_with_basic_solution(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed,
                                     double* coeffs, double* d_free, double* cost, int32_t* traj_status, uint32_t flags) {
  if (!p || !L) return MTG_ERR_INVALID_ARGUMENT;
  if (flags & MTG_FLAG_COST_ONLY) return set_err(p->ctx, MTG_ERR_INVALID_ARGUMENT, "MTG_FLAG_BASIC_SOLUTION needs coefficient output");
  mtg_context* ctx = p->ctx;
  const bool host = (flags & MTG_FLAG_HOST_POINTERS) != 0;
  const uint32_t inner = flags & ~(uint32_t)MTG_FLAG_BASIC_SOLUTION;
  if (batch <= 0) return mtg_solve_impl(p, batch, L, times, d_fixed, coeffs, d_free, cost, inner, false, traj_status);
  std::vector<int32_t> ts((size_t)batch, 0);
  int32_t* dev_ts = nullptr;           // device-pointer calls: the per-trajectory status the kernels write
  int rc;
  // A structurally rank-deficient plan is solved through its SHADOW (the same problem with null_dim more slots fixed to zero:
  // a regular system, the LDL^T kernels at full speed and accuracy -- cost within 1e-11 of the reference's on 50-segment
  // chains of free vertices where the dense pivoted QR is at 1e-5): shadow d_fixed gathered from the caller's, coefficients and
  // cost written straight to the caller's buffers, d_free scattered back with zeros at the pinned slots.
  const bool use_shadow = p->shadow != nullptr;
  mtg_plan* q = use_shadow ? p->shadow : p;
  const int Dd = p->D, nfs = q->n_fixed, nps = q->n_free;
  mtg_layout SL = *L;
  if (use_shadow) {
    mtg_fixed_contiguous(&SL, Dd, nfs);
    mtg_free_contiguous(&SL, Dd, nps);
  }
  const mtg_layout* QL = use_shadow ? &SL : L;
  if (host) {
    std::vector<double> sfx, sfr;
    const double* q_fixed = d_fixed;
    double* q_free = d_free;
    if (use_shadow) {
      sfx.assign((size_t)batch * Dd * std::max(nfs, 1), 0.0);
      sfr.assign((size_t)batch * Dd * std::max(nps, 1), 0.0);
      for (int64_t b = 0; b < batch; ++b) for (int dm = 0; dm < Dd; ++dm) for (int j = 0; j < nfs; ++j) {
            const int c = p->shadow_fixed_src[j];
            if (c >= 0) sfx[((size_t)b * Dd + dm) * nfs + j] = d_fixed[b * L->fixed_stride_b + dm * L->fixed_stride_d + c * L->fixed_stride_c];
          }
      q_fixed = sfx.data();
      q_free = d_free ? sfr.data() : nullptr;
    }
    rc = mtg_solve_impl(q, batch, QL, times, q_fixed, coeffs, q_free, cost, inner, false, ts.data());
    if (use_shadow && d_free && (rc == MTG_OK || rc == MTG_ERR_SINGULAR || rc == MTG_ERR_BAD_SEGMENT_TIME))
      for (int64_t b = 0; b < batch; ++b) for (int dm = 0; dm < Dd; ++dm) for (int j = 0; j < p->n_free; ++j) {
            const int c = p->free_in_shadow[j];
            d_free[b * L->free_stride_b + dm * L->free_stride_d + j * L->free_stride_c] = c >= 0 ? sfr[((size_t)b * Dd + dm) * nps + c] : 0.0;
          }
    // (bit 1 of the reported per-trajectory status: WHICH trajectories got a basic solution -- all of a deficient plan)
    if (traj_status) for (int64_t b = 0; b < batch; ++b) traj_status[b] = ts[b] | (use_shadow ? (int32_t)MTG_FLAG_SINGULAR : 0);
    if (rc != MTG_ERR_SINGULAR && rc != MTG_ERR_BAD_SEGMENT_TIME) return rc;
  } else {
    // The call has its OWN device status word and per-trajectory status, in a buffer of the plan: it neither reads nor clears
    // the context's word, so SINGULAR / BAD_TIME flags left by earlier asynchronous launches of this context are still there
    // for the caller's next mtg_context_sync (round 4 went through mtg_context_sync and lost them).
    int* own_word = nullptr;
    const double* q_fixed = d_fixed;
    double* q_free = d_free;
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
      const int rb = ensure_buffer(ctx, &p->basic_status, &p->basic_status_bytes, sizeof(double) + (size_t)batch * sizeof(int32_t));
      if (rb != MTG_OK) return rb;
      own_word = reinterpret_cast<int*>(p->basic_status);
      dev_ts = (traj_status && !use_shadow) ? traj_status : reinterpret_cast<int32_t*>(p->basic_status + 1);
      if (use_shadow) {
        const size_t n_fx = (size_t)batch * Dd * std::max(nfs, 1), n_fr = (size_t)batch * Dd * std::max(nps, 1);
        const int rs = ensure_buffer(ctx, &p->shadow_buf, &p->shadow_buf_bytes, (n_fx + n_fr) * sizeof(double));
        if (rs != MTG_OK) return rs;
        double* sfx = p->shadow_buf;
        q_fixed = sfx;
        q_free = d_free ? p->shadow_buf + n_fx : nullptr;     // (d_P only when the caller asked for it)
        launch_pin_gather(p, batch, L, d_fixed, sfx, ctx->stream);
      }
    }
    rc = mtg_solve_impl(q, batch, QL, times, q_fixed, coeffs, q_free, cost, inner, false, dev_ts, nullptr, nullptr, own_word);
    if (rc != MTG_OK) return rc;
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
      if (use_shadow && d_free) mtg_launch_pin_scatter(p, batch, L, q_free, d_free, ctx->stream);
      int word = 0;
      MTG_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_status, own_word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      MTG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      word = *ctx->h_status;
      if (word != 0) MTG_HIP_TRY(ctx, hipMemcpy(ts.data(), dev_ts, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (use_shadow && traj_status) {
        std::vector<int32_t> rep(ts);
        for (auto& x : rep) x |= (int32_t)MTG_FLAG_SINGULAR;
        MTG_HIP_TRY(ctx, hipMemcpy(traj_status, rep.data(), (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
      }
      if (word == 0) return MTG_OK;
    }
  }
  // one flagged trajectory after the other: gather its inputs (any strides), solve, recover, scatter
  const int K = p->K, D = p->D, nf = p->n_fixed, np = p->n_free, N = p->N;
  std::vector<double> t(K), fx((size_t)D * std::max(nf, 1)), fr((size_t)D * std::max(np, 1)), co((size_t)K * D * N);
  double cost1 = 0.0;
  bool any_bad_time = false;
  auto pull = [&](double* dst, const double* src, int64_t stride, int count) -> bool {   // dst[i] = src[i * stride]
    if (host) { for (int i = 0; i < count; ++i) dst[i] = src[(int64_t)i * stride]; return true; }
    return hipMemcpy2D(dst, sizeof(double), src, (size_t)stride * sizeof(double), sizeof(double), (size_t)count, hipMemcpyDeviceToHost) == hipSuccess;
  };
  auto push = [&](double* dst, int64_t stride, const double* src, int count) -> bool {   // dst[i * stride] = src[i]
    if (host) { for (int i = 0; i < count; ++i) dst[(int64_t)i * stride] = src[i]; return true; }
    return hipMemcpy2D(dst, (size_t)stride * sizeof(double), src, sizeof(double), sizeof(double), (size_t)count, hipMemcpyHostToDevice) == hipSuccess;
  };
  std::unique_lock<std::mutex> lock(ctx->mu, std::defer_lock);
  if (!host) { lock.lock(); MTG_HIP_TRY(ctx, hipSetDevice(ctx->device)); }
  for (int64_t b = 0; b < batch; ++b) {
    if (ts[b] & MTG_FLAG_BAD_TIME) { any_bad_time = true; continue; }
    if (!(ts[b] & MTG_FLAG_SINGULAR)) continue;
    bool ok = pull(t.data(), times + b * L->times_stride_b, std::max<int64_t>(L->times_stride_k, 1), K);
    for (int d = 0; d < D && ok && nf > 0; ++d)
      ok = pull(fx.data() + (size_t)d * nf, d_fixed + b * L->fixed_stride_b + d * L->fixed_stride_d, std::max<int64_t>(L->fixed_stride_c, 1), nf);
    if (!ok) return set_err(ctx, MTG_ERR_DEVICE, "basic solution: gathering a flagged trajectory failed");
    if (mtg_basic_solution_one(p->H, K, D, p->deriv, p->mask.data(), p->offF.data(), p->offP.data(), t.data(), fx.data(), fr.data()) < 0)
      return set_err(ctx, MTG_ERR_UNSUPPORTED, "basic solution: unsupported shape");
    // coefficients (and the cost) of this one trajectory: host build of the update path, contiguous AoS scratch
    MtgParams P;
    mtg_layout one;
    mtg_layout_aos(p, 1, &one);
    fill_common(p, P, 1, &one);
    int st_word = 0;
    P.times = t.data(); P.dfix = fx.data(); P.coeffs = co.data(); P.dfree = fr.data(); P.cost = cost ? &cost1 : nullptr;
    P.status = &st_word; P.tstatus = nullptr;
    P.vmask = p->mask.data(); P.offF = p->offF.data(); P.offP = p->offP.data();
    if (mtg_host_run(P, p->H, /*update=*/true) != 0) return set_err(ctx, MTG_ERR_UNSUPPORTED, "basic solution: no host update path");
    ok = push(coeffs + b * (int64_t)K * D * N, 1, co.data(), K * D * N);
    for (int d = 0; d < D && ok && d_free && np > 0; ++d)
      ok = push(d_free + b * L->free_stride_b + d * L->free_stride_d, std::max<int64_t>(L->free_stride_c, 1), fr.data() + (size_t)d * np, np);
    if (ok && cost) ok = push(cost + b, 1, &cost1, 1);
    if (!ok) return set_err(ctx, MTG_ERR_DEVICE, "basic solution: writing a trajectory back failed");
  }
  return any_bad_time ? set_err(ctx, MTG_ERR_BAD_SEGMENT_TIME, mtg_status_string(MTG_ERR_BAD_SEGMENT_TIME)) : MTG_OK;
}

// MTG_FLAG_REFINE (asynchronous, device pointers): x = the ordinary solve's d_P; r = -(R_PP x + R_PF d_F) in double-double
// (mtg_refine.hip); R_PP delta = r by the generic float64 kernel (zero fixed values, r as its explicit right-hand side);
// x += delta; coefficients (and the cost) recovered from x by the update path (LIN:263-283).
static int solve_refined(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed,
                         double* coeffs, double* d_free, double* cost, int32_t* traj_status, uint32_t flags) {
  if (!p || !L) return MTG_ERR_INVALID_ARGUMENT;
  mtg_context* ctx = p->ctx;
  if (flags & (MTG_FLAG_HOST_POINTERS | MTG_FLAG_COST_ONLY | MTG_FLAG_BASIC_SOLUTION))
    return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "MTG_FLAG_REFINE: device pointers, coefficient output, not with MTG_FLAG_BASIC_SOLUTION");
  const uint32_t inner = flags & ~(uint32_t)MTG_FLAG_REFINE;
  if (batch <= 0 || p->n_free == 0) return mtg_solve_impl(p, batch, L, times, d_fixed, coeffs, d_free, cost, inner, false, traj_status);
  const size_t nfree = (size_t)batch * p->D * p->n_free, nfix = (size_t)batch * p->D * std::max(p->n_fixed, 1);
  double *xbuf, *rbuf, *dbuf, *zbuf;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rb = ensure_buffer(ctx, &p->refine_buf, &p->refine_buf_bytes, (3 * nfree + nfix) * sizeof(double));
    if (rb != MTG_OK) return rb;
    xbuf = p->refine_buf; rbuf = xbuf + nfree; dbuf = rbuf + nfree; zbuf = dbuf + nfree;
    MTG_HIP_TRY(ctx, hipMemsetAsync(zbuf, 0, nfix * sizeof(double), ctx->stream));
  }
  // x lives in the caller's d_free when there is one, else in the plan's scratch (contiguous [B][D][n_free])
  mtg_layout XL = *L;
  double* x = d_free;
  if (!x) { x = xbuf; mtg_free_contiguous(&XL, p->D, p->n_free); }
  int rc = mtg_solve_impl(p, batch, &XL, times, d_fixed, coeffs, x, nullptr, inner, false, traj_status);
  if (rc != MTG_OK) return rc;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    MtgParams P;
    fill_common(p, P, batch, &XL);
    if (mtg_refine_residual_launch((void*)ctx->stream, p->H, p->K, p->D, p->deriv, P.h1off, P.vmask, P.offF, P.offP, (long long)batch, times,
                                   P.ts_b, P.ts_k, d_fixed, P.fs_b, P.fs_d, P.fs_c, x, P.ps_b, P.ps_d, P.ps_c, rbuf, p->n_free) != 0)
      return set_err(ctx, MTG_ERR_DEVICE, "MTG_FLAG_REFINE: residual launch failed");
  }
  // the correction solve: zero fixed values (contiguous), the residual as explicit right-hand side, delta contiguous
  mtg_layout CL = *L;
  mtg_fixed_contiguous(&CL, p->D, p->n_fixed);
  mtg_free_contiguous(&CL, p->D, p->n_free);
  const uint32_t generic = (inner & ~(uint32_t)(MTG_FLAG_FUSED_DIMS | MTG_FLAG_SPLIT_DIMS | MTG_FLAG_DIMLANE | MTG_FLAG_COOPERATIVE)) | MTG_FLAG_GENERIC_KERNEL;
  rc = mtg_solve_impl(p, batch, &CL, times, zbuf, coeffs, dbuf, nullptr, generic, false, nullptr, nullptr, nullptr, nullptr, rbuf);
  if (rc != MTG_OK) return rc;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mtg_refine_axpy_launch((void*)ctx->stream, x, XL.free_stride_b, XL.free_stride_d, XL.free_stride_c, dbuf, (long long)batch, p->D, p->n_free) != 0)
      return set_err(ctx, MTG_ERR_DEVICE, "MTG_FLAG_REFINE: update launch failed");
  }
  return mtg_solve_impl(p, batch, &XL, times, d_fixed, coeffs, x, cost, inner, true);
}

extern "C" {
int mtg_basic_solution_host(const mtg_plan* p, const double* times, const double* d_fixed, double* d_free, int32_t* rank) {
  if (!p || !times || (p->n_fixed > 0 && !d_fixed) || (p->n_free > 0 && !d_free)) return MTG_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < p->K; ++k)
    if (!(times[k] > 0.0)) return MTG_ERR_BAD_SEGMENT_TIME;
  const int r = mtg_basic_solution_one(p->H, p->K, p->D, p->deriv, p->mask.data(), p->offF.data(), p->offP.data(), times, d_fixed, d_free);
  if (r < 0) return MTG_ERR_UNSUPPORTED;
  if (rank) *rank = r;
  return MTG_OK;
}

// include/mtg_hip_lab.h: the double-double residual alone (what the tests compare with the residual formed at 50 digits)
int mtg_lab_refine_residual(mtg_plan* p, int64_t batch, const mtg_layout* L, const double* times, const double* d_fixed,
                                       const double* d_free, double* rhs_out) {
  if (!p || !L || !times || !d_free || !rhs_out || batch < 0 || (p->n_fixed > 0 && !d_fixed)) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0 || p->n_free == 0) return MTG_OK;
  mtg_context* ctx = p->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  MTG_HIP_TRY(ctx, hipSetDevice(ctx->device));
  MtgParams P;
  fill_common(p, P, batch, L);
  if (mtg_refine_residual_launch((void*)ctx->stream, p->H, p->K, p->D, p->deriv, P.h1off, P.vmask, P.offF, P.offP, (long long)batch, times,
                                 P.ts_b, P.ts_k, d_fixed, P.fs_b, P.fs_d, P.fs_c, d_free, P.ps_b, P.ps_d, P.ps_c, rhs_out, p->n_free) != 0)
    return set_err(ctx, MTG_ERR_DEVICE, "residual launch failed");
  return MTG_OK;
}

int mtg_solve_linear_status(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                            const double* d_fixed, double* coeffs, double* d_free, double* cost, int32_t* trajectory_status, uint32_t flags) {
  if (flags & MTG_FLAG_REFINE) return solve_refined(plan, batch, layout, times, d_fixed, coeffs, d_free, cost, trajectory_status, flags);
  if (flags & MTG_FLAG_BASIC_SOLUTION)
    return solve_with_basic_solution(plan, batch, layout, times, d_fixed, coeffs, d_free, cost, trajectory_status, flags);
  return mtg_solve_impl(plan, batch, layout, times, d_fixed, coeffs, d_free, cost, flags, false, trajectory_status);
}

int mtg_solve_linear(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                     const double* d_fixed, double* coeffs, double* d_free, double* cost, uint32_t flags) {
  return mtg_solve_linear_status(plan, batch, layout, times, d_fixed, coeffs, d_free, cost, nullptr, flags);
}
}  // extern "C"
