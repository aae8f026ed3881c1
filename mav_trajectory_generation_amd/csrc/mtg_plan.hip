// mtg_plan.hip -- the C ABI of include/mtg_hip.h, part 2: the structural rank decision, plan creation (with the shadow plan of
// a structurally rank-deficient pattern) and destruction, the plan queries.
#include "mtg_abi_internal.h"

// the generic kernels of a polynomial order (one translation unit each), resolved into the plan's MtgPlanForms
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

// STRUCTURAL rank deficiency of R_PP.  The cost 0.5 d^T R d = sum over segments of the integral of (p^(d))^2 (LIN:124-140) vanishes
// exactly on the trajectories whose every segment is a polynomial of degree < d; interior vertices share all h >= d + 1
// derivative slots (LIN:199-205), so those are ONE polynomial of degree < d over the whole trajectory, and the null space of R_PP
// is the subspace of it on which every FIXED slot vanishes: the functionals  p -> p^(q)(t_v)  for the fixed slots (v, q), q < d.
// Its dimension d - rank(those functionals on P_(d-1)) depends on the constraint PATTERN only (Hermite data at distinct
// instants are always independent; Birkhoff-type patterns -- a derivative fixed without the lower ones -- generically), not on
// the batch's segment times: it is computed here, once per plan, at two sets of generic vertex instants.
// Why not in the kernels: the reference decides "rank-deficient" with a rank-revealing QR (LIN:365-367); an LDL^T sweep sees a
// zero pivot as round-off x the conditioning of everything eliminated before it -- on chains of free vertices that is anything
// between 1e-12 and 1e0 of the diagonal, of either sign (tests/test_pivot_threshold.py), overlapping the legitimate pivots of
// regular ill-conditioned problems (1e-7 of the diagonal).  No pivot threshold separates the two; the structure does.
// pins (optional): null_dim free slots (vertex, derivative), lowest vertices / derivatives first, whose functionals complete the
// fixed ones to a basis of P_(d-1)'s dual -- fixing them (to zero) makes the system regular without changing the minimum cost
// (any minimiser differs from one that satisfies them by an element of the null space).
static int structural_null_dim(int H, int K, int d, const std::vector<int>& mask, std::vector<std::pair<int, int>>* pins = nullptr) {
  if (pins) pins->clear();
  if (d <= 0) return 0;
  int best_rank = 0;
  for (int trial = 0; trial < 2 && best_rank < d; ++trial) {
    // generic vertex instants in [0, 1]: increments from a fixed irrational rotation (the two trials share no ratio)
    std::vector<long double> tv((size_t)K + 1, 0.0L);
    for (int v = 1; v <= K; ++v) {
      const long double u = (v + 1) * (trial == 0 ? 0.6180339887498948482L : 0.4142135623730950488L);
      tv[v] = tv[v - 1] + (0.35L + (u - (long long)u)) / (long double)K;
    }
    auto functional = [&](int v, int q, std::vector<long double>& row) {      // p -> p^(q)(t_v) on the monomials 1, t, ..., t^(d-1)
      row.assign((size_t)d, 0.0L);
      for (int m = q; m < d; ++m) {
        long double c = 1.0L;
        for (int i = 0; i < q; ++i) c *= (long double)(m - i);
        for (int i = 0; i < m - q; ++i) c *= tv[v];
        row[m] = c;
      }
    };
    // incremental echelon basis: basis[i] has its pivot (largest entry at insertion) in column piv[i]
    std::vector<std::vector<long double>> basis;
    std::vector<int> piv;
    auto add_if_independent = [&](std::vector<long double> row) -> bool {
      long double scale = 0.0L;
      for (long double x : row) scale = std::max(scale, std::fabs(x));
      if (scale == 0.0L) return false;
      for (size_t i = 0; i < basis.size(); ++i) {
        const long double f = row[piv[i]] / basis[i][piv[i]];
        if (f != 0.0L) for (int c = 0; c < d; ++c) row[c] -= f * basis[i][c];
        row[piv[i]] = 0.0L;
      }
      int pc = -1;
      long double big = 1e-9L * scale;
      for (int c = 0; c < d; ++c) if (std::fabs(row[c]) > big) { big = std::fabs(row[c]); pc = c; }
      if (pc < 0) return false;
      basis.push_back(row);
      piv.push_back(pc);
      return true;
    };
    std::vector<long double> row;
    for (int v = 0; v <= K; ++v)
      for (int q = 0; q < H && q < d; ++q) if ((mask[v] >> q) & 1) { functional(v, q, row); add_if_independent(row); }
    const int rank = (int)basis.size();
    if (rank > best_rank) {
      best_rank = rank;
      if (pins) {
        pins->clear();
        for (int v = 0; v <= K && (int)basis.size() < d; ++v) for (int q = 0; q < H && q < d && (int)basis.size() < d; ++q) {
            if ((mask[v] >> q) & 1) continue;
            functional(v, q, row);
            if (add_if_independent(row)) pins->push_back({v, q});
          }
      }
    }
  }
  return d - best_rank;
}

extern "C" {
int mtg_plan_rank_deficiency(const mtg_plan* p) { return p ? p->null_dim : MTG_ERR_INVALID_ARGUMENT; }

int mtg_structural_rank_deficiency(int32_t n_coeffs, int32_t n_segments, int32_t derivative_to_optimize, const uint32_t* fixed_mask) {
  if (n_coeffs < 2 || n_coeffs > MTG_MAX_N || (n_coeffs & 1) || n_segments < 1 || !fixed_mask || derivative_to_optimize < 0 ||
      derivative_to_optimize > n_coeffs / 2 - 1)
    return MTG_ERR_INVALID_ARGUMENT;
  const int H = n_coeffs / 2;
  std::vector<int> mask((size_t)n_segments + 1);
  int n_free = 0;
  for (int v = 0; v <= n_segments; ++v) {
    mask[v] = (int)(fixed_mask[v] & (uint32_t)((1 << H) - 1));
    n_free += H - __builtin_popcount((unsigned)mask[v]);
  }
  return n_free > 0 ? structural_null_dim(H, n_segments, derivative_to_optimize, mask) : 0;
}

int mtg_plan_create(mtg_context* ctx, const mtg_plan_desc* desc, mtg_plan** out) {
  if (!ctx || !desc || !out || !desc->fixed_mask) return MTG_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const int N = desc->n_coeffs, D = desc->dimension, K = desc->n_segments, d = desc->derivative_to_optimize;
  if (N < 2 || N > MTG_MAX_N || (N & 1)) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "n_coeffs must be even in [2,12]");
  if (D < 1 || K < 1) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "dimension and n_segments must be >= 1");
  if (d < 0 || d > N / 2 - 1) return set_err(ctx, MTG_ERR_INVALID_ARGUMENT, "derivative_to_optimize out of range");
  mtg_plan* p = new (std::nothrow) mtg_plan();
  if (!p) return MTG_ERR_DEVICE;
  p->ctx = ctx; p->N = N; p->H = N / 2; p->D = D; p->K = K; p->deriv = d;
  const int full = (1 << p->H) - 1;
  p->mask.resize(K + 1);
  p->offF.assign(K + 2, 0);
  p->offP.assign(K + 2, 0);
  for (int v = 0; v <= K; ++v) {
    p->mask[v] = (int)(desc->fixed_mask[v] & (uint32_t)full);
    const int nf = __builtin_popcount((unsigned)p->mask[v]);
    p->offF[v + 1] = p->offF[v] + nf;
    p->offP[v + 1] = p->offP[v] + (p->H - nf);
  }
  p->n_fixed = p->offF[K + 1];
  p->n_free = p->offP[K + 1];
  std::vector<std::pair<int, int>> pins;
  p->null_dim = p->n_free > 0 ? structural_null_dim(p->H, K, d, p->mask, &pins) : 0;
  // everything of the launch decision that depends on the plan alone (mtg_launch_plan.h): the only table searches of a plan's life
  MtgPlanForms& f = p->forms;
  const int* mask = p->mask.data();
  f.H = p->H; f.D = D; f.K = K; f.n_fixed = p->n_fixed;
  f.free_mid = p->H - __builtin_popcount((unsigned)mask[(K + 1) / 2]);
  f.fast = mtg_find_static(p->H, D, K, d, mask);
  for (int dg = 1; dg < D && !f.fast_split; ++dg) {
    if (D % dg == 0) f.fast_split = mtg_find_static(p->H, dg, K, d, mask);
  }
  f.rolled = mtg_find_static(p->H, D, K, d, mask, true);
  for (int dg = 1; dg <= 4; ++dg) f.group[dg] = mtg_find_static(p->H, dg, K, d, mask);
  f.slab = mtg_find_slab(p->H, D, K, d, mask);
  f.dimlane = mtg_find_dimlane(p->H, D, K, d, mask);
  f.dimlane_rt = mtg_find_dimlane_rt(p->H, D, K, d, mask);
  f.coop_shape = mask[0] == full && mask[K] == full;
  for (int v = 1; v < K; ++v) f.coop_shape = f.coop_shape && mask[v] == 1;
  f.coop_lds = mtg_coop_lds_bytes(p->H, D, K);
  for (int dc = 1; dc <= 4; ++dc) {
    for (int mode = 0; mode < 3; ++mode) f.generic_solve[dc][mode] = mtg_pick_generic_solve(p->H, dc, mode);
    for (int wc = 0; wc < 2; ++wc) f.generic_update[dc][wc] = mtg_pick_generic_update(p->H, dc, wc != 0);
  }
  std::vector<int> tab;
  tab.insert(tab.end(), p->mask.begin(), p->mask.end());
  tab.insert(tab.end(), p->offF.begin(), p->offF.end());
  tab.insert(tab.end(), p->offP.begin(), p->offP.end());
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void**)&p->d_tables, tab.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(p->d_tables, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    delete p;
    return set_err(ctx, MTG_ERR_DEVICE, "plan table upload failed");
  }
  if (p->null_dim > 0 && (int)pins.size() == p->null_dim) {
    // the shadow plan: the same problem with the pinned slots fixed (a regular pattern: its own null_dim is 0, no recursion)
    std::vector<uint32_t> smask((size_t)K + 1);
    for (int v = 0; v <= K; ++v) smask[v] = (uint32_t)p->mask[v];
    for (auto& pq : pins) smask[pq.first] |= 1u << pq.second;
    mtg_plan_desc sd{N, D, K, d, smask.data()};
    const int rs = mtg_plan_create(ctx, &sd, &p->shadow);
    if (rs != MTG_OK || p->shadow->null_dim != 0) {
      if (p->shadow) mtg_plan_destroy(p->shadow);
      p->shadow = nullptr;       // (the per-trajectory pivoted QR of mtg_basic.cpp stays as the way to a basic solution)
    } else {
      int src = 0, sfree = 0;
      for (int v = 0; v <= K; ++v) for (int q = 0; q < p->H; ++q) {
          const bool fixed = (p->mask[v] >> q) & 1, sfixed = (smask[v] >> q) & 1;
          if (sfixed) p->shadow_fixed_src.push_back(fixed ? src : -1);
          if (fixed) ++src;
          if (!fixed) p->free_in_shadow.push_back(sfixed ? -1 : sfree);
          if (!sfixed) ++sfree;
        }
      std::vector<int> maps(p->shadow_fixed_src);
      maps.insert(maps.end(), p->free_in_shadow.begin(), p->free_in_shadow.end());
      if (hipMalloc((void**)&p->d_shadow_maps, maps.size() * sizeof(int)) != hipSuccess ||
          hipMemcpy(p->d_shadow_maps, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        mtg_plan_destroy(p);
        return set_err(ctx, MTG_ERR_DEVICE, "plan table upload failed");
      }
    }
  }
  *out = p;
  return MTG_OK;
}

int mtg_plan_destroy(mtg_plan* p) {
  if (!p) return MTG_OK;
  hipSetDevice(p->ctx->device);
  hipStreamSynchronize(p->ctx->stream);
  for (void* buf : {(void*)p->d_tables, (void*)p->ws, (void*)p->pert_cost, (void*)p->objective_ws, (void*)p->stage, (void*)p->basic_status,
                    (void*)p->d_shadow_maps, (void*)p->shadow_buf, (void*)p->refine_buf})
    if (buf) hipFree(buf);
  if (p->shadow) mtg_plan_destroy(p->shadow);
  delete p;
  return MTG_OK;
}

mtg_context* mtg_plan_context(const mtg_plan* p) { return p ? p->ctx : nullptr; }

int mtg_plan_get_shape(const mtg_plan* p, int32_t* n_coeffs, int32_t* dimension, int32_t* n_segments, int32_t* derivative_to_optimize) {
  if (!p) return MTG_ERR_INVALID_ARGUMENT;
  if (n_coeffs) *n_coeffs = p->N;
  if (dimension) *dimension = p->D;
  if (n_segments) *n_segments = p->K;
  if (derivative_to_optimize) *derivative_to_optimize = p->deriv;
  return MTG_OK;
}

int mtg_plan_get_info(const mtg_plan* p, mtg_plan_info* out) {
  if (!p || !out) return MTG_ERR_INVALID_ARGUMENT;
  out->n_all = p->N * p->K;
  out->n_fixed = p->n_fixed;
  out->n_free = p->n_free;
  out->kernel_variant = p->forms.fast ? (p->forms.fast->k < 0 ? 3 : 1) : (p->forms.fast_split ? 2 : 0);
  out->algorithmic_bytes_per_trajectory = 8ll * (p->K + (int64_t)p->D * p->n_fixed + (int64_t)p->K * p->D * p->N);
  return MTG_OK;
}

// used by mtg_workload.hip: a plan's context, shape and device-resident mask table
int mtg_plan_context_tables(const mtg_plan* plan, mtg_context** ctx, int* n_coeffs, int* dimension, int* n_segments, const int** device_masks) {
  if (!plan || !ctx || !n_coeffs || !dimension || !n_segments || !device_masks) return MTG_ERR_INVALID_ARGUMENT;
  *ctx = plan->ctx; *n_coeffs = plan->N; *dimension = plan->D; *n_segments = plan->K;
  *device_masks = plan->d_tables;     // [K + 1] fixed masks, then the offset tables
  return MTG_OK;
}
}  // extern "C"
