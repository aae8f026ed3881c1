// Host build of the launch decision (csrc/mtg_launch_plan.h) for tests/test_launch_plan.py: plain g++, no HIP.  The table entries
// are fabricated from the caller's integers; every kernel / launch-function pointer is a dummy non-null address that encodes a
// TAG (never called), so that the test sees which entry's which function a launch names.
// With -DMTG_LAUNCH_PLAN_EMU_MAIN: a stand-alone program that reads cases ("plan ... | knobs ... | call ..." integers, one case per
// line, as test_launch_plan.py --dump writes them) from standard input and prints the decisions (for sanitizer runs).
#include <stdint.h>
#include <string.h>

#include "../mav_trajectory_generation_amd/csrc/mtg_launch_plan.h"

namespace {
char tag_base[8192];   // tag t = the address tag_base + t
template <class Fn> Fn tagged(int tag) { return reinterpret_cast<Fn>(reinterpret_cast<uintptr_t>(tag_base + tag)); }
template <class Fn> long long tag_of(Fn fn) { return fn ? (long long)(reinterpret_cast<uintptr_t>(fn) - reinterpret_cast<uintptr_t>(tag_base)) : 0; }

constexpr int kStaticInts = 7, kPlanInts = 7 + 7 * kStaticInts + 4 + 11 + 6 + 1, kKnobInts = 14, kCallInts = 14, kLaunchInts = 15;

// Fabricated entries of one plan.  Tags: static entry e (1 fast, 2 fast_split, 3 rolled, 4 + dg group[dg]): fn[i] = 100 e + i,
// upd[w] = 100 e + 10 + w, upd_slab[w][phase] = 100 e + 20 + 2 w + phase; slab: fn[i] = 1000 + i, queue 1002, extra 1003; generic
// solve [dc][mode] = 2000 + 10 dc + mode, update [dc][wc] = 2100 + 10 dc + wc; dimlane launch 3000 / queue 3001 / extra 3002;
// run-time-K launch 3100.
struct Fabricated {
  MtgPlanForms f;
  MtgStaticEntry st[7];
  MtgSlabEntry slab;
  MtgDimlaneEntry dl;
  MtgDimlaneRtEntry rt;
  // plan: H D K n_fixed free_mid coop_shape coop_lds | 7 x (present d k heavy has_upd has_upd_slab upd_slab_lds) |
  //       slab: present lds has_queue has_extra | dimlane: present h k np tpw lo hi lds ws_per_lane has_queue has_extra |
  //       run-time-K: present tpw r_steps l_steps lds step_bytes_per_lane | generic kernels present
  explicit Fabricated(const long long* p) {
    memset(st, 0, sizeof(st)); memset(&slab, 0, sizeof(slab)); memset(&dl, 0, sizeof(dl)); memset(&rt, 0, sizeof(rt));
    f.H = (int)p[0]; f.D = (int)p[1]; f.K = (int)p[2]; f.n_fixed = (int)p[3]; f.free_mid = (int)p[4];
    f.coop_shape = p[5] != 0; f.coop_lds = (size_t)p[6];
    p += 7;
    const MtgStaticEntry** slot[7] = {&f.fast, &f.fast_split, &f.rolled, &f.group[1], &f.group[2], &f.group[3], &f.group[4]};
    for (int e = 0; e < 7; ++e, p += kStaticInts) {
      if (!p[0]) continue;
      MtgStaticEntry& s = st[e];
      const int t = 100 * (e + 1);
      s.h = f.H; s.d = (int)p[1]; s.k = (int)p[2]; s.heavy = (int)p[3];
      for (int i = 0; i < 5; ++i) s.fn[i] = tagged<SolveFn>(t + i);
      for (int w = 0; w < 2; ++w) {
        if (p[4]) s.upd[w] = tagged<UpdateFn>(t + 10 + w);
        for (int ph = 0; ph < 2 && p[5]; ++ph) s.upd_slab[w][ph] = tagged<UpdateFn>(t + 20 + 2 * w + ph);
      }
      s.upd_slab_lds = (size_t)p[6];
      *slot[e] = &s;
    }
    if (p[0]) {
      slab.h = f.H; slab.d = f.D; slab.k = f.K; slab.lds = (size_t)p[1];
      slab.fn[0] = tagged<SolveFn>(1000); slab.fn[1] = tagged<SolveFn>(1001);
      if (p[2]) slab.queue = tagged<SolveQueueFn>(1002);
      if (p[3]) slab.extra = tagged<SolveFn>(1003);
      f.slab = &slab;
    }
    p += 4;
    if (p[0]) {
      dl.h = (int)p[1]; dl.k = (int)p[2]; dl.dl = f.D; dl.np = (int)p[3]; dl.tpw = (int)p[4]; dl.lo_per_cu = (int)p[5]; dl.hi_per_cu = (int)p[6];
      dl.lds = (size_t)p[7]; dl.ws_per_lane = (size_t)p[8];
      dl.launch = tagged<decltype(dl.launch)>(3000);
      if (p[9]) dl.launch_queue = tagged<decltype(dl.launch_queue)>(3001);
      if (p[10]) dl.launch_extra = tagged<decltype(dl.launch_extra)>(3002);
      f.dimlane = &dl;
    }
    p += 11;
    if (p[0]) {
      rt.h = f.H; rt.dl = f.D; rt.tpw = (int)p[1]; rt.r_steps = (int)p[2]; rt.l_steps = (int)p[3]; rt.lds = (size_t)p[4];
      rt.step_bytes_per_lane = (size_t)p[5];
      rt.launch = tagged<decltype(rt.launch)>(3100);
      f.dimlane_rt = &rt;
    }
    p += 6;
    for (int dc = 1; dc <= 4 && p[0]; ++dc) {
      for (int m = 0; m < 3; ++m) f.generic_solve[dc][m] = tagged<SolveFn>(2000 + 10 * dc + m);
      for (int w = 0; w < 2; ++w) f.generic_update[dc][w] = tagged<UpdateFn>(2100 + 10 * dc + w);
    }
  }
};

// knobs: force_dg prefer_rolled no_dimlane dl_max_units_per_cu no_slab no_slab_extra no_dl_extra no_queue dl_grid_per_cu dl_rt
//        no_balance slab_policy rolled_wg_per_cu coop
MtgKnobs knobs_of(const long long* k) {
  MtgKnobs kn;
  kn.force_dg = (int)k[0]; kn.prefer_rolled = k[1] != 0; kn.no_dimlane = k[2] != 0; kn.dl_max_units_per_cu = (int)k[3];
  kn.no_slab = k[4] != 0; kn.no_slab_extra = k[5] != 0; kn.no_dl_extra = k[6] != 0; kn.no_queue = k[7] != 0;
  kn.dl_grid_per_cu = (int)k[8]; kn.dl_rt = (int)k[9]; kn.no_balance = k[10] != 0; kn.slab_policy = (int)k[11];
  kn.rolled_wg_per_cu = (int)k[12]; kn.coop = (int)k[13];
  return kn;
}
mtg_layout layout_of(const long long* s) { return mtg_layout{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]}; }

void put_launch(const MtgLaunch& l, long long* o) {
  const long long fn = l.fn ? tag_of(l.fn) : l.dl ? tag_of(l.dl->launch) : l.rt ? tag_of(l.rt->launch) : 0;
  const long long v[kLaunchInts] = {fn, l.dl != nullptr, l.rt != nullptr, l.coop, l.grid, l.gridy, l.block, (long long)l.lds, l.dim0, l.ntiles,
                                    (long long)l.ws_bytes, l.ws_stride, l.input_kind, (long long)l.attr, l.user_ws_param};
  memcpy(o, v, sizeof(v));
}
}  // namespace

extern "C" {

// call: batch | 8 layout strides (times b k, fixed b d c, free b d c) | flags update extra cost_only pert
// out: form, n, error | n x (fn tag, dl, rt, coop, grid, gridy, block, lds, dim0, ntiles, ws_bytes, ws_stride, input_kind, attr,
// user_ws_param); at most max_launches launches are written.  Returns the number of launches.
int mtg_launch_plan_emu(const long long* plan, const long long* knobs, int n_cu, const long long* call, int max_launches, long long* out) {
  const Fabricated fab(plan);
  const mtg_layout L = layout_of(call + 1);
  MtgCall c;
  c.batch = call[0]; c.L = &L; c.flags = (uint32_t)call[9];
  c.update = call[10] != 0; c.extra = call[11] != 0; c.cost_only = call[12] != 0; c.pert = call[13] != 0;
  const MtgLaunchPlan lp = mtg_launch_plan(fab.f, knobs_of(knobs), n_cu, c);
  out[0] = (long long)lp.form; out[1] = lp.n; out[2] = lp.error != nullptr;
  for (int i = 0; i < lp.n && i < max_launches; ++i) put_launch(lp.at(i), out + 3 + kLaunchInts * i);
  return lp.n;
}

// queue: n, batch, 8 layout strides, flags.  out: slab chosen, dimlane chosen, tiles_per_batch, input_kind, launches | per launch
// of up to kSeqMax batches: the fields of mtg_launch_plan_emu (fn tag: the queue kernel / launch function).
int mtg_queue_plan_emu(const long long* plan, const long long* knobs, int n_cu, const long long* queue, int max_launches, long long* out) {
  const Fabricated fab(plan);
  const MtgKnobs kn = knobs_of(knobs);
  const mtg_layout L = layout_of(queue + 2);
  const int n = (int)queue[0];
  const MtgQueuePlan q = mtg_queue_plan(fab.f, kn, n_cu, n, queue[1], &L, (uint32_t)queue[10]);
  int launches = 0;
  for (int i0 = 0; (q.slab || q.dl) && i0 < n; i0 += kSeqMax, ++launches) {
    if (launches >= max_launches) continue;
    long long* o = out + 5 + kLaunchInts * launches;
    put_launch(mtg_queue_launch(q, kn, n_cu, std::min(kSeqMax, n - i0)), o);
    o[0] = q.dl ? tag_of(q.dl->launch_queue) : tag_of(q.slab->queue);
  }
  out[0] = q.slab != nullptr; out[1] = q.dl != nullptr; out[2] = q.tiles_per_batch; out[3] = q.input_kind; out[4] = launches;
  return launches;
}

// the small rules mtg_multi.hip shares: which = 0 mtg_dl_offsets_fit(batch = a, padded = b), 1 mtg_all_resident(tiles = a, groups = b),
// 2 mtg_stage_lds_bytes(dims = a, N = b), 3 mtg_solve_lds_bytes(dims = a, N = b, free_mid = c), 4 mtg_balanced_grid(ntiles = a, cap = b)
long long mtg_launch_rule_emu(const long long* plan, const long long* knobs, int n_cu, int which, long long a, long long b, long long c) {
  const Fabricated fab(plan);
  switch (which) {
    case 0: return mtg_dl_offsets_fit(fab.f, a, b != 0);
    case 1: return mtg_all_resident(a, (int)b, n_cu);
    case 2: return (long long)mtg_stage_lds_bytes((int)a, (int)b);
    case 3: return (long long)mtg_solve_lds_bytes((int)a, (int)b, (int)c);
    case 4: return mtg_balanced_grid(knobs_of(knobs), (int)a, (int)b);
  }
  return -1;
}

}  // extern "C"

#ifdef MTG_LAUNCH_PLAN_EMU_MAIN
#include <cstdio>
#include <vector>
// one case per line: kind (0 call, 1 queue), n_cu, then plan, knobs and call / queue integers; prints the outputs
int main() {
  long long kind, n_cu;
  int cases = 0;
  while (scanf("%lld %lld", &kind, &n_cu) == 2) {
    const int tail = kind == 0 ? kCallInts : 11;
    std::vector<long long> in((size_t)(kPlanInts + kKnobInts + tail));
    for (long long& v : in) if (scanf("%lld", &v) != 1) return 2;
    std::vector<long long> out(5 + kLaunchInts * 8, 0);
    const int n = kind == 0 ? mtg_launch_plan_emu(in.data(), in.data() + kPlanInts, (int)n_cu, in.data() + kPlanInts + kKnobInts, 8, out.data())
                            : mtg_queue_plan_emu(in.data(), in.data() + kPlanInts, (int)n_cu, in.data() + kPlanInts + kKnobInts, 8, out.data());
    for (int i = 0; i < (kind == 0 ? 3 : 5) + kLaunchInts * std::min(n, 8); ++i) printf("%lld ", out[(size_t)i]);
    printf("\n");
    ++cases;
  }
  fprintf(stderr, "%d cases\n", cases);
  return cases > 0 ? 0 : 1;
}
#endif
