// mtg_multi_schedule.h -- the scheduling rules of a mixed request (mtg_multi.hip) as pure functions of a handful of integers:
// no HIP header, plain C++, so that the CPU tests reach them (tests/schedule_emu.cpp, tests/test_multi_schedule.py).
#ifndef MTG_MULTI_SCHEDULE_H_
#define MTG_MULTI_SCHEDULE_H_
#include <algorithm>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

inline long long mtg_work_estimate(int K, int N) { return (long long)K * N * N; }           // work per trajectory ~ chain length x N^2

struct MtgScheduleItem { int K, H, tiles; };   // one item of the cross-structure dimension-in-lane launch, in launch order

// What a schedule depends on (the context caches schedules by it): grid, schedule kind, then (K, H, tiles) per item.
inline std::vector<long long> mtg_dl_any_schedule_key(const MtgScheduleItem* items, int n_items, int grid, bool round_robin) {
  std::vector<long long> key{grid, round_robin ? 1 : 0};
  key.reserve(2 + 3 * (size_t)n_items);
  for (int i = 0; i < n_items; ++i) key.insert(key.end(), {items[i].K, items[i].H, items[i].tiles});
  return key;
}

// Every workgroup gets its own unit list: workgroup w runs units[wg_begin[w] .. wg_begin[w + 1]).  Unit = {item, tile}.
// Default: greedy longest-processing-time assignment (units in item order -- the caller sorts the items by decreasing work -- each
// to the least-loaded workgroup; ties -> the lowest index: the first `grid` units land on workgroups 0, 1, 2, ...).  Cost model
// from the per-bucket kernel times (profiles/r03b_configs.jsonl): ~0.03 us x K x (N/2)^2 + ~2.5 us per unit.
// round_robin (MTG_DL_ANY_SCHED=rr): round 2's schedule (units w, w + grid, ... of the list, every second FULL round reversed).
template <class Unit>
void mtg_dl_any_schedule(const MtgScheduleItem* items, int n_items, int grid, bool round_robin, std::vector<Unit>& units,
                         std::vector<int>& wg_begin) {
  std::vector<Unit> all;
  for (int i = 0; i < n_items; ++i)
    for (int t = 0; t < items[i].tiles; ++t) all.push_back(Unit{i, t});
  std::vector<std::vector<Unit>> lists((size_t)grid);
  if (round_robin) {
    for (size_t r = 0; r * (size_t)grid < all.size(); ++r) {
      const size_t lo = r * (size_t)grid, hi = std::min(all.size(), lo + (size_t)grid);
      const bool rev = (r & 1) && hi - lo == (size_t)grid;
      for (size_t u = lo; u < hi; ++u) lists[rev ? (hi - 1 - u) : (u - lo)].push_back(all[u]);
    }
  } else {
    typedef std::pair<long long, int> Load;      // (load, workgroup): min-heap
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (int w = 0; w < grid; ++w) heap.push(Load(0, w));
    for (const Unit& u : all) {
      const Load l = heap.top();
      heap.pop();
      lists[(size_t)l.second].push_back(u);
      heap.push(Load(l.first + (long long)items[u.item].K * items[u.item].H * items[u.item].H + 90, l.second));
    }
  }
  wg_begin.assign((size_t)grid + 1, 0);
  units.clear();
  units.reserve(all.size());
  for (int w = 0; w < grid; ++w) {
    units.insert(units.end(), lists[(size_t)w].begin(), lists[(size_t)w].end());
    wg_begin[(size_t)w + 1] = (int)units.size();
  }
}

// Side streams of MTG_FLAG_CONCURRENT_ITEMS: longest-processing-time-first.  order[s]: the items by decreasing estimate (stable);
// lane_of[s]: the least-loaded lane when order[s] is placed -- or, items of one plan sharing its workspace (same stream, in
// order), the lane of that plan's earlier item.  Returns the number of lanes, min(max_lanes, n).
inline int mtg_lpt_lanes(const double* estimate, const int* plan_id, int n, int max_lanes, int* order, int* lane_of) {
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order, order + n, [&](int a, int b) { return estimate[a] > estimate[b]; });
  const int n_lanes = std::min(max_lanes, n);
  std::vector<double> load((size_t)std::max(1, n_lanes), 0.0);
  for (int s = 0; s < n; ++s) {
    int lane = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    for (int r = 0; r < s; ++r)
      if (plan_id[order[r]] == plan_id[order[s]]) lane = lane_of[r];
    load[(size_t)lane] += estimate[order[s]];
    lane_of[s] = lane;
  }
  return n_lanes;
}

#endif  // MTG_MULTI_SCHEDULE_H_
