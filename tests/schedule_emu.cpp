// Host build of the mixed-request scheduling rules (csrc/mtg_multi_schedule.h) for tests/test_multi_schedule.py: plain g++, no HIP.
#include "../mav_trajectory_generation_amd/csrc/mtg_multi_schedule.h"

namespace {
struct Unit { int item, tile; };
}

extern "C" {

// khw: [n_items][3] = (K, H, tiles) in launch order; units_out: [sum of tiles][2] = (item, tile); wg_begin_out: [grid + 1].
// Returns the number of units.
int mtg_schedule_emu_dl_any(const int* khw, int n_items, int grid, int round_robin, int* units_out, int* wg_begin_out) {
  std::vector<MtgScheduleItem> items((size_t)n_items);
  for (int i = 0; i < n_items; ++i) items[(size_t)i] = MtgScheduleItem{khw[3 * i], khw[3 * i + 1], khw[3 * i + 2]};
  std::vector<Unit> units;
  std::vector<int> wg_begin;
  mtg_dl_any_schedule(items.data(), n_items, grid, round_robin != 0, units, wg_begin);
  for (size_t u = 0; u < units.size(); ++u) { units_out[2 * u] = units[u].item; units_out[2 * u + 1] = units[u].tile; }
  std::copy(wg_begin.begin(), wg_begin.end(), wg_begin_out);
  return (int)units.size();
}

// order_out, lane_out: [n]; returns the number of lanes
int mtg_schedule_emu_lpt_lanes(const double* estimate, const int* plan_id, int n, int max_lanes, int* order_out, int* lane_out) {
  return mtg_lpt_lanes(estimate, plan_id, n, max_lanes, order_out, lane_out);
}

}  // extern "C"
