"""The scheduling rules of a mixed request (csrc/mtg_multi_schedule.h, used by csrc/mtg_multi.hip: mtg_multi_create) as pure
functions, built for the host (tests/schedule_emu.cpp): the per-workgroup unit lists of the cross-structure dimension-in-lane
launch -- greedy through a min-heap of (load, workgroup), or round-robin with every second full round reversed -- and the
side-stream assignment of MTG_FLAG_CONCURRENT_ITEMS.  Each against an independent restatement written here, element for element
(the tie rule -- lowest workgroup index -- is part of the behaviour), and against the invariants any valid schedule has.  No GPU."""
import ctypes
import heapq
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")

ITEMS = [(32, 6, 2), (8, 5, 7), (8, 5, 1), (4, 4, 3)]      # (K, H, tiles): 13 units
# (items, grid, round robin): ties in the heap, one unit per workgroup, a single item; three full rounds and a partial one (the
# reversed and the unreversed branch), two full rounds and a partial one
CASES = [(ITEMS, 4, False), (ITEMS, 13, False), ([(8, 5, 5)], 2, False), (ITEMS, 4, True), (ITEMS, 5, True)]


@pytest.fixture(scope="module")
def emu():
    so, src = os.path.join(ROOT, "tests", "libmtg_schedule_emu.so"), os.path.join(ROOT, "tests", "schedule_emu.cpp")
    deps = [src, os.path.join(CSRC, "mtg_multi_schedule.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.mtg_schedule_emu_dl_any.argtypes = [ip, ctypes.c_int, ctypes.c_int, ctypes.c_int, ip, ip]
    lib.mtg_schedule_emu_lpt_lanes.argtypes = [dp, ip, ctypes.c_int, ctypes.c_int, ip, ip]
    return lib


def unit_cost(item):
    k, h, _ = item
    return k * h * h + 90


def library_schedule(lib, items, grid, rr):
    ip = ctypes.POINTER(ctypes.c_int)
    khw = np.ascontiguousarray(items, dtype=np.int32)
    nunits = sum(t for _, _, t in items)
    units = np.full((nunits, 2), -1, dtype=np.int32)
    wg_begin = np.full(grid + 1, -1, dtype=np.int32)
    n = lib.mtg_schedule_emu_dl_any(khw.ctypes.data_as(ip), len(items), grid, int(rr), units.ctypes.data_as(ip), wg_begin.ctypes.data_as(ip))
    assert n == nunits
    return [tuple(u) for u in units.tolist()], wg_begin.tolist()


def restated_schedule(items, grid, rr):
    """Units in item order, then tile order.  Greedy: each to the workgroup on top of a heap of (load, workgroup) tuples, whose load
    grows by K H^2 + 90.  Round-robin: unit u of round r = u // grid goes to workgroup u % grid, mirrored in odd FULL rounds."""
    units = [(i, t) for i, (_, _, tiles) in enumerate(items) for t in range(tiles)]
    lists = [[] for _ in range(grid)]
    if rr:
        for u, unit in enumerate(units):
            r, pos = divmod(u, grid)
            full = (r + 1) * grid <= len(units)
            lists[grid - 1 - pos if (r % 2 == 1 and full) else pos].append(unit)
    else:
        heap = [(0, w) for w in range(grid)]
        heapq.heapify(heap)
        for unit in units:
            load, w = heapq.heappop(heap)
            lists[w].append(unit)
            heapq.heappush(heap, (load + unit_cost(items[unit[0]]), w))
    wg_begin = [0]
    for lst in lists:
        wg_begin.append(wg_begin[-1] + len(lst))
    return [u for lst in lists for u in lst], wg_begin


@pytest.mark.parametrize("items,grid,rr", CASES)
def test_unit_lists_equal_the_restatement(emu, items, grid, rr):
    assert library_schedule(emu, items, grid, rr) == restated_schedule(items, grid, rr)


@pytest.mark.parametrize("items,grid,rr", CASES)
def test_schedule_invariants(emu, items, grid, rr):
    units, wg_begin = library_schedule(emu, items, grid, rr)
    nunits = sum(t for _, _, t in items)
    assert len(wg_begin) == grid + 1 and wg_begin[0] == 0 and wg_begin[grid] == nunits
    assert all(a <= b for a, b in zip(wg_begin, wg_begin[1:]))
    assert sorted(units) == [(i, t) for i, (_, _, tiles) in enumerate(items) for t in range(tiles)]      # every pair exactly once
    if not rr:
        # always assigning to the least-loaded workgroup keeps the loads within one (largest) unit cost of each other
        loads = [sum(unit_cost(items[i]) for i, _ in units[wg_begin[w]:wg_begin[w + 1]]) for w in range(grid)]
        assert max(loads) - min(loads) <= max(unit_cost(it) for it in items)


def test_partial_round_and_empty_workgroups_are_reached():
    """The cases are the ones they claim to be (restatement only)."""
    _, wg4 = restated_schedule(ITEMS, 4, True)
    assert [b - a for a, b in zip(wg4, wg4[1:])] == [4, 3, 3, 3]            # 13 = 3 full rounds + 1 unit
    units5, wg5 = restated_schedule(ITEMS, 5, True)
    assert units5[wg5[4]:wg5[5]] == [(1, 2), (1, 3)]                         # round 1 reversed: its first unit on the last workgroup
    _, wg = restated_schedule([(8, 5, 5)], 8, False)
    assert wg[5:] == [5, 5, 5, 5]                                            # more workgroups than units: empty lists


def library_lanes(lib, est, plan_id, max_lanes):
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    e, pid = np.ascontiguousarray(est, dtype=np.float64), np.ascontiguousarray(plan_id, dtype=np.int32)
    order, lane = np.full(len(est), -1, dtype=np.int32), np.full(len(est), -1, dtype=np.int32)
    n_lanes = lib.mtg_schedule_emu_lpt_lanes(e.ctypes.data_as(dp), pid.ctypes.data_as(ip), len(est), max_lanes, order.ctypes.data_as(ip),
                                             lane.ctypes.data_as(ip))
    return n_lanes, order.tolist(), lane.tolist()


def restated_lanes(est, plan_id, max_lanes):
    """Items by decreasing estimate (stable); each on the least-loaded lane (lowest index on ties) unless its plan already has one."""
    order = sorted(range(len(est)), key=lambda i: -est[i])
    n_lanes = min(max_lanes, len(est))
    load, lane_of_plan, lanes = [0.0] * n_lanes, {}, []
    for i in order:
        lane = lane_of_plan.setdefault(plan_id[i], load.index(min(load)))
        load[lane] += est[i]
        lanes.append(lane)
    return n_lanes, order, lanes


@pytest.mark.parametrize("est,plan_id", [([5, 9, 9, 1, 4, 7], [0, 1, 2, 0, 3, 1]), ([3, 8, 5], [0, 1, 2])])
def test_lane_assignment(emu, est, plan_id):
    n_lanes, order, lanes = library_lanes(emu, est, plan_id, 4)
    assert (n_lanes, order, lanes) == restated_lanes(est, plan_id, 4)
    assert n_lanes == min(4, len(est)) and all(0 <= lane < n_lanes for lane in lanes)
    lane_of_item = dict(zip(order, lanes))
    for a in range(len(est)):
        for b in range(len(est)):
            if plan_id[a] == plan_id[b]:
                assert lane_of_item[a] == lane_of_item[b]
