"""The shape rules the three per-segment host entries share (csrc/mtg_segment_lane.h: shape_ok): ONE table of argument cases,
run against mtg_check_input_feasibility_host, mtg_magnitude_soft_cost_host and mtg_check_half_plane_feasibility_host.  N below
and above each entry's range, K = 0, D = 0 and above the entry's maximum, batch = -1, a zero stride, time strides that alias two
segments in both layouts, and the accepted neighbour of each.  Return codes only: what the accepted calls compute is the matter
of test_feasibility.py, test_time_objective.py and test_half_plane.py."""
import ctypes

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L

OK, INVALID = 0, -1
B, K = 3, 4                      # of every case that does not vary them
# entry: (smallest N, largest D)
ENTRIES = {"feasibility": (5, 32), "objective": (4, 4), "half_plane": (1, 32)}

# (id, N, K, D, batch, ts_b, ts_k, expected); N as an offset from the entry's minimum ("min", off) or a number, D likewise ("max", off)
CASES = [
    ("n_below_min", ("min", -1), K, 3, B, K, 1, INVALID),
    ("n_min", ("min", 0), K, 3, B, K, 1, OK),
    ("n_odd", 7, K, 3, B, K, 1, OK),
    ("n_12", 12, K, 3, B, K, 1, OK),
    ("n_13", 13, K, 3, B, K, 1, INVALID),
    ("k_0", 10, 0, 3, B, 1, 1, INVALID),
    ("k_1", 10, 1, 3, B, 1, 1, OK),
    ("d_0", 10, K, 0, B, K, 1, INVALID),
    ("d_1", 10, K, 1, B, K, 1, OK),
    ("d_max", 10, K, ("max", 0), B, K, 1, OK),
    ("d_above_max", 10, K, ("max", 1), B, K, 1, INVALID),
    ("batch_minus_1", 10, K, 3, -1, K, 1, INVALID),
    ("batch_0", 10, K, 3, 0, K, 1, OK),
    ("batch_1", 10, K, 3, 1, K, 1, OK),
    ("ts_b_0", 10, K, 3, B, 0, 1, INVALID),
    ("ts_k_0", 10, K, 3, B, K, 0, INVALID),
    ("ts_k_negative", 10, K, 3, B, K, -1, INVALID),
    ("rows_bk_touching", 10, K, 3, B, K * 2, 2, OK),                  # [B][K], segments two apart: rows exactly K * ts_k apart
    ("rows_bk_overlapping", 10, K, 3, B, K * 2 - 1, 2, INVALID),      # ts_b = K ts_k - 1 (and ts_k < B ts_b: not [K][B] either)
    ("rows_bk_padded", 10, K, 3, B, K * 2 + 3, 2, OK),
    ("rows_kb_touching", 10, K, 3, B, 2, B * 2, OK),                  # [K][B], trajectories two apart
    ("rows_kb_overlapping", 10, K, 3, B, 2, B * 2 - 1, INVALID),      # ts_k = B ts_b - 1 (and ts_b < K ts_k)
    ("rows_kb_padded", 10, K, 3, B, 2, B * 2 + 3, OK),
    ("soa", 10, K, 3, B, 1, B, OK),
]


def resolve(entry, n, d):
    n_min, d_max = ENTRIES[entry]
    n = n_min + n[1] if isinstance(n, tuple) else n
    d = d_max + d[1] if isinstance(d, tuple) else d
    return n, d


def call(entry, n, k, d, batch, ts_b, ts_k):
    """The entry's return code on valid data of that shape (buffers sized for the accepted reading of the arguments)."""
    lib = L.load()
    nb, nk, nd, nn = max(batch, 1), max(k, 1), max(d, 1), max(n, 1)
    rng = np.random.default_rng(1000 * nn + nd)
    coeffs = rng.standard_normal((nb, nk, nd, nn))
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    i32 = lambda *shape: np.empty(shape, dtype=np.int32)
    f64 = lambda *shape: np.empty(shape, dtype=np.float64)
    if entry == "feasibility":
        c = m.InputConstraints.defaults().to_c()
        return lib.mtg_check_input_feasibility_host(n, k, d, batch, coeffs.ctypes.data, times.ctypes.data, ts_b, ts_k, ctypes.byref(c),
                                                    i32(nb).ctypes.data, i32(nb).ctypes.data, i32(nb, nk).ctypes.data,
                                                    f64(nb, nk, 6).ctypes.data)
    if entry == "objective":
        c = m.TimeObjectiveParams(constraints=[(1, 2.0)]).to_c()
        return lib.mtg_magnitude_soft_cost_host(n, k, d, batch, coeffs.ctypes.data, times.ctypes.data, ts_b, ts_k, ctypes.byref(c),
                                                f64(nb).ctypes.data, f64(nb, 1).ctypes.data, f64(nb, 1).ctypes.data)
    planes = m.bounding_box_half_planes([0, 0, 0], [50, 50, 50])
    return lib.mtg_check_half_plane_feasibility_host(n, k, d, batch, coeffs.ctypes.data, times.ctypes.data, ts_b, ts_k,
                                                     planes.ctypes.data, 6, 0, 0, i32(nb).ctypes.data, i32(nb).ctypes.data,
                                                     i32(nb).ctypes.data, f64(nb, nk).ctypes.data, f64(nb).ctypes.data)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shared_argument_rules(entry, case):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    n, d = resolve(entry, n, d)
    assert call(entry, n, k, d, batch, ts_b, ts_k) == expected, (entry, name, n, k, d, batch, ts_b, ts_k)


def test_segment_count_limit_of_the_half_plane_word():
    """2^22 segments do not fit segment << 8 | plane: the half-plane host entry refuses them before it reads anything (the
    feasibility host entry has no such limit; its device entry has)."""
    lib = L.load()
    one = np.ones((1,))
    planes = m.bounding_box_half_planes([0, 0, 0], [50, 50, 50])
    out = np.empty((1,), dtype=np.int32)
    assert lib.mtg_check_half_plane_feasibility_host(10, 1 << 22, 3, 0, one.ctypes.data, one.ctypes.data, 1 << 22, 1, planes.ctypes.data,
                                                     6, 0, 0, out.ctypes.data, None, None, None, None) == INVALID
    assert lib.mtg_check_half_plane_feasibility_host(10, (1 << 22) - 1, 3, 0, one.ctypes.data, one.ctypes.data, 1 << 22, 1,
                                                     planes.ctypes.data, 6, 0, 0, out.ctypes.data, None, None, None, None) == OK
