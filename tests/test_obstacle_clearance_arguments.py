"""Argument table of mtg_check_obstacle_clearance_host, after tests/test_segment_arguments.py: the shape rules the per-segment
host entries share (csrc/mtg_segment_lane.h: shape_ok) with this entry's own limits -- N 1 .. 12, D 3 or 4, fewer than 2^19
segments, 1 .. 4096 obstacles, an obstacle stride >= 0, an inflation >= 0 and finite, radii >= 0 and finite, and the required
pointers.  Return codes only: what the accepted calls compute is the matter of test_obstacle_clearance.py."""
import numpy as np
import pytest

from mav_trajectory_generation_amd import _lib as L

OK, INVALID = 0, -1
B, K = 3, 4                      # of every case that does not vary them

# (id, N, K, D, batch, ts_b, ts_k, expected)
SHAPE_CASES = [
    ("n_0", 0, K, 3, B, K, 1, INVALID),
    ("n_1", 1, K, 3, B, K, 1, OK),
    ("n_odd", 7, K, 3, B, K, 1, OK),
    ("n_12", 12, K, 3, B, K, 1, OK),
    ("n_13", 13, K, 3, B, K, 1, INVALID),
    ("k_0", 10, 0, 3, B, 1, 1, INVALID),
    ("k_1", 10, 1, 3, B, 1, 1, OK),
    ("d_0", 10, K, 0, B, K, 1, INVALID),
    ("d_2", 10, K, 2, B, K, 1, INVALID),
    ("d_3", 10, K, 3, B, K, 1, OK),
    ("d_4", 10, K, 4, B, K, 1, OK),
    ("d_5", 10, K, 5, B, K, 1, INVALID),
    ("batch_minus_1", 10, K, 3, -1, K, 1, INVALID),
    ("batch_0", 10, K, 3, 0, K, 1, OK),
    ("batch_1", 10, K, 3, 1, K, 1, OK),
    ("ts_b_0", 10, K, 3, B, 0, 1, INVALID),
    ("ts_k_0", 10, K, 3, B, K, 0, INVALID),
    ("ts_k_negative", 10, K, 3, B, K, -1, INVALID),
    ("rows_bk_touching", 10, K, 3, B, K * 2, 2, OK),
    ("rows_bk_overlapping", 10, K, 3, B, K * 2 - 1, 2, INVALID),
    ("rows_bk_padded", 10, K, 3, B, K * 2 + 3, 2, OK),
    ("rows_kb_touching", 10, K, 3, B, 2, B * 2, OK),
    ("rows_kb_overlapping", 10, K, 3, B, 2, B * 2 - 1, INVALID),
    ("rows_kb_padded", 10, K, 3, B, 2, B * 2 + 3, OK),
    ("soa", 10, K, 3, B, 1, B, OK),
]

# (id, n_obstacles, stride, inflation, radius of the last sphere, expected)
OBSTACLE_CASES = [
    ("m_0", 0, 0, 0.0, 1.0, INVALID),
    ("m_1", 1, 0, 0.0, 1.0, OK),
    ("m_4096", 4096, 0, 0.0, 1.0, OK),
    ("m_4097", 4097, 0, 0.0, 1.0, INVALID),
    ("stride_negative", 2, -8, 0.0, 1.0, INVALID),
    ("stride_per_trajectory", 2, 8, 0.0, 1.0, OK),
    ("stride_padded", 2, 11, 0.0, 1.0, OK),
    ("inflation_negative", 2, 0, -1e-300, 1.0, INVALID),
    ("inflation_zero", 2, 0, 0.0, 1.0, OK),
    ("inflation_nan", 2, 0, float("nan"), 1.0, INVALID),
    ("inflation_inf", 2, 0, float("inf"), 1.0, INVALID),
    ("radius_zero", 2, 0, 0.0, 0.0, OK),
    ("radius_negative", 2, 0, 0.0, -1e-300, INVALID),
    ("radius_nan", 2, 0, 0.0, float("nan"), INVALID),
    ("radius_inf", 2, 0, 0.0, float("inf"), INVALID),
    ("radius_negative_in_the_last_set", 2, 8, 0.0, -1.0, INVALID),
]


def call(n, k, d, batch, ts_b, ts_k, n_obstacles=2, stride=0, inflation=0.0, last_radius=1.0, null=None):
    """The entry's return code on valid data of that shape (buffers sized for the accepted reading of the arguments)."""
    lib = L.load()
    nb, nk, nd, nn, nm = max(batch, 1), max(k, 1), max(d, 1), max(n, 1), max(n_obstacles, 1)
    rng = np.random.default_rng(1000 * nn + nd)
    coeffs = rng.standard_normal((nb, nk, nd, nn))
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    obstacles = np.ones(((nb - 1) * max(stride, 0) + 4 * nm,))
    obstacles[0::4], obstacles[1::4], obstacles[2::4] = 40.0 + np.arange(obstacles[0::4].size), 50.0, 60.0   # (ever further away)
    obstacles[(nb - 1) * max(stride, 0) + 4 * nm - 1] = last_radius
    feas = np.empty((nb,), dtype=np.int32)
    ptr = {"coeffs": coeffs.ctypes.data, "times": times.ctypes.data, "obstacles": obstacles.ctypes.data, "feasible": feas.ctypes.data}
    if null:
        ptr[null] = None
    return lib.mtg_check_obstacle_clearance_host(n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["obstacles"], n_obstacles, stride,
                                                 inflation, ptr["feasible"], None, None, None, None, None, None)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules(case):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    assert call(n, k, d, batch, ts_b, ts_k) == expected, case


@pytest.mark.parametrize("case", OBSTACLE_CASES, ids=[c[0] for c in OBSTACLE_CASES])
def test_obstacle_rules(case):
    name, n_obstacles, stride, inflation, last_radius, expected = case
    assert call(10, K, 3, B, K, 1, n_obstacles, stride, inflation, last_radius) == expected, case


@pytest.mark.parametrize("null", ["coeffs", "times", "obstacles", "feasible"])
def test_required_pointers(null):
    assert call(10, K, 3, B, K, 1, null=null) == INVALID


def test_segment_count_limit_of_the_failure_word():
    """2^19 segments do not fit segment << 12 | obstacle: the entry refuses them before it reads anything."""
    lib = L.load()
    one = np.ones((4,))
    out = np.empty((1,), dtype=np.int32)
    args = (3, 0, one.ctypes.data, one.ctypes.data, 1 << 19, 1, one.ctypes.data, 1, 0, 0.0, out.ctypes.data, None, None, None, None, None, None)
    assert lib.mtg_check_obstacle_clearance_host(10, 1 << 19, *args) == INVALID
    assert lib.mtg_check_obstacle_clearance_host(10, (1 << 19) - 1, *args) == OK
