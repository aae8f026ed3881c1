"""Argument table of mtg_check_keep_out_zones_host and mtg_keep_out_boxes, after tests/test_obstacle_clearance_arguments.py: the
shape rules the per-segment host entries share (csrc/mtg_segment_lane.h: shape_ok) with this entry's own limits -- N 1 .. 12, D 3
or 4, fewer than 2^19 segments, 1 .. 4096 zones of 1 .. 8 planes, a zone stride >= 0, an inflation >= 0 and finite, unit normals,
finite offsets, and the required pointers.  Return codes only: what the accepted calls compute is the matter of test_keep_out.py."""
import numpy as np
import pytest

import mav_trajectory_generation_amd as m
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

# (id, n_zones, n_planes, stride, inflation, the last plane's (nx, offset), expected); every other plane is (1, 0, 0, 40 + index)
ZONE_CASES = [
    ("m_0", 0, 6, 0, 0.0, (1.0, 50.0), INVALID),
    ("m_1", 1, 6, 0, 0.0, (1.0, 50.0), OK),
    ("m_4096", 4096, 1, 0, 0.0, (1.0, 50.0), OK),
    ("m_4097", 4097, 1, 0, 0.0, (1.0, 50.0), INVALID),
    ("p_0", 2, 0, 0, 0.0, (1.0, 50.0), INVALID),
    ("p_1", 2, 1, 0, 0.0, (1.0, 50.0), OK),
    ("p_8", 2, 8, 0, 0.0, (1.0, 50.0), OK),
    ("p_9", 2, 9, 0, 0.0, (1.0, 50.0), INVALID),
    ("stride_negative", 2, 6, -48, 0.0, (1.0, 50.0), INVALID),
    ("stride_per_trajectory", 2, 6, 48, 0.0, (1.0, 50.0), OK),
    ("stride_padded", 2, 6, 53, 0.0, (1.0, 50.0), OK),
    ("inflation_negative", 2, 6, 0, -1e-300, (1.0, 50.0), INVALID),
    ("inflation_zero", 2, 6, 0, 0.0, (1.0, 50.0), OK),
    ("inflation_nan", 2, 6, 0, float("nan"), (1.0, 50.0), INVALID),
    ("inflation_inf", 2, 6, 0, float("inf"), (1.0, 50.0), INVALID),
    ("normal_negated", 2, 6, 0, 0.0, (-1.0, 50.0), OK),
    ("normal_within_1e-9", 2, 6, 0, 0.0, (1.0 + 4e-10, 50.0), OK),
    ("normal_long", 2, 6, 0, 0.0, (1.0 + 1e-9, 50.0), INVALID),
    ("normal_short", 2, 6, 0, 0.0, (1.0 - 1e-9, 50.0), INVALID),
    ("normal_zero", 2, 6, 0, 0.0, (0.0, 50.0), INVALID),
    ("normal_nan", 2, 6, 0, 0.0, (float("nan"), 50.0), INVALID),
    ("offset_nan", 2, 6, 0, 0.0, (1.0, float("nan")), INVALID),
    ("offset_inf", 2, 6, 0, 0.0, (1.0, float("inf")), INVALID),
    ("normal_long_in_the_last_set", 2, 6, 48, 0.0, (1.1, 50.0), INVALID),
]


def call(n, k, d, batch, ts_b, ts_k, n_zones=2, n_planes=6, stride=0, inflation=0.0, last=(1.0, 50.0), null=None):
    """The entry's return code on valid data of that shape (buffers sized for the accepted reading of the arguments)."""
    lib = L.load()
    nb, nk, nd, nn = max(batch, 1), max(k, 1), max(d, 1), max(n, 1)
    planes = max(n_zones, 1) * max(n_planes, 1)
    rng = np.random.default_rng(1000 * nn + nd)
    coeffs = rng.standard_normal((nb, nk, nd, nn))
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    zones = np.zeros(((nb - 1) * max(stride, 0) + 4 * planes,))
    for b in range(nb if stride > 0 else 1):
        rows = zones[b * stride:b * stride + 4 * planes].reshape(planes, 4)   # (a view; the padding between the sets is never read)
        rows[:, 0], rows[:, 3] = 1.0, 40.0 + np.arange(planes)                # x > 40: ever further away
    end = (nb - 1) * max(stride, 0) + 4 * planes
    zones[end - 4], zones[end - 1] = last
    feas = np.empty((nb,), dtype=np.int32)
    ptr = {"coeffs": coeffs.ctypes.data, "times": times.ctypes.data, "zones": zones.ctypes.data, "feasible": feas.ctypes.data}
    if null:
        ptr[null] = None
    return lib.mtg_check_keep_out_zones_host(n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["zones"], n_zones, n_planes, stride,
                                             inflation, ptr["feasible"], None, None, None, None, None, None)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules(case):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    assert call(n, k, d, batch, ts_b, ts_k) == expected, case


@pytest.mark.parametrize("case", ZONE_CASES, ids=[c[0] for c in ZONE_CASES])
def test_zone_rules(case):
    name, n_zones, n_planes, stride, inflation, last, expected = case
    assert call(10, K, 3, B, K, 1, n_zones, n_planes, stride, inflation, last) == expected, case


@pytest.mark.parametrize("null", ["coeffs", "times", "zones", "feasible"])
def test_required_pointers(null):
    assert call(10, K, 3, B, K, 1, null=null) == INVALID


def test_segment_count_limit_of_the_failure_word():
    """2^19 segments do not fit segment << 12 | zone: the entry refuses them before it reads anything."""
    lib = L.load()
    one = np.array([1.0, 0.0, 0.0, 50.0])
    out = np.empty((1,), dtype=np.int32)
    args = (3, 0, one.ctypes.data, one.ctypes.data, 1 << 19, 1, one.ctypes.data, 1, 1, 0, 0.0, out.ctypes.data, None, None, None, None, None, None)
    assert lib.mtg_check_keep_out_zones_host(10, 1 << 19, *args) == INVALID
    assert lib.mtg_check_keep_out_zones_host(10, (1 << 19) - 1, *args) == OK


# (id, n, sizes of the last box, null pointer, expected)
BOX_CASES = [
    ("n_negative", -1, (1.0, 1.0, 1.0), None, INVALID),
    ("n_0", 0, (1.0, 1.0, 1.0), None, OK),
    ("n_0_null", 0, (1.0, 1.0, 1.0), "all", OK),
    ("n_2", 2, (1.0, 1.0, 1.0), None, OK),
    ("size_tiny", 2, (1.0, 5e-324, 1.0), None, OK),
    ("size_zero", 2, (1.0, 0.0, 1.0), None, INVALID),
    ("size_negative", 2, (1.0, 1.0, -1.0), None, INVALID),
    ("size_nan", 2, (float("nan"), 1.0, 1.0), None, INVALID),
    ("size_inf", 2, (1.0, float("inf"), 1.0), None, INVALID),
    ("null_centers", 2, (1.0, 1.0, 1.0), "centers", INVALID),
    ("null_sizes", 2, (1.0, 1.0, 1.0), "sizes", INVALID),
    ("null_out", 2, (1.0, 1.0, 1.0), "out", INVALID),
]


@pytest.mark.parametrize("case", BOX_CASES, ids=[c[0] for c in BOX_CASES])
def test_box_helper_rules(case):
    name, n, last, null, expected = case
    lib = L.load()
    rows = max(n, 1)
    centers, sizes, out = np.zeros((rows, 3)), np.ones((rows, 3)), np.full((rows, 6, 4), -77.5)
    sizes[-1] = last
    ptr = {"centers": centers.ctypes.data, "sizes": sizes.ctypes.data, "out": out.ctypes.data}
    for key in ptr:
        if null in (key, "all"):
            ptr[key] = None
    assert lib.mtg_keep_out_boxes(n, ptr["centers"], ptr["sizes"], ptr["out"]) == expected
    if expected == INVALID:
        assert (out == -77.5).all()          # nothing is written before every size is known to be good


def test_python_helper_and_wrapper_refuse_bad_shapes():
    with pytest.raises(m.MtgError):
        m.keep_out_boxes([[0.0, 0.0, 0.0]], [[1.0, 0.0, 1.0]])
    with pytest.raises(m.MtgError):
        m.keep_out_boxes([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    with pytest.raises(m.MtgError):
        m.keep_out_boxes([[0.0, 0.0, 0.0]], [[1.0, 1.0]])
    coeffs, times = np.zeros((2, 3, 3, 4)), np.ones((2, 3))
    box = m.keep_out_boxes([[9.0, 9.0, 9.0]], [1.0, 1.0, 1.0])
    assert m.check_keep_out_zones_host(coeffs, times, box).trajectory_feasible.tolist() == [1, 1]
    for bad in (box[0, :, :3], box[None, None], np.zeros((3, 1, 6, 4)), box[0, 0]):
        with pytest.raises(m.MtgError):
            m.check_keep_out_zones_host(coeffs, times, bad)
    with pytest.raises(m.MtgError):
        m.check_keep_out_zones_host(coeffs, times, box, inflation=-1.0)
