"""Argument table of mtg_check_trajectory_separation_host, after tests/test_obstacle_clearance_arguments.py: the shape rules the
per-segment host entries share (csrc/mtg_segment_lane.h: shape_ok), per side, with this entry's own limits -- N 1 .. 12, D 3 or 4,
1 .. 1024 segments per side, n_pairs >= 0 with n_pairs * Ka < 2^31, a min_separation >= 0 and finite, pair indices inside their
batches, the required pointers, and the three pair-closest outputs that need the first three per-segment outputs.  Return codes
only: what the accepted calls compute is the matter of test_trajectory_separation.py.  The device entry checks its arguments
with the same two predicates (csrc/mtg_separation_lane.h: arguments_ok, outputs_ok) before it looks at its context, and returns for
n_pairs = 0 before it needs one: with a null context and no pairs its whole table runs here, without a device; with pairs, a
null context is refused after the arguments."""
import numpy as np
import pytest

from mav_trajectory_generation_amd import _lib as L

OK, INVALID = 0, -1
B, K = 3, 4                      # of every case that does not vary them

# (id, N, K, D, batch, ts_b, ts_k, expected): one side varies, the other is (10 or N, K, D, B, K, 1)
SHAPE_CASES = [
    ("n_0", 0, K, 3, B, K, 1, INVALID),
    ("n_1", 1, K, 3, B, K, 1, OK),
    ("n_odd", 7, K, 3, B, K, 1, OK),
    ("n_12", 12, K, 3, B, K, 1, OK),
    ("n_13", 13, K, 3, B, K, 1, INVALID),
    ("k_0", 10, 0, 3, B, 1, 1, INVALID),
    ("k_1", 10, 1, 3, B, 1, 1, OK),
    ("k_1024", 10, 1024, 3, B, 1024, 1, OK),
    ("k_1025", 10, 1025, 3, B, 1025, 1, INVALID),
    ("d_0", 10, K, 0, B, K, 1, INVALID),
    ("d_2", 10, K, 2, B, K, 1, INVALID),
    ("d_3", 10, K, 3, B, K, 1, OK),
    ("d_4", 10, K, 4, B, K, 1, OK),
    ("d_5", 10, K, 5, B, K, 1, INVALID),
    ("batch_minus_1", 10, K, 3, -1, K, 1, INVALID),
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

# (id, min_separation, expected)
SEPARATION_CASES = [("zero", 0.0, OK), ("positive", 2.5, OK), ("negative", -1e-300, INVALID), ("nan", float("nan"), INVALID),
                    ("inf", float("inf"), INVALID)]

# (id, pair, expected) with batches of B on both sides
PAIR_CASES = [("first", (0, 0), OK), ("last", (B - 1, B - 1), OK), ("a_negative", (-1, 0), INVALID), ("a_beyond", (B, 0), INVALID),
              ("b_negative", (0, -1), INVALID), ("b_beyond", (0, B), INVALID)]

OUTPUTS = ("feasible", "first_a", "first_b", "separation", "closest_time", "closest_a", "closest_b", "seg_separation", "seg_time", "seg_b",
           "seg_pieces")


def side(n, k, d, batch, ts_b, ts_k):
    """(K, B, coeffs, times, ts_b, ts_k, start) with buffers sized for the accepted reading of the arguments; the arrays ride along."""
    nb, nk, nd, nn = max(batch, 1), max(k, 1), max(d, 1), max(n, 1)
    coeffs = np.random.default_rng(1000 * nn + nd).standard_normal((nb, nk, nd, nn))
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    start = np.zeros((nb,))
    return [k, batch, coeffs.ctypes.data, times.ctypes.data, ts_b, ts_k, start.ctypes.data], (coeffs, times, start)


def call(n, d, a, b, n_pairs=2, pair=(0, 0), min_separation=1.0, null=(), wanted=("feasible",), entry="mtg_check_trajectory_separation_host",
         ctx=False):
    """The entry's return code; a, b: the (K, batch, ts_b, ts_k) of the two sides."""
    lib = L.load()
    sa, keep_a = side(n, a[0], d, *a[1:])
    sb, keep_b = side(n, b[0], d, *b[1:])
    pairs = np.zeros((max(n_pairs, 1), 2), dtype=np.int32)
    pairs[-1] = pair
    ka = max(a[0], 1)
    out = {name: (np.empty((max(n_pairs, 1) * (ka if name.startswith("seg_") else 1),),
                           dtype=np.float64 if name in ("separation", "closest_time", "seg_separation", "seg_time") else np.int32))
           for name in OUTPUTS}
    ptr = {name: (out[name].ctypes.data if name in wanted else None) for name in OUTPUTS}
    ptr.update(coeffs_a=sa[2], times_a=sa[3], coeffs_b=sb[2], times_b=sb[3], pairs=pairs.ctypes.data)
    for name in null:
        ptr[name] = None
    sa[2], sa[3], sb[2], sb[3] = ptr["coeffs_a"], ptr["times_a"], ptr["coeffs_b"], ptr["times_b"]
    args = [n, d] + sa + sb + [n_pairs, ptr["pairs"], min_separation] + [ptr[name] for name in OUTPUTS]
    return getattr(lib, entry)(*(([None] if ctx else []) + args))


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules_of_either_side(case, which):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    varied, plain = (k, batch, ts_b, ts_k), (K, B, K, 1)
    assert call(n, d, varied if which == "a" else plain, plain if which == "a" else varied) == expected, case


@pytest.mark.parametrize("case", SEPARATION_CASES, ids=[c[0] for c in SEPARATION_CASES])
def test_min_separation_rules(case):
    assert call(10, 3, (K, B, K, 1), (K, B, K, 1), min_separation=case[1]) == case[2], case


@pytest.mark.parametrize("case", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_pair_indices_are_verified_on_the_host(case):
    assert call(10, 3, (K, B, K, 1), (K, B, K, 1), pair=case[1]) == case[2], case


def test_pair_count_rules():
    plain = (K, B, K, 1)
    assert call(10, 3, plain, plain, n_pairs=0) == OK
    assert call(10, 3, plain, plain, n_pairs=-1) == INVALID
    assert call(10, 3, plain, plain, n_pairs=0, null=("pairs",)) == INVALID
    # n_pairs * Ka must stay below 2^31: refused before anything is read
    assert call(10, 3, (1024, 1, 1024, 1), plain, n_pairs=1 << 21, pair=(0, 0)) == INVALID
    # a batch of 0 on a side: no index is inside it
    assert call(10, 3, (K, 0, K, 1), plain) == INVALID
    assert call(10, 3, (K, 0, K, 1), plain, n_pairs=0) == OK


@pytest.mark.parametrize("null", ["coeffs_a", "times_a", "coeffs_b", "times_b", "pairs", "feasible"])
def test_required_pointers(null):
    plain = (K, B, K, 1)
    wanted = tuple(o for o in ("feasible",) if o != null)
    assert call(10, 3, plain, plain, null=(null,), wanted=wanted) == INVALID


@pytest.mark.parametrize("closest", ["closest_time", "closest_a", "closest_b"])
def test_pair_closest_outputs_need_the_segment_outputs(closest):
    plain = (K, B, K, 1)
    segs = ("seg_separation", "seg_time", "seg_b")
    assert call(10, 3, plain, plain, wanted=("feasible", closest) + segs) == OK
    assert call(10, 3, plain, plain, wanted=("feasible", closest)) == INVALID
    for missing in segs:
        assert call(10, 3, plain, plain, wanted=("feasible", closest) + tuple(s for s in segs if s != missing) + ("seg_pieces",)) == INVALID
    assert call(10, 3, plain, plain, wanted=OUTPUTS) == OK


DEVICE = dict(entry="mtg_check_trajectory_separation", ctx=True, n_pairs=0)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_device_entry_shape_rules_without_a_device(case, which):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    varied, plain = (k, batch, ts_b, ts_k), (K, B, K, 1)
    assert call(n, d, varied if which == "a" else plain, plain if which == "a" else varied, **DEVICE) == expected, case


def test_device_entry_other_rules_without_a_device():
    plain = (K, B, K, 1)
    for name, msep, expected in SEPARATION_CASES:
        assert call(10, 3, plain, plain, min_separation=msep, **DEVICE) == expected, name
    assert call(10, 3, plain, plain, **dict(DEVICE, n_pairs=-1)) == INVALID
    assert call(10, 3, (1024, 1, 1024, 1), plain, **dict(DEVICE, n_pairs=1 << 21)) == INVALID
    for null in ("coeffs_a", "times_a", "coeffs_b", "times_b", "pairs", "feasible"):
        assert call(10, 3, plain, plain, null=(null,), wanted=tuple(o for o in ("feasible",) if o != null), **DEVICE) == INVALID, null
    segs = ("seg_separation", "seg_time", "seg_b")
    for closest in ("closest_time", "closest_a", "closest_b"):
        assert call(10, 3, plain, plain, wanted=("feasible", closest) + segs, **DEVICE) == OK
        assert call(10, 3, plain, plain, wanted=("feasible", closest), **DEVICE) == INVALID
        for missing in segs:
            assert call(10, 3, plain, plain, wanted=("feasible", closest) + tuple(x for x in segs if x != missing), **DEVICE) == INVALID
    # with pairs to check, a null context is refused -- after the arguments, before anything touches a device
    assert call(10, 3, plain, plain, **dict(DEVICE, n_pairs=2)) == INVALID
    assert call(10, 3, plain, plain, wanted=OUTPUTS, **dict(DEVICE, n_pairs=2)) == INVALID
