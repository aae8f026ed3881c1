"""Certified distance-field check, host form (mtg_certify_distance_field_host: the lane code of csrc/mtg_certify_lane.h compiled by
g++; no device): against the independent longdouble replay (tests/certified_field_ref.py) on the committed coefficient fixtures,
soundness against the dense sampled check, answers computed by hand on exactly representable numbers, the grid's boundary, the
three limits, NaN, layouts, optional outputs and the Lipschitz helper."""
import ctypes
import functools
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import certified_field_ref as C
from test_distance_field import CASES, H, INFLATION, field_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLIDES, FREE, DEPTH, BUDGET = 0, 1, 2, 3
OUTSIDES = [0.0, np.inf]
S = 2.0 ** -36


@functools.lru_cache(maxsize=None)
def field_of(name, outside):
    coeffs, times, grid, origin = field_case(name)
    f = m.DistanceField(grid, origin, H, outside)
    return f, f.lipschitz_bound()


@functools.lru_cache(maxsize=None)
def host(name, outside, layout="aos", **limits):
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, outside)
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    return m.certify_distance_field_host(coeffs, t, f, lip, inflation=INFLATION, times_layout=layout, **limits)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- against the replay ---------------------------------------------------------------------------------------------------------

PROTOTYPE = {"n10_k8_d3_fast": (79, 21), "n5_k3_d3": (29, 11), "n12_k4_d4": (27, 33), "n7_k4_d4": (20, 20)}   # FREE, COLLIDES (outside +inf)


def compare_with_replay(name, outside, r, **limits):
    """r: a CertifiedFieldResult of numpy arrays of a whole fixture case (or of its first trajectories)."""
    coeffs, times, grid, origin = field_case(name)
    n = len(r.trajectory_result)
    _, lip = field_of(name, outside)
    e = C.replay(coeffs[:n], times[:n], grid, origin, H, outside, lip, INFLATION, **limits)
    fragile = e["fragile"]
    print(f"{name} outside={outside}: {int(fragile.sum())} of {fragile.size} segments fragile; verdicts {np.bincount(r.segment_result.ravel(), minlength=4)}; "
          f"largest frontier {int(e['largest_frontier'].max())}; nodes mean {r.segment_nodes.mean():.1f} max {int(r.segment_nodes.max())}")
    assert fragile.sum() <= 0.02 * fragile.size
    ok = ~fragile
    assert np.array_equal(r.segment_result[ok], e["result"][ok])
    assert np.array_equal(r.segment_nodes[ok], e["nodes"][ok])
    assert np.array_equal(r.segment_depth[ok], e["depth"][ok])
    assert np.array_equal(r.segment_closest_time[ok], e["closest_time"][ok])
    assert np.array_equal(r.segment_first_failing_time[ok], e["first_failing_time"][ok], equal_nan=True)
    for got, want, tol in ((r.segment_lower_bound, e["lower_bound"], e["tol_lower"]), (r.segment_sampled_clearance, e["sampled"], e["tol_sampled"])):
        fin = np.isfinite(want) & ok
        assert np.array_equal(got[~np.isfinite(want) & ok], want[~np.isfinite(want) & ok], equal_nan=True)
        err = np.abs(got[fin] - want[fin])
        print(f"  largest |got - replay| {err.max():.3e}; largest share of the bound {(err / tol[fin]).max():.3f}")
        assert (err <= tol[fin]).all()
    # the trajectory outputs follow from the segment outputs
    not_free = r.segment_result != FREE
    first = np.where(not_free.any(axis=1), not_free.argmax(axis=1), -1)
    assert np.array_equal(r.first_failing_segment, first)
    assert np.array_equal(r.trajectory_result, np.where(first < 0, FREE, np.take_along_axis(r.segment_result, np.maximum(first, 0)[:, None], 1)[:, 0]))
    assert np.array_equal(r.trajectory_lower_bound, r.segment_lower_bound.min(axis=1))
    assert np.array_equal(r.trajectory_sampled_clearance, r.segment_sampled_clearance.min(axis=1))
    return e


@pytest.mark.parametrize("outside", OUTSIDES, ids=["out0", "outinf"])
@pytest.mark.parametrize("name", CASES)
def test_host_form_against_the_replay(name, outside):
    r = host(name, outside)
    e = compare_with_replay(name, outside, r)
    assert not np.isin(r.segment_result, (DEPTH, BUDGET)).any()          # nothing undecided at depth 16
    assert e["largest_frontier"].max() <= 44
    if outside == np.inf:
        assert ((r.trajectory_result == FREE).sum(), (r.trajectory_result == COLLIDES).sum()) == PROTOTYPE[name]


def test_times_as_k_b_equal_b_k():
    assert same(host("n12_k4_d4", 0.0), host("n12_k4_d4", 0.0, layout="soa"))


# ---- soundness, independent of the rule: the sampled check at a fine spacing ------------------------------------------------------

@pytest.mark.parametrize("outside", OUTSIDES, ids=["out0", "outinf"])
@pytest.mark.parametrize("name", CASES)
def test_soundness_against_dense_samples(name, outside):
    coeffs, times, _, _ = field_case(name)
    f, _ = field_of(name, outside)
    r = host(name, outside)
    dense = m.check_distance_field_host(coeffs, times, f, float(times.min()) / 4000.0, inflation=INFLATION, max_samples=1 << 20)
    assert (dense.segment_samples >= 4001).all()
    lowest = dense.segment_clearance
    print(f"{name} outside={outside}: largest gap dense minimum - lower bound {np.nanmax(np.where(np.isfinite(lowest), lowest - r.segment_lower_bound, 0)):.3e}; "
          f"{int((lowest < r.segment_sampled_clearance).sum())} segments with a dense minimum below the sampled clearance")
    assert (r.segment_lower_bound <= lowest).all()
    assert (r.segment_lower_bound <= r.segment_sampled_clearance).all()
    failing = dense.segment_first_failing_sample >= 0
    assert not (failing & (r.segment_result == FREE)).any()
    assert (r.segment_result[failing] != FREE).all()
    assert (r.segment_lower_bound[r.segment_result == FREE] > 0.0).all()
    assert (r.segment_sampled_clearance[r.segment_result == COLLIDES] <= 0.0).all()


def position(coeffs, t):
    return np.array([np.polynomial.polynomial.polyval(t, coeffs[a]) for a in range(3)])


def clearance_at(field, points, inflation):
    """Direct lookups: one-segment trajectories with T = 0 resting at the points."""
    points = np.atleast_2d(points)
    c = np.zeros((len(points), 1, 3, 2))
    c[:, 0, :, 0] = points
    return m.check_distance_field_host(c, np.zeros((len(points), 1)), field, 0.25, inflation=inflation).segment_clearance[:, 0]


def test_a_collision_between_two_samples_of_the_sampled_check():
    """The motivating case: a fixture trajectory that the sampled check passes at dt = 0.05 and that collides."""
    name = "n10_k8_d3_fast"
    coeffs, times, _, _ = field_case(name)
    f, _ = field_of(name, np.inf)
    sampled = m.check_distance_field_host(coeffs, times, f, 0.05, inflation=INFLATION)
    r = host(name, np.inf)
    missed = np.nonzero((sampled.trajectory_feasible == 1) & (r.trajectory_result == COLLIDES))[0]
    print("passed by the sampled check at dt = 0.05, proven colliding:", missed)
    assert len(missed) >= 1
    for b in missed:
        k = r.first_failing_segment[b]
        t = r.segment_first_failing_time[b, k]
        assert 0.0 < t < times[b, k]
        assert clearance_at(f, position(coeffs[b, k], t), INFLATION)[0] <= 0.0
    assert not ((sampled.trajectory_feasible == 0) & (r.trajectory_result == FREE)).any()


# ---- answers computed by hand: an 8 x 6 x 4 grid, h = 1, origin 0, a field linear in one axis, L = its slope --------------------

NX, NY, NZ = 8, 6, 4


def linear_field(axis, outside=np.inf, slope=None):
    """d = x, 2 y or 3 z (exact in float32)."""
    iz, iy, ix = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    slope = axis + 1 if slope is None else slope
    return m.DistanceField(((ix, iy, iz)[axis] * float(slope)).astype(np.float32), (0.0, 0.0, 0.0), 1.0, outside)


def axis_line(axis, start, speed):
    """One trajectory [1][3][2]: start + speed t along `axis`, the other two coordinates at 1."""
    c = np.zeros((1, 3, 2))
    c[0, :, 0] = 1.0
    c[0, axis] = (start, speed)
    return c


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_straight_lines_by_hand(axis):
    """Clearance k (x - 1) with k = axis + 1 = L and an inflation of k, along x = 3 - v t: an axis mix-up cannot pass (8 x 6 x 4
    voxels, one slope per axis).  For a straight line the root's reach is |v| w exactly and the bound c - L |v| w is the true
    minimum over the node, less the slack of order s = 2^-36."""
    k = float(axis + 1)
    f = linear_field(axis)
    assert abs(f.lipschitz_bound() - k) <= 1e-12 and f.lipschitz_bound() >= k
    tiny = 1e-8 * k
    # far from zero: x from 3 to 2 in T = 2; the root (m = 1, x = 2.5) certifies the segment: bound 1.5 k - 0.5 k = k
    r = m.certify_distance_field_host(axis_line(axis, 3.0, -0.5), [2.0], f, k, inflation=k, min_depth=0)
    assert r.segment_result[0] == FREE and r.trajectory_result == FREE and r.first_failing_segment == -1
    assert r.segment_nodes[0] == 1 and r.segment_depth[0] == 0
    assert r.segment_sampled_clearance[0] == 1.5 * k and r.segment_closest_time[0] == 1.0 and np.isnan(r.segment_first_failing_time[0])
    assert k - tiny <= r.segment_lower_bound[0] < k and r.trajectory_lower_bound == r.segment_lower_bound[0]
    # grazing zero: x from 3 to 1 in T = 2, clearance 0 at t = T only.  The last node of every level ends at T, its bound is
    # -O(s): it is split down to max_depth = 6; its sibling is certified.  1 + 2 * 6 nodes.
    r = m.certify_distance_field_host(axis_line(axis, 3.0, -1.0), [2.0], f, k, inflation=k, min_depth=0, max_depth=6)
    assert r.segment_result[0] == DEPTH and r.trajectory_result == DEPTH and r.first_failing_segment == 0
    assert r.segment_nodes[0] == 13 and r.segment_depth[0] == 6 and np.isnan(r.segment_first_failing_time[0])
    assert r.segment_sampled_clearance[0] == k * 2.0 ** -6 and r.segment_closest_time[0] == 2.0 - 2.0 ** -6
    assert -tiny <= r.segment_lower_bound[0] < 0.0
    # crossing zero: the same line for T = 3.  Root m = 1.5: c = k / 2, bound -k: split; m = 0.75: c = 1.25 k, bound k / 2:
    # certified; m = 2.25: c = -k / 4: fails, its bound is -k / 4 - 3 k / 4 = the true minimum -k.
    r = m.certify_distance_field_host(axis_line(axis, 3.0, -1.0), [3.0], f, k, inflation=k, min_depth=0)
    assert r.segment_result[0] == COLLIDES and r.trajectory_result == COLLIDES and r.first_failing_segment == 0
    assert r.segment_nodes[0] == 3 and r.segment_depth[0] == 1 and r.segment_first_failing_time[0] == 2.25
    assert r.segment_sampled_clearance[0] == -0.25 * k and r.segment_closest_time[0] == 2.25
    assert -k - tiny <= r.segment_lower_bound[0] < -k and r.trajectory_sampled_clearance == -0.25 * k
    # the closed form of the root's bound, to the last bit: N = 2 runs zero-padded, Rh_a and the bound as the rule writes them
    r = m.certify_distance_field_host(axis_line(axis, 3.0, -0.5), [2.0], f, k, inflation=k, min_depth=0, max_depth=0)
    rh = [S * 1.0, S * 1.0, S * 1.0]
    rh[axis] = 0.5 * (1.0 + S) + S * (3.0 + 0.5)            # fma(s, A, R (1 + s)): exact here
    reach = np.sqrt(rh[2] * rh[2] + (rh[1] * rh[1] + rh[0] * rh[0])) * (1.0 + S)
    want = ((2.5 * k - k) - k * reach) - S * ((2.5 * k + k) + 2.0 * k / 1.0)
    assert abs(r.segment_lower_bound[0] - want) <= 4.0 * 2.0 ** -53 * k


def graze_batch():
    """(coeffs [3][2][3][2], times [3][2], field d = x, L, inflation): lines along y that run a hair beside the zero level set
    x = 1 (an inflation of 1), so that whole levels survive and the frontier passes 64 nodes -- 256, 512 and 512 on the parallel
    lines -- and tilted ones that cross it, where failing, certified and surviving nodes alternate within a chunk."""
    coeffs = np.zeros((3, 2, 3, 2))
    times = np.array([[4.0, 2.0], [4.0, 3.0], [2.0, 4.0]])
    coeffs[:, :, 1, 0], coeffs[:, :, 1, 1], coeffs[:, :, 2, 0] = 0.5, 1.0, 1.0            # y from 0.5 at speed 1, z = 1
    coeffs[:, :, 0, 0] = 1.0 + np.array([[2.0 ** -6, 2.0 ** -5], [2.0 ** -7, 2.0 ** -6], [2.0 ** -8, 2.0 ** -7]])
    coeffs[0, 1, 0, 1], coeffs[1, 1, 0, 1], coeffs[2, 1, 0, 1] = -0.03, 2.0 ** -9, -0.003               # x tilted: two cross x = 1
    return coeffs, times, linear_field(0), 1.0, 1.0


def test_a_frontier_beyond_one_chunk_of_64():
    coeffs, times, f, lip, inflation = graze_batch()
    r = m.certify_distance_field_host(coeffs, times, f, lip, inflation=inflation, min_depth=0, max_frontier=1024)
    e = C.replay(coeffs, times, f.distances, f.origin, 1.0, np.inf, lip, inflation, min_depth=0, max_frontier=1024)
    print("largest frontiers", e["largest_frontier"].tolist(), "nodes", r.segment_nodes.tolist(), "verdicts", r.segment_result.tolist())
    assert (e["largest_frontier"][:, 0] > 64).all() and e["largest_frontier"].max() >= 512
    assert np.array_equal(r.segment_nodes, e["nodes"]) and np.array_equal(r.segment_result, e["result"]) and np.array_equal(r.segment_depth, e["depth"])
    # a parallel line at clearance e is certified once w (1 + s) + slack < e: w = e / 2, a full tree down to that level
    assert r.segment_result[:, 0].tolist() == [FREE] * 3 and r.segment_nodes[:, 0].tolist() == [511, 1023, 1023]
    assert r.segment_result[:, 1].tolist() == [COLLIDES, FREE, COLLIDES] and (r.segment_nodes[:, 1] > 1).all()
    # the budget: with max_frontier = 256 the 256 survivors of level 8 would need 512 places
    r = m.certify_distance_field_host(coeffs, times, f, lip, inflation=inflation, min_depth=0, max_frontier=256)
    assert r.segment_result[:, 0].tolist() == [FREE, BUDGET, BUDGET] and r.segment_nodes[:, 0].tolist() == [511, 511, 511]
    assert r.segment_depth[:, 0].tolist() == [8, 8, 8] and r.trajectory_result.tolist() == [COLLIDES, BUDGET, BUDGET]


# ---- the grid's boundary --------------------------------------------------------------------------------------------------------

def test_leaving_the_grid_and_wholly_outside():
    # x from 6 to 9, the grid ends at x = 7: free with outside = +inf; the nodes beyond the grid are bounded from the clamped
    # point x = 7, and the true minimum inside the grid is 6 at t = 0
    c = axis_line(0, 6.0, 1.0)
    r = m.certify_distance_field_host(c, [3.0], linear_field(0, np.inf), 1.0, min_depth=0)
    assert r.segment_result[0] == FREE and 0.0 < r.segment_lower_bound[0] <= 6.0 and np.isfinite(r.segment_lower_bound[0])
    # the root's sample (x = 7.5, R = 1.5) is outside and its box touches the grid: its bound is D(7, 1, 1) - L Rh = 5.5, not
    # +infinity, and certifies the segment at once
    assert r.segment_nodes[0] == 1 and r.segment_sampled_clearance[0] == np.inf and 5.5 - 1e-8 <= r.segment_lower_bound[0] < 5.5
    # with an inflation of 5 the root is not enough (bound 0.5 - ...: still certified); of 5.75 it splits: m = 0.75 (x = 6.75,
    # inside: c = 1, bound 0.25) and m = 2.25 (x = 8.25, R = 0.75: beyond reach of the grid, +infinity)
    r = m.certify_distance_field_host(c, [3.0], linear_field(0, np.inf), 1.0, inflation=5.75, min_depth=0)
    assert r.segment_result[0] == FREE and r.segment_nodes[0] == 3 and r.segment_sampled_clearance[0] == 1.0 and r.segment_closest_time[0] == 0.75
    assert 0.25 - 1e-8 <= r.segment_lower_bound[0] < 0.25
    # the same line with outside = 0: collides, first at the first evaluated sample beyond x = 7
    r = m.certify_distance_field_host(c, [3.0], linear_field(0, 0.0), 1.0, min_depth=0)
    assert r.segment_result[0] == COLLIDES and r.segment_first_failing_time[0] == 1.5 and r.segment_sampled_clearance[0] == 0.0
    assert r.segment_lower_bound[0] <= 0.0
    # wholly outside, beyond reach of the grid: only the outside branch; one node
    far = axis_line(0, 10.0, 1.0)
    r = m.certify_distance_field_host(far, [2.0], linear_field(0, 5.0), 1.0, inflation=1.0, min_depth=0)
    assert r.segment_result[0] == FREE and r.segment_nodes[0] == 1 and r.segment_lower_bound[0] == 4.0 == r.segment_sampled_clearance[0]
    r = m.certify_distance_field_host(far, [2.0], linear_field(0, 1.0), 1.0, inflation=1.0, min_depth=0, max_depth=5)
    assert r.segment_result[0] == COLLIDES and r.segment_nodes[0] == 1 and r.segment_lower_bound[0] == 0.0 and r.segment_first_failing_time[0] == 1.0
    r = m.certify_distance_field_host(far, [2.0], linear_field(0, -np.inf), 1.0, min_depth=0)
    assert r.segment_result[0] == COLLIDES and r.segment_lower_bound[0] == -np.inf


# ---- the three limits -----------------------------------------------------------------------------------------------------------

DEPTH3 = {"n10_k8_d3_fast": 88, "n5_k3_d3": 53, "n12_k4_d4": 48, "n7_k4_d4": 68}       # code 2 at max_depth = 3, first 25 trajectories
FRONTIER4 = {"n10_k8_d3_fast": 63, "n5_k3_d3": 33, "n12_k4_d4": 36, "n7_k4_d4": 57}    # code 3 at max_frontier = 4


def first25(name, **limits):
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, np.inf)
    return m.certify_distance_field_host(coeffs[:25], times[:25], f, lip, inflation=INFLATION, **limits)


@pytest.mark.parametrize("name", CASES)
def test_depth_limit_and_budget(name):
    full = first25(name)
    r = first25(name, min_depth=0, max_depth=3)
    compare_with_replay(name, np.inf, r, min_depth=0, max_depth=3)
    assert (r.segment_result == DEPTH).sum() == DEPTH3[name] and not (r.segment_result == BUDGET).any() and r.segment_depth.max() == 3
    assert (r.segment_lower_bound[r.segment_result == DEPTH] <= 0.0).all()
    assert (r.segment_result[full.segment_result == FREE] != COLLIDES).all()
    assert (r.segment_lower_bound <= full.segment_sampled_clearance).all()
    r = first25(name, min_depth=0, max_frontier=4)
    compare_with_replay(name, np.inf, r, min_depth=0, max_frontier=4)
    assert (r.segment_result == BUDGET).sum() == FRONTIER4[name]
    assert (r.segment_lower_bound[r.segment_result == BUDGET] == -np.inf).all()
    assert np.isfinite(r.segment_lower_bound[r.segment_result == FREE]).all()
    stopped = r.segment_result == BUDGET
    assert (r.segment_nodes[stopped] <= full.segment_nodes[stopped] + 15).all() and (r.trajectory_lower_bound[stopped.any(axis=1)] == -np.inf).all()


@pytest.mark.parametrize("name", CASES)
def test_min_depth_does_not_change_the_verdicts(name):
    a, b, c = (host(name, np.inf, min_depth=d) for d in (0, 4, 6))
    assert not np.isin(np.stack([a.segment_result, b.segment_result, c.segment_result]), (DEPTH, BUDGET)).any()
    assert np.array_equal(a.segment_result, b.segment_result) and np.array_equal(b.segment_result, c.segment_result)
    assert np.array_equal(a.trajectory_result, c.trajectory_result) and (c.segment_nodes >= 64).all() and (a.segment_depth <= 16).all()


def test_the_limits_at_their_extremes():
    f, c = linear_field(0), axis_line(0, 3.0, -1.0)
    r = m.certify_distance_field_host(c, [2.0], f, 1.0, inflation=1.0, min_depth=0, max_depth=24, max_frontier=2)      # grazing: 1 + 2 * 24
    assert r.segment_result[0] == DEPTH and r.segment_nodes[0] == 49 and r.segment_depth[0] == 24
    assert r.segment_closest_time[0] == 2.0 - 2.0 ** -24
    r = m.certify_distance_field_host(c, [2.0], f, 1.0, inflation=1.0, min_depth=10, max_depth=10, max_frontier=1024)
    assert r.segment_result[0] == DEPTH and r.segment_nodes[0] == 1024 and r.segment_depth[0] == 10
    # a field that certifies nothing (L far too large for the clearance): every node splits, the budget stops the third level
    r = m.certify_distance_field_host(c, [1.0], f, 1e6, inflation=1.0, min_depth=0, max_frontier=2)
    assert r.segment_result[0] == BUDGET and r.segment_nodes[0] == 3 and r.segment_depth[0] == 1 and r.segment_lower_bound[0] == -np.inf
    assert r.segment_sampled_clearance[0] == 1.25 and r.segment_closest_time[0] == 0.75
    r = m.certify_distance_field_host(c, [1.0], f, 1e6, inflation=1.0, min_depth=10, max_frontier=1024)
    assert r.segment_result[0] == BUDGET and r.segment_nodes[0] == 1024 and r.segment_depth[0] == 10


@pytest.mark.parametrize("T", [0.0, -0.5, np.nan])
def test_segment_times_that_are_not_positive(T):
    """One node at m = 0 with w = 0 (a NaN T: m = T, everything NaN, which fails)."""
    r = m.certify_distance_field_host(axis_line(0, 3.0, -1.0), [T], linear_field(0), 1.0, inflation=1.0)
    assert r.segment_nodes[0] == 1 and r.segment_depth[0] == 0
    if T != T:
        assert r.segment_result[0] == COLLIDES and np.isnan(r.segment_sampled_clearance[0]) and np.isnan(r.segment_lower_bound[0])
        assert np.isnan(r.segment_closest_time[0]) and np.isnan(r.segment_first_failing_time[0]) and np.isnan(r.trajectory_lower_bound)
    else:
        assert r.segment_result[0] == FREE and r.segment_sampled_clearance[0] == 2.0 and r.segment_closest_time[0] == 0.0
        assert 2.0 - 1e-8 <= r.segment_lower_bound[0] < 2.0
    # the lone node is terminal whatever its bound: resting exactly on the zero level set it fails, a hair above it is undecided
    r = m.certify_distance_field_host(axis_line(0, 1.0, 0.0), [0.0], linear_field(0), 1.0, inflation=1.0)
    assert r.segment_result[0] == COLLIDES and r.segment_first_failing_time[0] == 0.0
    r = m.certify_distance_field_host(axis_line(0, 1.0 + 2.0 ** -40, 0.0), [0.0], linear_field(0), 1.0, inflation=1.0)
    assert r.segment_result[0] == DEPTH and r.segment_sampled_clearance[0] == 2.0 ** -40 and r.segment_lower_bound[0] < 0.0


# ---- NaN, yaw, shapes -----------------------------------------------------------------------------------------------------------

def test_nan_voxels():
    # under a sample: COLLIDES, and the NaN wins both bounds
    g = linear_field(0)
    g.distances[1, 1, 3] = np.nan                                              # centre (3, 1, 1)
    r = m.certify_distance_field_host(axis_line(0, 5.0, -1.0), [4.0], g, 1.0, min_depth=0)     # the root samples (3, 1, 1)
    assert r.segment_result[0] == COLLIDES and np.isnan(r.segment_sampled_clearance[0]) and np.isnan(r.segment_lower_bound[0])
    assert r.segment_first_failing_time[0] == 2.0 and r.segment_closest_time[0] == 2.0 and np.isnan(r.trajectory_sampled_clearance)
    # only in reach: outside = +inf and one node (max_depth 0) whose sample is outside the grid: x from 1 to 5, y from 0.5 to
    # -3.5; m = 2 samples (3, -1.5, 1) (+inf, passes).  Its box (reach 2 along x and y) touches the grid and its clamped point
    # (3, 0, 1) is the NaN voxel: the bound is NaN, the node is not certified and the NaN wins the lower bound
    g = linear_field(0)
    g.distances[1, 0, 3] = np.nan
    c = np.zeros((1, 3, 2))
    c[0, :, 0], c[0, :, 1] = (1.0, 0.5, 1.0), (1.0, -1.0, 0.0)
    r = m.certify_distance_field_host(c, [4.0], g, 1.0, min_depth=0, max_depth=0)
    assert r.segment_result[0] == DEPTH and np.isnan(r.segment_lower_bound[0]) and r.segment_sampled_clearance[0] == np.inf
    assert np.isnan(r.trajectory_lower_bound) and np.isnan(r.segment_first_failing_time[0]) and r.segment_nodes[0] == 1
    clean = m.certify_distance_field_host(c, [4.0], linear_field(0), 1.0, min_depth=0, max_depth=0)      # 3 - sqrt(8) > 0
    assert clean.segment_result[0] == FREE and 0.17 < clean.segment_lower_bound[0] < 0.18


def test_nan_coefficients_and_the_yaw_dimension():
    name = "n12_k4_d4"
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, np.inf)
    clean = host(name, np.inf)
    dirty = coeffs.copy()
    dirty[:, :, 3] = np.nan                                                    # yaw is never read
    assert same(m.certify_distance_field_host(dirty, times, f, lip, inflation=INFLATION), clean)
    dirty = coeffs.copy()
    dirty[7, 2, 1, 3] = np.nan
    d = m.certify_distance_field_host(dirty, times, f, lip, inflation=INFLATION)
    assert d.segment_result[7, 2] == COLLIDES and np.isnan(d.segment_lower_bound[7, 2]) and np.isnan(d.segment_sampled_clearance[7, 2])
    assert d.segment_nodes[7, 2] == 16 and d.segment_first_failing_time[7, 2] == times[7, 2] / 32.0 and np.isnan(d.trajectory_lower_bound[7])
    others = np.ones(clean.segment_result.shape, bool)
    others[7, 2] = False
    assert np.array_equal(d.segment_lower_bound[others], clean.segment_lower_bound[others])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 9, 11])
def test_odd_and_small_n_equal_the_padded_even_form(n):
    from distance_field_ref import spheres_field
    rng = np.random.default_rng(n)
    coeffs = rng.uniform(-1.0, 1.0, (6, 3, 3, n))
    coeffs[..., 0] += 4.0
    times = rng.uniform(0.3, 2.0, (6, 3))
    f = m.DistanceField(spheres_field((0.0, 0.0, 0.0), (33, 30, 29), 0.25, [[4.0, 4.0, 4.0]], [0.8]), (0.0, 0.0, 0.0), 0.25, 0.5)
    even = max(4, n + (n & 1))
    padded = np.zeros((6, 3, 3, even))
    padded[..., :n] = coeffs
    a, b = (m.certify_distance_field_host(c, times, f, 1.6, inflation=0.1) for c in (coeffs, padded))
    assert same(a, b) and set(np.unique(a.segment_result)) <= {COLLIDES, FREE}


def test_a_single_trajectory_comes_without_the_batch_axis():
    name = "n7_k4_d4"
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, 0.0)
    full = host(name, 0.0)
    one = m.certify_distance_field_host(coeffs[5], times[5], f, lip, inflation=INFLATION)
    assert one.segment_lower_bound.shape == (4,) and one.trajectory_result.shape == () and one.lipschitz == lip
    assert all(np.array_equal(a, b[5], equal_nan=True) for a, b in zip(one[:11], full[:11]))
    assert m.certify_distance_field_host(coeffs[5], times[5], f, inflation=INFLATION).lipschitz == lip       # None: computed


# ---- optional outputs, guard words ----------------------------------------------------------------------------------------------

def raw_host_call(coeffs, times, field_c, lip, limits, inflation, outs):
    lib = L.load()
    b, k, d, n = coeffs.shape
    return lib.mtg_certify_distance_field_host(n, k, d, b, coeffs.ctypes.data, times.ctypes.data, k, 1, ctypes.byref(field_c), lip, *limits,
                                               inflation, *[None if o is None else o.ctypes.data for o in outs])


def output_shapes(b, k):
    i, f = np.int32, np.float64
    return [((b,), i), ((b,), i), ((b, k), i), ((b, k), f), ((b, k), f), ((b, k), f), ((b, k), f), ((b, k), i), ((b, k), i), ((b,), f), ((b,), f)]


def test_optional_outputs_in_every_combination_and_guard_words():
    from test_distance_field import field_struct
    coeffs, times, grid, origin = field_case("n5_k3_d3")
    coeffs, times = np.ascontiguousarray(coeffs[:5]), np.ascontiguousarray(times[:5])
    fc = field_struct(grid, origin, H)
    _, lip = field_of("n5_k3_d3", 0.0)
    b, k = times.shape
    GUARD, limits = 3, (4, 16, 1024)

    def buffers():
        return [np.full(int(np.prod(s)) + 2 * GUARD, -77, dtype=dt) for s, dt in output_shapes(b, k)]
    full = buffers()
    assert raw_host_call(coeffs, times, fc, lip, limits, INFLATION, [a[GUARD:] for a in full]) == 0
    for a in full:                                    # written in full, and not beyond
        assert (a[:GUARD] == -77).all() and (a[-GUARD:] == -77).all() and not (a[GUARD:-GUARD] == -77).any()
    want = m.certify_distance_field_host(coeffs, times, m.DistanceField(grid, origin, H), lip, inflation=INFLATION)
    for a, w in zip(full, want[:11]):
        assert np.array_equal(a[GUARD:-GUARD].reshape(w.shape), w, equal_nan=True)
    for present in itertools.product([False, True], repeat=10):
        some = buffers()
        outs = [some[0][GUARD:]] + [some[i + 1][GUARD:] if p else None for i, p in enumerate(present)]
        assert raw_host_call(coeffs, times, fc, lip, limits, INFLATION, outs) == 0
        for i, (a, ref) in enumerate(zip(some, full)):
            assert np.array_equal(a, ref, equal_nan=True) if (i == 0 or present[i - 1]) else (a == -77).all()
    assert raw_host_call(coeffs, times, fc, lip, limits, INFLATION, [None] * 11) == -1       # trajectory_result is required
    untouched = buffers()
    L.load().mtg_certify_distance_field_host(5, 3, 3, 0, coeffs.ctypes.data, times.ctypes.data, 3, 1, ctypes.byref(fc), lip, *limits,
                                             INFLATION, *[a.ctypes.data for a in untouched])              # batch = 0
    assert all((a == -77).all() for a in untouched)


# ---- the Lipschitz helper -------------------------------------------------------------------------------------------------------

def test_lipschitz_bound_against_brute_force():
    rng = np.random.default_rng(7)
    grid = rng.uniform(-2.0, 2.0, (4, 5, 6)).astype(np.float32)
    h = 0.3
    worst = 0.0
    g = grid.astype(np.float64)
    for z in range(3):
        for y in range(4):
            for x in range(5):
                cell = g[z:z + 2, y:y + 2, x:x + 2]
                gx, gy, gz = np.abs(cell[:, :, 1] - cell[:, :, 0]).max(), np.abs(cell[:, 1, :] - cell[:, 0, :]).max(), np.abs(cell[1] - cell[0]).max()
                worst = max(worst, np.sqrt(gx * gx + gy * gy + gz * gz) / h)
    got = m.DistanceField(grid, (0.0, 0.0, 0.0), h).lipschitz_bound()
    assert worst <= got <= worst * (1.0 + 1e-14)
    # it is a Lipschitz constant of the interpolant: random pairs of points inside the grid
    f = m.DistanceField(grid, (0.0, 0.0, 0.0), h, 0.0)
    a, b = (rng.uniform(0.0, 1.0, (4000, 3)) * (np.array([5, 4, 3]) * h) for _ in range(2))
    b = a + (b - a) * rng.uniform(0.0, 0.2, (4000, 1))
    da, db = clearance_at(f, a, 0.0), clearance_at(f, b, 0.0)
    assert (np.abs(da - db) <= got * np.linalg.norm(a - b, axis=1) * (1.0 + 1e-9)).all()
    for name in CASES:
        assert 1.5 < field_of(name, 0.0)[1] < 1.65


def test_lipschitz_bound_with_a_non_finite_voxel_is_refused():
    for bad in (np.nan, np.inf):
        grid = np.ones((3, 4, 5), dtype=np.float32)
        grid[1, 2, 3] = bad
        f = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5)
        assert not np.isfinite(f.lipschitz_bound())
        with pytest.raises(m.MtgError):
            m.certify_distance_field_host(np.zeros((1, 3, 4)), [1.0], f)
    lib, out = L.load(), ctypes.c_double(-5.0)
    grid = np.ones((1, 4, 5), dtype=np.float32)
    fc = L.DistanceFieldC(grid.ctypes.data, 5, 4, 1, (ctypes.c_double * 3)(0.0, 0.0, 0.0), 0.5, 0.0, 1)
    assert lib.mtg_distance_field_lipschitz_host(ctypes.byref(fc), ctypes.byref(out)) == -1 and out.value == -5.0     # nz = 1
    assert lib.mtg_distance_field_lipschitz_host(None, ctypes.byref(out)) == -1
    with pytest.raises(m.MtgError):
        m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5).lipschitz_bound()


# ---- exports, binding, build remarks -----------------------------------------------------------------------------------------

def test_exports_binding_and_signature():
    from mav_trajectory_generation_amd import segment_checks as sc
    for n in ("CertifiedFieldResult", "certify_distance_field", "certify_distance_field_host"):
        assert getattr(m, n) is getattr(sc, n)
        assert n not in dir(m)                       # resolved on use, not bound: dir() of the package is pinned elsewhere
    assert callable(m.DistanceField.lipschitz_bound)
    assert str(inspect.signature(m.certify_distance_field)) == (
        "(ctx: \"'Context'\", coeffs, times, field: 'DistanceField', lipschitz: 'Optional[float]' = None, inflation: 'float' = 0.0, "
        "min_depth: 'int' = 4, max_depth: 'int' = 16, max_frontier: 'int' = 1024, times_layout: 'str' = 'aos', "
        "want_segments: 'bool' = True) -> 'CertifiedFieldResult'")
    assert list(inspect.signature(m.certify_distance_field_host).parameters) == ["coeffs", "times", "field", "lipschitz", "inflation", "min_depth",
                                                                                "max_depth", "max_frontier", "times_layout"]
    assert m.CertifiedFieldResult._fields == ("trajectory_result", "first_failing_segment", "segment_result", "segment_lower_bound",
                                              "segment_sampled_clearance", "segment_closest_time", "segment_first_failing_time", "segment_nodes",
                                              "segment_depth", "trajectory_lower_bound", "trajectory_sampled_clearance", "lipschitz")
    header = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for fn, n_args in (("mtg_certify_distance_field", 26), ("mtg_certify_distance_field_host", 25), ("mtg_distance_field_lipschitz_host", 2)):
        decl = re.search(r"int %s\(([^;]*)\);" % fn, header).group(1)
        assert len(decl.split(",")) == n_args == len(L.EXPORTS[fn][1])
        assert hasattr(L.load(), fn)
    codes = re.search(r"enum \{ MTG_FIELD_COLLIDES = 0, MTG_FIELD_FREE = 1, MTG_FIELD_UNDECIDED_DEPTH = 2, MTG_FIELD_UNDECIDED_BUDGET = 3 \};", header)
    assert codes


def test_no_instantiation_uses_scratch():
    """Over the build's resource remarks (MTG_BUILD_REMARKS=<dir> at build time), when the build was made with them: the five
    segment kernels (N = 4 .. 12), the init and the decode kernel; 8 KB of LDS per workgroup."""
    remarks = os.environ.get("MTG_BUILD_REMARKS")
    log = os.path.join(remarks, "mtg_certify.log") if remarks else None
    if not log or not os.path.exists(log):
        pytest.skip("the build was not made with MTG_BUILD_REMARKS")
    text = open(log).read()
    names = re.findall(r"Function Name: (\S*certify\S*)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    assert len(names) >= 7 and len(scratch) >= len(names)
    assert max(scratch) == 0, list(zip(names, scratch))
    assert max(lds) == 8192
