"""Keep-out zone check, host form (mtg_check_keep_out_zones_host: the lane code of csrc/mtg_keepout_lane.h compiled by g++; no
device): against the reference's own root finders and evaluation (tests/golden/reference_keep_out_*.npz,
make_reference_keep_out_golden.py), an independent longdouble reference (tests/keep_out_ref.py), independence of pruning,
padding and list order, answers computed by hand, layouts and edge cases."""
import glob
import os
import re

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import keep_out_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("n10_k2_d3", "n10_k8_d3_fast", "n12_k1_d4", "n12_k4_d4", "n5_k3_d3", "n7_k4_d4")


def load_case(name):
    """(coeffs, times, the keep-out golden file): the inputs are the input-feasibility and half-plane fixtures', read from there."""
    z = np.load(os.path.join(GOLDEN, f"reference_keep_out_{name}.npz"))
    hp = np.load(os.path.join(GOLDEN, f"reference_half_plane_{name}.npz"))
    src = hp if "coeffs" in hp.files else np.load(os.path.join(GOLDEN, f"reference_feasibility_{name}.npz"))
    return src["coeffs"], src["times"], z


def fixture_scale(z, s):
    """[B][M]: max_j |offset_j| + inflation + the REFERENCE's max ||p|| over the trajectory's segments."""
    return np.abs(z[f"{s}/zones"][..., 3]).max(axis=-1) + float(z[f"{s}/inflation"]) + z["max_position"][:, None]


def check_against_fixture(name, run):
    """run(coeffs, times, zones, inflation) -> KeepOutResult of numpy arrays.  Returns the worst ref - got."""
    coeffs, times, z = load_case(name)
    worst_low = 0.0
    for s in z["zone_sets"]:
        zones, inflation, robust = z[f"{s}/zones"], float(z[f"{s}/inflation"]), z[f"{s}/robust"]
        assert robust.all(), (name, s)   # the cap on non-robust trajectories is 0
        r = run(coeffs, times, zones, inflation)
        assert np.array_equal(r.trajectory_feasible[robust], z[f"{s}/trajectory_feasible"][robust]), s
        assert np.array_equal(r.first_failing_segment[robust], z[f"{s}/first_failing_segment"][robust]), s
        assert np.array_equal(r.first_failing_zone[robust], z[f"{s}/first_failing_zone"][robust]), s
        assert np.array_equal(~(r.segment_clearance > 0.0), ~z[f"{s}/segment_feasible"]), s
        scale = fixture_scale(z, s).max(axis=1)[:, None]                        # [B][1]: the widest of the trajectory's zones
        diff = r.segment_clearance - z[f"{s}/segment_clearance"]                # got - ref
        print(f"{name}/{s}: got - ref in [{diff.min():.3e}, {diff.max():.3e}], shares of the bounds "
              f"{(diff / (1e-9 * np.maximum(1.0, scale))).max():.2e} / {(-diff / (1e-6 * scale)).max():.2e}")
        # the reference's candidates are values of the same function: its minimum can only be too large
        assert (diff <= 1e-9 * np.maximum(1.0, scale)).all(), (s, diff.max())
        assert (-diff <= 1e-6 * scale).all(), (s, diff.min())
        worst_low = max(worst_low, float((-diff).max()))
        # the nearest zone is the reference's wherever its runner-up is further away than both margins
        pair = np.sort(z[f"{s}/clearance"], axis=2)
        clear_cut = (pair.shape[2] == 1) | (pair[:, :, min(1, pair.shape[2] - 1)] - pair[:, :, 0] > 2e-6 * scale)
        assert np.array_equal(r.segment_nearest_zone[clear_cut], z[f"{s}/segment_nearest_zone"][clear_cut]), s
        assert np.array_equal(r.trajectory_clearance, r.segment_clearance.min(axis=1))
    return worst_low


def test_golden_files_are_complete():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "reference_keep_out_*.npz"))) == sorted(
        f"reference_keep_out_{c}.npz" for c in CASES)
    rng = np.random.default_rng(2026)
    centres, sizes = rng.uniform(-8.0, 8.0, (16, 3)), rng.uniform(0.5, 2.5, (16, 3))
    for name in CASES:
        _, _, z = load_case(name)
        sets = list(z["zone_sets"])
        assert sets[:3] == ["z16", "z1", "z16_inflated"] and ("per_trajectory" in sets) == (name == "n10_k2_d3")
        # the axis-aligned half of z16 is what the helper makes of the seeded centres and sizes, bit for bit
        assert np.array_equal(z["z16/zones"][0::2], m.keep_out_boxes(centres[0::2], sizes[0::2]))
        assert z["z16/zones"].shape == (16, 6, 4) and np.abs((z["z16/zones"][..., :3] ** 2).sum(axis=-1) - 1.0).max() <= 1e-14
        assert np.array_equal(z["z1/zones"], z["z16/zones"][:1]) and float(z["z16_inflated/inflation"]) == 0.3
        for s in sets:
            assert z[f"{s}/robust"].all(), (name, s)
    feasible = {c: int(load_case(c)[2]["z16/trajectory_feasible"].sum()) for c in CASES[:4]}
    assert feasible == {"n10_k2_d3": 83, "n10_k8_d3_fast": 40, "n12_k1_d4": 167, "n12_k4_d4": 26}
    late = {c: int((load_case(c)[2]["z16/first_failing_segment"] > 0).sum()) for c in CASES[:4]}
    assert late == {"n10_k2_d3": 23, "n10_k8_d3_fast": 38, "n12_k1_d4": 0, "n12_k4_d4": 25}


@pytest.mark.parametrize("name", CASES)
def test_host_form_against_the_reference(name):
    """The reference's minimum can only be too large (a candidate it misses).  The measured worst ref - got over the six cases
    is in DESIGN.md section 4.13."""
    worst = check_against_fixture(name, lambda c, t, z, infl: m.check_keep_out_zones_host(c, t, z, inflation=infl))
    print(f"{name}: worst ref - got {worst:.3e}")


def compare_with_independent_reference(n, d, family, r):
    z = R.reference(n, d, family)
    ref = z["pair"].min(axis=2)
    bound = 1e-9 * np.maximum(1.0, z["scale"].max(axis=1))[:, None]
    err = np.abs(r.segment_clearance.astype(R.LD) - ref).astype(np.float64)
    print(f"n{n} d{d} {family}: largest |got - ref| {err.max():.3e}, largest share of the bound {(err / bound).max():.2e}")
    assert (err <= bound).all(), (n, d, family, float(err.max()), float((err / bound).max()))
    ref64 = ref.astype(np.float64)
    assert np.array_equal(r.trajectory_feasible, (ref64 > 0.0).all(axis=1).astype(np.int32))   # (no clearance within the bound of 0: below)
    assert (np.abs(ref64) > 10.0 * bound).all()
    fails = ~(z["pair"].astype(np.float64) > 0.0)
    seg_fail = fails.any(axis=2)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1)
    assert np.array_equal(r.first_failing_segment, fseg)
    assert np.array_equal(r.first_failing_zone, [-1 if k < 0 else int(fails[b, k].argmax()) for b, k in enumerate(fseg)])
    # the nearest zone and the closest time, wherever the runner-up is further away than the bound
    order = np.sort(z["pair"].astype(np.float64), axis=2)
    clear_cut = order[:, :, 1] - order[:, :, 0] > 10.0 * bound
    nearest = z["pair"].argmin(axis=2)
    assert np.array_equal(r.segment_nearest_zone[clear_cut], nearest[clear_cut])
    # the time: the envelope at the reported time is the reported clearance
    for b in range(R.B):
        for k in range(R.K):
            zone = z["zones"][r.segment_nearest_zone[b, k]]
            assert 0.0 <= r.segment_closest_time[b, k] <= z["times"][b, k]
            at = float(R.envelope(z["coeffs"][b, k], zone, [r.segment_closest_time[b, k]])[0])
            assert abs(at - r.segment_clearance[b, k]) <= bound[b, 0]
    return float((err / bound).max())


@pytest.mark.parametrize("n,d,family", R.CASES, ids=[f"n{n}_d{d}_{f}" for n, d, f in R.CASES])
def test_host_form_against_the_independent_reference(n, d, family):
    """Tolerance 1e-9 max(1, scale), the sphere and per-axis checks' own.  Measured worst share of it: DESIGN.md section 4.13."""
    z = R.reference(n, d, family)
    r = m.check_keep_out_zones_host(z["coeffs"], z["times"], z["zones"])
    compare_with_independent_reference(n, d, family, r)
    half = -0.5 * (z["zones"][:, 0::2, 3] + z["zones"][:, 1::2, 3])                            # [M][3] half sizes: the offsets of a face pair
    if family == "waypoint":      # the start of segment (s, s mod K) is the centre of box s
        for s in range(R.M):
            assert r.segment_clearance[s, s % R.K] <= -half[s].min() * (1.0 - 1e-12)
        assert not r.trajectory_feasible[:R.M].any()
    if family == "through":       # the seeded segment passes through the centre of its box
        for s, (b, k) in enumerate(z["seeded"]):
            assert r.segment_clearance[b, k] <= -half[s].min() * (1.0 - 1e-12)
    if family == "corner":
        # the seeded segment's minimum over its own box lies at a crossing of two planes, where no h_j' vanishes: without the
        # h_i - h_j candidates the answer is wrong by far more than the tolerance
        lost = np.array([float(z["no_pairs"][b, k, s] - z["pair"][b, k, s]) for s, (b, k) in enumerate(z["seeded"])])
        kinds = np.array([z["kind"][b, k, s] for s, (b, k) in enumerate(z["seeded"])])
        print(f"corner: seeded minima at a crossing {int((kinds == R.PAIR).sum())}/{R.M}, lost without the crossings up to {lost.max():.3f}")
        assert (kinds == R.PAIR).sum() >= R.M // 2 and lost.max() > 1e-2
        single = [m.check_keep_out_zones_host(z["coeffs"][b, k][None, None], z["times"][b, k][None, None], z["zones"][s])
                  for s, (b, k) in enumerate(z["seeded"])]
        for s, (b, k) in enumerate(z["seeded"]):
            assert abs(float(single[s].segment_clearance[0, 0]) - float(z["pair"][b, k, s])) <= 1e-9 * max(1.0, z["scale"][b, s])


@pytest.mark.parametrize("n,d,family", [(4, 3, "through"), (7, 4, "corner"), (10, 3, "waypoint"), (12, 4, "far"), (12, 3, "corner")])
def test_the_independent_reference_misses_nothing(n, d, family):
    """Against a 2001-point grid.  The reference is a minimum over values of the function, each in [0, T]: it is never above the
    grid minimum by more than rounding (both contain the ends; the grid's float64 Horner against longdouble power sums).  It is
    below it by no more than the grid's resolution allows: every h_j has |h_j'| <= ||p'|| (unit normals), so does their maximum,
    and the nearest grid point is at most T / (2 * 2000) away: grid - true minimum <= speed_bound * T / 4000."""
    z = R.reference(n, d, family)
    grid = R.grid_min(z["coeffs"], z["times"], z["zones"])
    ref = z["pair"].astype(np.float64)
    rounding = 1e-12 * np.maximum(1.0, z["scale"])[:, None, :]
    resolution = (R.speed_bound(z["coeffs"], z["times"]) * z["times"] / (2.0 * (R.GRID - 1)))[:, :, None]
    print(f"n{n} d{d} {family}: ref - grid in [{(ref - grid).min():.3e}, {(ref - grid).max():.3e}], resolution up to {resolution.max():.3e}")
    assert (ref <= grid + rounding).all()
    assert (ref >= grid - resolution - rounding).all()


# ---- answers computed by hand ---------------------------------------------------------------------------------------------------

UNIT_BOX = dict(center=[0.0, 0.0, 0.0], size=[1.0, 1.0, 1.0])


def line(a, v, n=4):
    """One segment p(t) = a + v t as coeffs [1][3][n]."""
    c = np.zeros((1, 3, n))
    c[0, :, 0], c[0, :, 1] = a, v
    return c


def test_straight_line_through_the_unit_box():
    """(t - 2, 0.3, 0), T = 4, through the unit box at the origin: inside the slab |y| <= 0.5 by 0.2 throughout, and inside the
    other two slabs by more than that while |x| <= 0.3: the clearance is -0.2 (the distance to the face y = 0.5), attained on
    a whole interval.  The planes are bounding_box_half_planes' as they stand."""
    zone = m.bounding_box_half_planes(**UNIT_BOX)
    r = m.check_keep_out_zones_host(line([-2.0, 0.3, 0.0], [1.0, 0.0, 0.0]), np.array([4.0]), zone)
    assert abs(float(r.trajectory_clearance) - (-0.2)) <= 1e-15 and int(r.trajectory_feasible) == 0
    assert int(r.first_failing_segment) == 0 and int(r.first_failing_zone) == 0 and int(r.segment_nearest_zone[0]) == 0
    assert 1.7 - 1e-12 <= float(r.segment_closest_time[0]) <= 2.3 + 1e-12
    # pushed out by 0.25: 0.25 deeper
    r = m.check_keep_out_zones_host(line([-2.0, 0.3, 0.0], [1.0, 0.0, 0.0]), np.array([4.0]), zone, inflation=0.25)
    assert abs(float(r.trajectory_clearance) - (-0.45)) <= 1e-15


def test_line_past_a_corner_of_the_unit_box():
    """The line x + y = 1.6, z = 0 ((1.6 - t, t, 0), T = 1.6) passes the edge (0.5, 0.5, z) outside the box.  h_x = x - 0.5 =
    1.1 - t falls, h_y = y - 0.5 = t - 0.5 rises, every other h is negative: the envelope's minimum is where h_x = h_y, t = 0.8,
    value 0.3 -- no h_j' vanishes anywhere.  The Euclidean distance to the edge there is 0.3 sqrt 2: the clearance is a lower
    bound of it."""
    zone = m.bounding_box_half_planes(**UNIT_BOX)
    c = line([1.6, 0.0, 0.0], [-1.0, 1.0, 0.0])
    r = m.check_keep_out_zones_host(c, np.array([1.6]), zone)
    # (a crossing's value is FIRST order in the root's error, 1e-12 T at unit speed, unlike a stationary value)
    assert abs(float(r.trajectory_clearance) - 0.3) <= 1e-11 and abs(float(r.segment_closest_time[0]) - 0.8) <= 1e-11
    assert int(r.trajectory_feasible) == 1 and int(r.first_failing_segment) == -1 and int(r.first_failing_zone) == -1
    euclid = np.linalg.norm(np.array([0.8, 0.8]) - 0.5)
    assert abs(euclid - 0.3 * np.sqrt(2.0)) <= 1e-15 and float(r.trajectory_clearance) <= euclid
    # a vehicle of radius 0.31 enters the pushed-out planes by 0.01 and fails; the Minkowski sum with that ball (0.31 < 0.3 sqrt 2)
    # would pass: the pushed-out planes are a superset of it
    r = m.check_keep_out_zones_host(c, np.array([1.6]), zone, inflation=0.31)
    assert int(r.trajectory_feasible) == 0 and abs(float(r.trajectory_clearance) + 0.01) <= 1e-11
    r = m.check_keep_out_zones_host(c, np.array([1.6]), zone, inflation=0.29)
    assert int(r.trajectory_feasible) == 1 and abs(float(r.trajectory_clearance) - 0.01) <= 1e-11


def test_segment_ending_exactly_on_a_face():
    """(t - 2.5, 0, 0) over T = 2 ends at x = -0.5, on the face: the clearance is exactly 0 at t = T, and 0 is not > 0."""
    zone = m.bounding_box_half_planes(**UNIT_BOX)
    r = m.check_keep_out_zones_host(line([-2.5, 0.0, 0.0], [1.0, 0.0, 0.0]), np.array([2.0]), zone)
    assert float(r.trajectory_clearance) == 0.0 and float(r.segment_closest_time[0]) == 2.0
    assert int(r.trajectory_feasible) == 0 and int(r.first_failing_segment) == 0 and int(r.first_failing_zone) == 0
    # ... and one that stops short of it by 2^-20 passes
    r = m.check_keep_out_zones_host(line([-2.5, 0.0, 0.0], [1.0, 0.0, 0.0]), np.array([2.0 - 2.0 ** -20]), zone)
    assert float(r.trajectory_clearance) == 2.0 ** -20 and int(r.trajectory_feasible) == 1


def test_parabola_over_a_face():
    """(t, 0, 1 + (t - 1)^2), T = 2, over the box's top face z = 0.5: the minimum of h_z = z - 0.5 is a root of h_z', t = 1,
    value 0.5, exact where the nearest point lies in a face."""
    c = np.zeros((1, 3, 5))
    c[0, 0, 0], c[0, 0, 1] = -1.0, 1.0
    c[0, 2, :3] = [2.0, -2.0, 1.0]
    r = m.check_keep_out_zones_host(c, np.array([2.0]), m.bounding_box_half_planes(**UNIT_BOX))
    assert abs(float(r.trajectory_clearance) - 0.5) <= 1e-15 and abs(float(r.segment_closest_time[0]) - 1.0) <= 1e-9


# ---- independence of pruning, order and padding ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,s", [("n10_k8_d3_fast", "z16"), ("n12_k4_d4", "z16_inflated"), ("n7_k4_d4", "z16")])
def test_results_do_not_depend_on_pruning_or_order(name, s):
    coeffs, times, z = load_case(name)
    zones, inflation = z[f"{s}/zones"], float(z[f"{s}/inflation"])
    r = m.check_keep_out_zones_host(coeffs, times, zones, inflation=inflation)
    singles = [m.check_keep_out_zones_host(coeffs, times, zones[h:h + 1], inflation=inflation) for h in range(len(zones))]   # never pruned
    pair = np.stack([q.segment_clearance for q in singles], axis=2)                                   # [B][K][M]
    assert np.array_equal(r.segment_clearance, pair.min(axis=2))
    assert np.array_equal(r.segment_nearest_zone, pair.argmin(axis=2))                                # (argmin: the smallest index)
    pair_time = np.stack([q.segment_closest_time for q in singles], axis=2)
    assert np.array_equal(r.segment_closest_time, np.take_along_axis(pair_time, pair.argmin(axis=2)[:, :, None], axis=2)[:, :, 0])
    fails = ~(pair > 0.0)
    seg_fail = fails.any(axis=2)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1)
    fzone = np.array([-1 if k < 0 else int(fails[b, k].argmax()) for b, k in enumerate(fseg)])
    assert np.array_equal(r.first_failing_segment, fseg) and np.array_equal(r.first_failing_zone, fzone)
    assert np.array_equal(r.trajectory_feasible, (fseg < 0).astype(np.int32))
    perm = np.random.default_rng(7).permutation(len(zones))
    q = m.check_keep_out_zones_host(coeffs, times, zones[perm], inflation=inflation)
    assert np.array_equal(q.segment_clearance, r.segment_clearance) and np.array_equal(q.trajectory_clearance, r.trajectory_clearance)
    assert np.array_equal(q.segment_closest_time, r.segment_closest_time)
    assert np.array_equal(perm[q.segment_nearest_zone], r.segment_nearest_zone)
    assert np.array_equal(q.trajectory_feasible, r.trajectory_feasible) and np.array_equal(q.first_failing_segment, r.first_failing_segment)
    inverse = np.argsort(perm)
    failing_sets = [np.flatnonzero(fails[b, k]) if k >= 0 else None for b, k in enumerate(fseg)]
    assert [int(v) for v in q.first_failing_zone] == [-1 if f is None else int(inverse[f].min()) for f in failing_sets]


def test_ties_and_duplicates_go_to_the_smallest_index():
    coeffs, times, z = load_case("n10_k2_d3")
    zones = z["z16/zones"]
    doubled = np.concatenate([zones[5:9], zones[:8], zones[5:9]])      # every one of 5 .. 8 three times
    r = m.check_keep_out_zones_host(coeffs, times, doubled)
    first = {5: 0, 6: 1, 7: 2, 8: 3, 0: 4, 1: 5, 2: 6, 3: 7, 4: 8}
    q = m.check_keep_out_zones_host(coeffs, times, zones[:9])
    assert np.array_equal(r.segment_clearance, q.segment_clearance)
    assert np.array_equal(r.segment_nearest_zone, np.vectorize(first.get)(q.segment_nearest_zone))
    assert np.array_equal(r.first_failing_segment, q.first_failing_segment)


@pytest.mark.parametrize("repeat", [0, 3, 5])
def test_a_zone_padded_by_repeating_a_plane_is_the_same_zone(repeat):
    """P = 6 padded to 8 with two copies of one plane (the first, a middle one, the last): every output bit for bit."""
    coeffs, times, z = load_case("n10_k8_d3_fast")
    zones = z["z16/zones"]
    r = m.check_keep_out_zones_host(coeffs, times, zones, inflation=0.1)
    padded = np.concatenate([zones, zones[:, repeat:repeat + 1], zones[:, repeat:repeat + 1]], axis=1)
    assert padded.shape == (16, 8, 4)
    q = m.check_keep_out_zones_host(coeffs, times, padded, inflation=0.1)
    assert all(np.array_equal(x, y) for x, y in zip(r, q))


@pytest.mark.parametrize("planes", [1, 4, 6, 8])
def test_planes_per_zone(planes):
    """P = 1 (a half space), 4 (an infinite prism: a box without its z faces), 6 (the box), 8 (the box cut by two more planes
    through its centre region): each against the longdouble reference, and the sets nest -- fewer planes, a larger zone, no
    larger clearance."""
    z = R.reference(10, 3, "through")
    rng = np.random.default_rng(4100 + planes)
    if planes <= 6:
        zones = z["zones"][:, :planes].copy()
    else:
        extra = rng.standard_normal((R.M, 2, 3))
        extra /= np.linalg.norm(extra, axis=2, keepdims=True)
        centres = np.array([[z["coeffs"][b, k, :3, 0]] for b, k in z["seeded"]])                  # (somewhere near each box)
        zones = np.concatenate([z["zones"], np.concatenate([extra, (extra * centres).sum(axis=2, keepdims=True) - 0.2], axis=2)], axis=1)
    r = m.check_keep_out_zones_host(z["coeffs"], z["times"], zones)
    scale = R.scale_of(z["coeffs"], z["times"], zones)
    ref = np.array([[min(R.zone_clearance(z["coeffs"][b, k], z["times"][b, k], zone)[0] for zone in zones) for k in range(R.K)]
                    for b in range(0, R.B, 4)])
    bound = 1e-9 * np.maximum(1.0, scale.max(axis=1))[0::4, None]
    err = np.abs(r.segment_clearance[0::4].astype(R.LD) - ref).astype(np.float64)
    print(f"P = {planes}: largest share of the bound {(err / bound).max():.2e}")
    assert (err <= bound).all()
    box = m.check_keep_out_zones_host(z["coeffs"], z["times"], z["zones"])
    if planes <= 6:
        assert (r.segment_clearance <= box.segment_clearance).all()
    else:
        assert (r.segment_clearance >= box.segment_clearance).all()


def test_layouts_sets_and_single_zone():
    coeffs, times, z = load_case("n10_k2_d3")
    zones = z["z16/zones"]
    r = m.check_keep_out_zones_host(coeffs, times, zones)
    q = m.check_keep_out_zones_host(coeffs, np.ascontiguousarray(times.T), zones, times_layout="soa")
    assert all(np.array_equal(x, y) for x, y in zip(r, q))
    # a set per trajectory equals the shared call trajectory by trajectory
    per = z["per_trajectory/zones"]
    r = m.check_keep_out_zones_host(coeffs, times, per)
    for b in (0, 1, 77, 149):
        one = m.check_keep_out_zones_host(coeffs[b], times[b], per[b])
        assert all(np.array_equal(x[b], y) for x, y in zip(r, one))
    # one trajectory without the batch axis; a [P][4] array is one zone
    one = m.check_keep_out_zones_host(coeffs[3], times[3], zones)
    assert one.segment_clearance.shape == (2,) and np.ndim(one.trajectory_feasible) == 0
    a, b = m.check_keep_out_zones_host(coeffs, times, zones[2]), m.check_keep_out_zones_host(coeffs, times, zones[2:3])
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a.segment_nearest_zone == 0).all()
    # inflation moves every offset by the same amount, up to the rounding of that addition
    r = m.check_keep_out_zones_host(coeffs, times, zones, inflation=0.3)
    grown = zones.copy()
    grown[..., 3] -= 0.3
    q = m.check_keep_out_zones_host(coeffs, times, grown)
    assert np.abs(r.segment_clearance - q.segment_clearance).max() <= 8 * np.finfo(float).eps * 30.0
    assert np.array_equal(r.trajectory_feasible, q.trajectory_feasible) and np.array_equal(r.segment_nearest_zone, q.segment_nearest_zone)


def test_segment_time_not_positive():
    """T <= 0: no interior candidates, both ends are still evaluated."""
    coeffs, times, z = load_case("n10_k2_d3")
    coeffs, times = coeffs[:4].copy(), times[:4].copy()
    times[1, 0], times[2, 1] = 0.0, -0.5
    zones = z["z16/zones"]
    r = m.check_keep_out_zones_host(coeffs, times, zones)
    for b, k in ((1, 0), (2, 1)):
        ends = [min(float(R.envelope(coeffs[b, k], zone, [t])[0]) for zone in zones) for t in (0.0, times[b, k])]
        assert abs(r.segment_clearance[b, k] - min(ends)) <= 1e-9 and r.segment_closest_time[b, k] in (0.0, times[b, k])


def test_yaw_is_never_read_and_a_nan_coefficient_fails_and_wins():
    coeffs, times, z = load_case("n12_k4_d4")
    zones = z["z16/zones"]
    clean = m.check_keep_out_zones_host(coeffs, times, zones)
    dirty = coeffs.copy()
    dirty[:, :, 3] = np.nan
    assert all(np.array_equal(x, y) for x, y in zip(m.check_keep_out_zones_host(dirty, times, zones), clean))
    dirty = coeffs.copy()
    dirty[5, 3, 1, 4] = np.nan
    r = m.check_keep_out_zones_host(dirty, times, zones)
    assert r.trajectory_feasible[5] == 0 and r.first_failing_segment[5] == min(3, clean.first_failing_segment[5] if clean.first_failing_segment[5] >= 0 else 3)
    assert np.isnan(r.segment_clearance[5, 3]) and np.isnan(r.trajectory_clearance[5]) and r.segment_nearest_zone[5, 3] == 0
    others = np.arange(len(coeffs)) != 5
    for x, y in zip(r, clean):
        assert np.array_equal(x[others], y[others])
    assert np.array_equal(np.delete(r.segment_clearance[5], 3), np.delete(clean.segment_clearance[5], 3))
    # a NaN segment time: both ends are evaluated, the second is NaN
    t_bad = times.copy()
    t_bad[2, 1] = np.nan
    r = m.check_keep_out_zones_host(coeffs, t_bad, zones)
    assert np.isnan(r.segment_clearance[2, 1]) and r.trajectory_feasible[2] == 0


def test_outputs_are_written_in_full_and_not_beyond():
    lib = L.load()
    coeffs, times, z = load_case("n12_k4_d4")
    zones = np.ascontiguousarray(z["z16/zones"])
    bsz, k, d, n = coeffs.shape
    pad = 3
    i32 = lambda size: np.full((size + 2 * pad,), -77, dtype=np.int32)
    f64 = lambda size: np.full((size + 2 * pad,), -77.5)
    bufs = [i32(bsz), i32(bsz), i32(bsz), f64(bsz * k), i32(bsz * k), f64(bsz * k), f64(bsz)]
    ptr = lambda a: a.ctypes.data + pad * a.itemsize
    assert lib.mtg_check_keep_out_zones_host(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, k, 1, zones.ctypes.data, 16, 6, 0, 0.0,
                                             *[ptr(a) for a in bufs]) == 0
    r = m.check_keep_out_zones_host(coeffs, times, zones)
    for a, want in zip(bufs, r):
        assert (a[:pad] == a.dtype.type(-77 if a.dtype == np.int32 else -77.5)).all() and (a[-pad:] == a[:pad]).all()
        assert np.array_equal(a[pad:-pad], np.asarray(want).ravel())
    # every optional output may be absent
    feas = np.empty((bsz,), dtype=np.int32)
    assert lib.mtg_check_keep_out_zones_host(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, k, 1, zones.ctypes.data, 16, 6, 0, 0.0,
                                             feas.ctypes.data, None, None, None, None, None, None) == 0
    assert np.array_equal(feas, r.trajectory_feasible)


def test_keep_out_boxes_helper():
    centres, sizes = [[1.0, 2.0, 3.0], [-4.0, 0.5, 6.0]], [[2.0, 4.0, 6.0], [1.0, 1.0, 0.5]]
    zones = m.keep_out_boxes(centres, sizes)
    assert zones.shape == (2, 6, 4)
    for i in range(2):
        assert np.array_equal(zones[i], m.bounding_box_half_planes(centres[i], sizes[i]))
    assert zones[0].tolist() == [[1, 0, 0, 0], [-1, 0, 0, -2], [0, 1, 0, 0], [0, -1, 0, -4], [0, 0, 1, 0], [0, 0, -1, -6]]
    assert np.array_equal(m.keep_out_boxes(centres, [1.0, 2.0, 3.0])[1], m.bounding_box_half_planes(centres[1], [1.0, 2.0, 3.0]))
    assert m.keep_out_boxes(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 6, 4)


def test_package_exports_and_header_and_binding_agree():
    from mav_trajectory_generation_amd import segment_checks as sc
    for name in ("keep_out_boxes", "check_keep_out_zones", "check_keep_out_zones_host", "KeepOutResult"):
        assert getattr(m, name) is getattr(sc, name)
    from mav_trajectory_generation_amd import check_keep_out_zones  # noqa: F401
    with pytest.raises(AttributeError):
        m.no_such_name
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for name in ("mtg_check_keep_out_zones", "mtg_check_keep_out_zones_host", "mtg_keep_out_boxes"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]), name
    assert len(L.EXPORTS["mtg_check_keep_out_zones"][1]) == 21 and len(L.EXPORTS["mtg_check_keep_out_zones_host"][1]) == 20


def test_no_instantiation_uses_scratch():
    """Over the build's resource remarks (MTG_BUILD_REMARKS=<dir> at build time), when the build was made with them: the ten
    segment kernels (N = 4 .. 12, shared and per-trajectory sets) and the decode kernel."""
    remarks = os.environ.get("MTG_BUILD_REMARKS")
    log = os.path.join(remarks, "mtg_keepout.log") if remarks else None
    if not log or not os.path.exists(log):
        pytest.skip("the build was not made with MTG_BUILD_REMARKS")
    text = open(log).read()
    names = re.findall(r"Function Name: (\S*keepout\S*)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) >= 11 and len(scratch) >= len(names)
    assert max(scratch) == 0, list(zip(names, scratch))
