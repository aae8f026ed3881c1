"""Sphere-obstacle clearance check, host form (mtg_check_obstacle_clearance_host: the lane code of csrc/mtg_obstacle_lane.h
compiled by g++; no device): against the reference's own candidates and evaluation
(tests/golden/reference_obstacle_clearance_*.npz, make_reference_obstacle_clearance_golden.py), an independent exact reference
(tests/obstacle_clearance_ref.py), independence of pruning and list order, known answers, layouts and edge cases."""
import glob
import os
import re

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import obstacle_clearance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("n10_k2_d3", "n10_k8_d3_fast", "n12_k1_d4", "n12_k4_d4", "n5_k3_d3", "n7_k4_d4")


def load_case(name):
    """(coeffs, times, the obstacle golden file): the inputs are the input-feasibility and half-plane fixtures', read from there."""
    z = np.load(os.path.join(GOLDEN, f"reference_obstacle_clearance_{name}.npz"))
    hp = np.load(os.path.join(GOLDEN, f"reference_half_plane_{name}.npz"))
    src = hp if "coeffs" in hp.files else np.load(os.path.join(GOLDEN, f"reference_feasibility_{name}.npz"))
    return src["coeffs"], src["times"], z


def fixture_scale(z, s):
    """[B][M]: r + inflation + ||c|| + the REFERENCE's max ||p|| over the trajectory's segments."""
    obs = z[f"{s}/obstacles"]
    return obs[..., 3] + float(z[f"{s}/inflation"]) + np.sqrt((obs[..., :3] ** 2).sum(axis=-1)) + z["max_position"][:, None]


def check_against_fixture(name, run):
    """run(coeffs, times, obstacles, inflation) -> ObstacleClearanceResult of numpy arrays.  Returns the worst ref - got."""
    coeffs, times, z = load_case(name)
    worst_low = 0.0
    for s in z["obstacle_sets"]:
        obs, inflation, robust = z[f"{s}/obstacles"], float(z[f"{s}/inflation"]), z[f"{s}/robust"]
        assert robust.all(), (name, s)   # the cap on non-robust trajectories is 0
        r = run(coeffs, times, obs, inflation)
        assert np.array_equal(r.trajectory_feasible[robust], z[f"{s}/trajectory_feasible"][robust]), s
        assert np.array_equal(r.first_failing_segment[robust], z[f"{s}/first_failing_segment"][robust]), s
        assert np.array_equal(r.first_failing_obstacle[robust], z[f"{s}/first_failing_obstacle"][robust]), s
        assert np.array_equal(~(r.segment_clearance > 0.0), ~z[f"{s}/segment_feasible"]), s
        scale = fixture_scale(z, s).max(axis=1)[:, None]                        # [B][1]: the widest of the trajectory's spheres
        diff = r.segment_clearance - z[f"{s}/segment_clearance"]                # got - ref
        print(f"{name}/{s}: got - ref in [{diff.min():.3e}, {diff.max():.3e}], shares of the bounds "
              f"{(diff / (1e-9 * np.maximum(1.0, scale))).max():.2e} / {(-diff / (1e-6 * scale)).max():.2e}")
        # the reference's candidates are values of the same function: its minimum can only be too large
        assert (diff <= 1e-9 * np.maximum(1.0, scale)).all(), (s, diff.max())
        assert (-diff <= 1e-6 * scale).all(), (s, diff.min())
        worst_low = max(worst_low, float((-diff).max()))
        # the nearest obstacle is the reference's wherever its runner-up is further away than both margins
        pair = np.sort(z[f"{s}/clearance"], axis=2)
        clear_cut = (pair.shape[2] == 1) | (pair[:, :, min(1, pair.shape[2] - 1)] - pair[:, :, 0] > 2e-6 * scale)
        assert np.array_equal(r.segment_nearest_obstacle[clear_cut], z[f"{s}/segment_nearest_obstacle"][clear_cut]), s
        assert np.array_equal(r.trajectory_clearance, r.segment_clearance.min(axis=1))
    return worst_low


def test_golden_files_are_complete():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "reference_obstacle_clearance_*.npz"))) == sorted(
        f"reference_obstacle_clearance_{c}.npz" for c in CASES)
    rng = np.random.default_rng(2024)
    centres, radii = rng.uniform(-8.0, 8.0, (16, 3)), rng.uniform(0.5, 1.5, 16)
    for name in CASES:
        _, _, z = load_case(name)
        sets = list(z["obstacle_sets"])
        assert sets[:3] == ["s16", "s1", "s16_inflated"] and ("per_trajectory" in sets) == (name == "n10_k2_d3")
        assert np.array_equal(z["s16/obstacles"], np.concatenate([centres, radii[:, None]], axis=1))
        assert np.array_equal(z["s1/obstacles"], z["s16/obstacles"][:1]) and float(z["s16_inflated/inflation"]) == 0.3
        for s in sets:
            assert z[f"{s}/robust"].all(), (name, s)
    feasible = {c: int(load_case(c)[2]["s16/trajectory_feasible"].sum()) for c in CASES[:4]}
    assert feasible == {"n10_k2_d3": 131, "n10_k8_d3_fast": 47, "n12_k1_d4": 191, "n12_k4_d4": 49}
    late = {c: int((load_case(c)[2]["s16/first_failing_segment"] > 0).sum()) for c in CASES[:4]}
    assert late == {"n10_k2_d3": 10, "n10_k8_d3_fast": 44, "n12_k1_d4": 0, "n12_k4_d4": 10}


@pytest.mark.parametrize("name", CASES)
def test_host_form_against_the_reference(name):
    """Measured worst ref - got over the six cases: 4.6e-12 (n10_k8_d3_fast; the reference's minimum at a scattered pseudo-root),
    DESIGN.md section 4.12."""
    worst = check_against_fixture(name, lambda c, t, o, infl: m.check_obstacle_clearance_host(c, t, o, inflation=infl))
    print(f"{name}: worst ref - got {worst:.3e}")


def compare_with_independent_reference(n, d, family, r):
    z = R.reference(n, d, family)
    ref = z["pair"].min(axis=2)
    bound = 1e-9 * np.maximum(1.0, z["scale"].max(axis=1))[:, None]
    err = np.abs(r.segment_clearance.astype(R.LD) - ref).astype(np.float64)
    assert (err <= bound).all(), (n, d, family, float(err.max()), float((err / bound).max()))
    ref64 = ref.astype(np.float64)
    assert np.array_equal(r.trajectory_feasible, (ref64 > 0.0).all(axis=1).astype(np.int32))   # (no clearance within the bound of 0: below)
    assert (np.abs(ref64) > 10.0 * bound).all()
    # the nearest obstacle and the closest time, wherever the runner-up is further away than the bound
    order = np.sort(z["pair"].astype(np.float64), axis=2)
    clear_cut = order[:, :, 1] - order[:, :, 0] > 10.0 * bound
    nearest = z["pair"].argmin(axis=2)
    assert np.array_equal(r.segment_nearest_obstacle[clear_cut], nearest[clear_cut])
    # the time: the distance at the reported time is the reported clearance
    for b in range(R.B):
        for k in range(R.K):
            o = z["obstacles"][r.segment_nearest_obstacle[b, k]]
            assert 0.0 <= r.segment_closest_time[b, k] <= z["times"][b, k]
            at = float(R.distance(z["coeffs"][b, k], o[:3], [r.segment_closest_time[b, k]])[0]) - o[3]
            assert abs(at - r.segment_clearance[b, k]) <= bound[b, 0]
    return float((err / bound).max())


@pytest.mark.parametrize("n,d,family", R.CASES, ids=[f"n{n}_d{d}_{f}" for n, d, f in R.CASES])
def test_host_form_against_the_independent_reference(n, d, family):
    z = R.reference(n, d, family)
    r = m.check_obstacle_clearance_host(z["coeffs"], z["times"], z["obstacles"])
    share = compare_with_independent_reference(n, d, family, r)
    print(f"n{n} d{d} {family}: largest share of the bound {share:.2e}")
    if family == "waypoint":
        for s in range(R.M):
            assert r.segment_clearance[s, s % R.K] <= -z["obstacles"][s, 3]
        assert not r.trajectory_feasible[:R.M].any()


@pytest.mark.parametrize("n,d,family", [(4, 3, "through"), (7, 4, "through"), (10, 3, "waypoint"), (12, 4, "far")])
def test_the_independent_reference_misses_nothing(n, d, family):
    z = R.reference(n, d, family)
    grid = R.grid_min(z["coeffs"], z["times"], z["obstacles"])
    bound = 1e-9 * np.maximum(1.0, z["scale"])[:, None, :]
    assert (z["pair"].astype(np.float64) <= grid + bound).all()


@pytest.mark.parametrize("name,s", [("n10_k8_d3_fast", "s16"), ("n12_k4_d4", "s16_inflated"), ("n7_k4_d4", "s16")])
def test_results_do_not_depend_on_pruning_or_order(name, s):
    coeffs, times, z = load_case(name)
    obs, inflation = z[f"{s}/obstacles"], float(z[f"{s}/inflation"])
    r = m.check_obstacle_clearance_host(coeffs, times, obs, inflation=inflation)
    singles = [m.check_obstacle_clearance_host(coeffs, times, obs[h:h + 1], inflation=inflation) for h in range(len(obs))]   # never pruned
    pair = np.stack([q.segment_clearance for q in singles], axis=2)                                   # [B][K][M]
    assert np.array_equal(r.segment_clearance, pair.min(axis=2))
    assert np.array_equal(r.segment_nearest_obstacle, pair.argmin(axis=2))                            # (argmin: the smallest index)
    pair_time = np.stack([q.segment_closest_time for q in singles], axis=2)
    assert np.array_equal(r.segment_closest_time, np.take_along_axis(pair_time, pair.argmin(axis=2)[:, :, None], axis=2)[:, :, 0])
    fails = ~(pair > 0.0)
    seg_fail = fails.any(axis=2)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1)
    fobs = np.array([-1 if k < 0 else int(fails[b, k].argmax()) for b, k in enumerate(fseg)])
    assert np.array_equal(r.first_failing_segment, fseg) and np.array_equal(r.first_failing_obstacle, fobs)
    assert np.array_equal(r.trajectory_feasible, (fseg < 0).astype(np.int32))
    perm = np.random.default_rng(7).permutation(len(obs))
    q = m.check_obstacle_clearance_host(coeffs, times, obs[perm], inflation=inflation)
    assert np.array_equal(q.segment_clearance, r.segment_clearance) and np.array_equal(q.trajectory_clearance, r.trajectory_clearance)
    assert np.array_equal(q.segment_closest_time, r.segment_closest_time)
    assert np.array_equal(perm[q.segment_nearest_obstacle], r.segment_nearest_obstacle)
    assert np.array_equal(q.trajectory_feasible, r.trajectory_feasible) and np.array_equal(q.first_failing_segment, r.first_failing_segment)
    inverse = np.argsort(perm)
    failing_sets = [np.flatnonzero(fails[b, k]) if k >= 0 else None for b, k in enumerate(fseg)]
    assert [int(v) for v in q.first_failing_obstacle] == [-1 if f is None else int(inverse[f].min()) for f in failing_sets]


def test_ties_and_duplicates_go_to_the_smallest_index():
    coeffs, times, z = load_case("n10_k2_d3")
    obs = z["s16/obstacles"]
    doubled = np.concatenate([obs[5:9], obs[:8], obs[5:9]])      # every one of 5 .. 8 three times
    r = m.check_obstacle_clearance_host(coeffs, times, doubled)
    first = {5: 0, 6: 1, 7: 2, 8: 3, 0: 4, 1: 5, 2: 6, 3: 7, 4: 8}
    q = m.check_obstacle_clearance_host(coeffs, times, obs[:9])
    assert np.array_equal(r.segment_clearance, q.segment_clearance)
    assert np.array_equal(r.segment_nearest_obstacle, np.vectorize(first.get)(q.segment_nearest_obstacle))
    assert np.array_equal(r.first_failing_segment, q.first_failing_segment)


def test_reference_scenario_curve_past_a_sphere():
    """test_feasibility.cpp:296-309: x = t, y = 0, z = t^2, T = 1, against a sphere at (0.5, 0, -1).  The squared distance
    (t - 1/2)^2 + (t^2 + 1)^2 has the derivative 4 t^3 + 6 t - 1, whose one real root t* (Cardano: u^3 + (3/2) u - 1/4 = 0)
    lies in (0, 1); the minimum distance is the value there."""
    coeffs = np.zeros((1, 3, 3))
    coeffs[0, 0, 1] = 1.0
    coeffs[0, 2, 2] = 1.0
    disc = np.sqrt((1.0 / 8.0) ** 2 + (1.0 / 2.0) ** 3)           # u = cbrt(q/2 + D) + cbrt(q/2 - D), q = 1/4, p = 3/2
    t_star = np.cbrt(1.0 / 8.0 + disc) + np.cbrt(1.0 / 8.0 - disc)
    assert abs(4.0 * t_star ** 3 + 6.0 * t_star - 1.0) <= 1e-15 and 0.0 < t_star < 1.0
    exact = np.sqrt((t_star - 0.5) ** 2 + (t_star ** 2 + 1.0) ** 2)
    for radius, inflation in ((0.25, 0.0), (0.9, 0.0), (0.9, 0.2), (1.0, 0.02)):
        r = m.check_obstacle_clearance_host(coeffs, np.array([1.0]), m.sphere_obstacles([[0.5, 0.0, -1.0]], radius), inflation=inflation)
        assert abs(float(r.trajectory_clearance) - (exact - radius - inflation)) <= 1e-12
        assert abs(float(r.segment_closest_time[0]) - t_star) <= 1e-9
        assert bool(r.trajectory_feasible) == (exact - radius - inflation > 0.0)
        assert int(r.first_failing_obstacle) == (-1 if exact - radius - inflation > 0.0 else 0)


def test_straight_line_past_a_sphere():
    """p(t) = a + v t over T = 4 past c: the perpendicular distance where its foot lies inside the segment, else the nearer end's."""
    a, v = np.array([-3.0, 1.0, 2.0]), np.array([2.0, 0.5, -1.0])
    coeffs = np.zeros((1, 3, 4))
    coeffs[0, :, 0], coeffs[0, :, 1] = a, v
    for c in ([1.0, 4.0, 1.0], [-6.0, 0.0, 2.0], [9.0, 9.0, -4.0]):
        c = np.array(c)
        foot = np.dot(c - a, v) / np.dot(v, v)
        t = min(max(foot, 0.0), 4.0)
        exact = np.linalg.norm(a + v * t - c)
        r = m.check_obstacle_clearance_host(coeffs, np.array([4.0]), m.sphere_obstacles([c], 0.5))
        assert abs(float(r.trajectory_clearance) - (exact - 0.5)) <= 1e-12 and abs(float(r.segment_closest_time[0]) - t) <= 1e-9


def test_layouts_sets_and_inflation():
    coeffs, times, z = load_case("n10_k2_d3")
    obs = z["s16/obstacles"]
    r = m.check_obstacle_clearance_host(coeffs, times, obs)
    q = m.check_obstacle_clearance_host(coeffs, np.ascontiguousarray(times.T), obs, times_layout="soa")
    assert all(np.array_equal(x, y) for x, y in zip(r, q))
    # a set per trajectory equals the shared call trajectory by trajectory
    per = z["per_trajectory/obstacles"]
    r = m.check_obstacle_clearance_host(coeffs, times, per)
    for b in (0, 1, 77, 149):
        one = m.check_obstacle_clearance_host(coeffs[b], times[b], per[b])
        assert all(np.array_equal(x[b], y) for x, y in zip(r, one))
    # one trajectory without the batch axis
    one = m.check_obstacle_clearance_host(coeffs[3], times[3], obs)
    assert one.segment_clearance.shape == (2,) and np.ndim(one.trajectory_feasible) == 0
    # inflation is the same amount on every radius, up to the rounding of that addition (a few ulps of the distance)
    r = m.check_obstacle_clearance_host(coeffs, times, obs, inflation=0.3)
    grown = obs.copy()
    grown[:, 3] += 0.3
    q = m.check_obstacle_clearance_host(coeffs, times, grown)
    assert np.abs(r.segment_clearance - q.segment_clearance).max() <= 8 * np.finfo(float).eps * 30.0
    assert np.array_equal(r.trajectory_feasible, q.trajectory_feasible) and np.array_equal(r.segment_nearest_obstacle, q.segment_nearest_obstacle)


def test_segment_time_not_positive():
    coeffs, times, z = load_case("n10_k2_d3")
    coeffs, times = coeffs[:4].copy(), times[:4].copy()
    times[1, 0], times[2, 1] = 0.0, -0.5
    obs = z["s16/obstacles"]
    r = m.check_obstacle_clearance_host(coeffs, times, obs)
    for b, k in ((1, 0), (2, 1)):
        ends = [min(float(R.distance(coeffs[b, k], o[:3], [t])[0]) - o[3] for o in obs) for t in (0.0, times[b, k])]
        assert abs(r.segment_clearance[b, k] - min(ends)) <= 1e-9 and r.segment_closest_time[b, k] in (0.0, times[b, k])


def test_nan_coefficients_and_nan_obstacles():
    coeffs, times, z = load_case("n10_k8_d3_fast")
    obs = z["s16/obstacles"]
    clean = m.check_obstacle_clearance_host(coeffs, times, obs)
    dirty = coeffs.copy()
    dirty[5, 3, 1, 4] = np.nan
    r = m.check_obstacle_clearance_host(dirty, times, obs)
    assert r.trajectory_feasible[5] == 0 and r.first_failing_segment[5] == min(3, clean.first_failing_segment[5] if clean.first_failing_segment[5] >= 0 else 3)
    assert np.isnan(r.segment_clearance[5, 3]) and np.isnan(r.trajectory_clearance[5]) and r.segment_nearest_obstacle[5, 3] == 0
    others = np.arange(len(coeffs)) != 5
    for x, y in zip(r, clean):
        assert np.array_equal(x[others], y[others])
    assert np.array_equal(np.delete(r.segment_clearance[5], 3), np.delete(clean.segment_clearance[5], 3))
    # a NaN obstacle fails every segment it is given to: first failing segment 0, and the smallest NaN index is reported
    bad = obs.copy()
    bad[11, 1], bad[13, 0] = np.nan, np.nan
    r = m.check_obstacle_clearance_host(coeffs, times, bad)
    assert not r.trajectory_feasible.any() and (r.first_failing_segment == 0).all() and np.isnan(r.segment_clearance).all()
    assert (r.segment_nearest_obstacle == 11).all() and np.isnan(r.trajectory_clearance).all()
    fails0 = ~(np.stack([m.check_obstacle_clearance_host(coeffs, times, obs[h:h + 1]).segment_clearance[:, 0] for h in range(11)], axis=1) > 0.0)
    assert np.array_equal(r.first_failing_obstacle, np.where(fails0.any(axis=1), fails0.argmax(axis=1), 11))


def test_outputs_are_written_in_full_and_not_beyond():
    lib = L.load()
    coeffs, times, z = load_case("n12_k4_d4")
    obs = np.ascontiguousarray(z["s16/obstacles"])
    bsz, k, d, n = coeffs.shape
    pad = 3
    i32 = lambda size: np.full((size + 2 * pad,), -77, dtype=np.int32)
    f64 = lambda size: np.full((size + 2 * pad,), -77.5)
    bufs = [i32(bsz), i32(bsz), i32(bsz), f64(bsz * k), i32(bsz * k), f64(bsz * k), f64(bsz)]
    ptr = lambda a: a.ctypes.data + pad * a.itemsize
    assert lib.mtg_check_obstacle_clearance_host(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, k, 1, obs.ctypes.data, 16, 0, 0.0,
                                                 *[ptr(a) for a in bufs]) == 0
    r = m.check_obstacle_clearance_host(coeffs, times, obs)
    for a, want in zip(bufs, r):
        assert (a[:pad] == a.dtype.type(-77 if a.dtype == np.int32 else -77.5)).all() and (a[-pad:] == a[:pad]).all()
        assert np.array_equal(a[pad:-pad], np.asarray(want).ravel())
    # every optional output may be absent
    feas = np.empty((bsz,), dtype=np.int32)
    assert lib.mtg_check_obstacle_clearance_host(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, k, 1, obs.ctypes.data, 16, 0, 0.0,
                                                 feas.ctypes.data, None, None, None, None, None, None) == 0
    assert np.array_equal(feas, r.trajectory_feasible)


def test_sphere_obstacles_helper():
    assert m.sphere_obstacles([[1, 2, 3], [4, 5, 6]], [0.5, 0.25]).tolist() == [[1, 2, 3, 0.5], [4, 5, 6, 0.25]]
    assert m.sphere_obstacles(np.zeros((3, 2, 3)), 1.0).shape == (3, 2, 4)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(m.MtgError):
            m.sphere_obstacles([[0, 0, 0]], bad)


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for name in ("mtg_check_obstacle_clearance", "mtg_check_obstacle_clearance_host"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]), name
    assert len(L.EXPORTS["mtg_check_obstacle_clearance"][1]) == 20 and len(L.EXPORTS["mtg_check_obstacle_clearance_host"][1]) == 19
