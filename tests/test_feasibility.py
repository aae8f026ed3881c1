"""Analytic input-feasibility check (FeasibilityAnalytic of mav_trajectory_generation_ros), CPU part: the library's host entry
mtg_check_input_feasibility_host -- the same lane code the device kernel runs (csrc/mtg_feasibility_lane.h) -- against the
reference's own verdicts (tests/golden/reference_feasibility_*.npz, written by tests/golden/make_reference_feasibility_golden.py)
and against hand-made polynomials whose answer follows from the rules of feasibility_analytic.cpp:42-233."""
import ctypes
import glob
import math
import os
import re

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_feasibility_*.npz")))
NAMES = m.InputConstraints.NAMES
G = 9.81
R = m.InputFeasibilityResult


def constraints_of(limits, min_section_time_s=0.05):
    c = m.InputConstraints(min_section_time_s=float(min_section_time_s))
    for name, value in zip(NAMES, limits):
        if np.isfinite(value):
            c.add_constraint(name, float(value))
    return c


def fixture_sets():
    for path in GOLDEN:
        z = np.load(path)
        for s in z["limit_sets"]:
            yield os.path.basename(path), str(s), z


def compare_with_fixture(z, s, traj, first, seg, bounds):
    """The assertions both entry points share: verdicts equal on every robust trajectory, bounds within 1e-9 relative wherever the
    implementation wrote a number, every quantity up to and including the failing check a number."""
    robust = z[f"{s}/robust"]
    bsz = robust.shape[0]
    n_bad = int((~robust).sum())
    assert n_bad <= 0.01 * bsz and n_bad <= max(1, bsz // 100), (s, n_bad)
    assert np.array_equal(seg[robust], z[f"{s}/segment_result"][robust])
    assert np.array_equal(traj[robust], z[f"{s}/trajectory_result"][robust])
    assert np.array_equal(first[robust], z[f"{s}/first_failing_segment"][robust])
    ref = z[f"{s}/segment_bounds"]
    assert not np.isfinite(bounds[~np.isfinite(ref)]).any()        # a quantity whose limit is absent is not computed
    wrote = np.isfinite(bounds)
    rel = np.abs(bounds[wrote] - ref[wrote]) / np.abs(ref[wrote])
    print(f"{s}: worst relative bound error {rel.max() if rel.size else 0.0:.2e} over {rel.size} numbers")
    assert (rel <= 1e-9).all()
    # thrust (0, 1) -> velocity (2) -> yaw rate (4) -> yaw acceleration (5) -> roll/pitch (3): everything up to the failing check
    upto = {0: (0, 1, 2, 4, 5, 3), 1: (0, 1, 2, 4, 5), 2: (0, 1), 3: (0, 1), 4: (0, 1, 2), 6: (0, 1, 2, 4), 7: (0, 1, 2, 4, 5)}
    ref_seg = z[f"{s}/segment_result"]
    for code, cols in upto.items():
        rows = (ref_seg == code) & robust[:, None]
        for q in cols:
            assert (np.isfinite(bounds[rows][:, q]) == np.isfinite(ref[rows][:, q])).all(), (code, q)


def test_fixture_set_conditions():
    """What the committed set has to hold: every code the analytic checker can return at least 5 times as a trajectory verdict
    and at least once with a failing segment that is not the first, never 5, one limit set with min_section_time_s = 0.01."""
    assert len(GOLDEN) >= 4
    seen, later, sections = {}, {}, set()
    for path in GOLDEN:
        assert os.path.getsize(path) <= 300 * 1000
    for _, s, z in fixture_sets():
        traj, first = z[f"{s}/trajectory_result"], z[f"{s}/first_failing_segment"]
        sections.add(float(z[f"{s}/min_section_time_s"]))
        for code in np.unique(traj):
            seen[int(code)] = seen.get(int(code), 0) + int((traj == code).sum())
            later[int(code)] = later.get(int(code), 0) + int(((traj == code) & (first > 0)).sum())
    for code in (0, 1, 2, 3, 4, 6, 7):
        assert seen.get(code, 0) >= 5, code
        if code:
            assert later.get(code, 0) >= 1, code
    assert 5 not in seen
    assert 0.01 in sections and 0.05 in sections


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[len("reference_feasibility_"):-4] for p in GOLDEN])
def test_host_entry_vs_reference(path):
    z = np.load(path)
    for s in z["limit_sets"]:
        c = constraints_of(z[f"{s}/limits"], z[f"{s}/min_section_time_s"])
        traj, first, seg, bounds = m.check_input_feasibility_host(z["coeffs"], z["times"], c)
        compare_with_fixture(z, s, traj, first, seg, bounds)
        # [K][B] times: same answer
        traj2, first2, seg2, bounds2 = m.check_input_feasibility_host(z["coeffs"], np.ascontiguousarray(z["times"].T), c, times_layout="soa")
        assert np.array_equal(traj, traj2) and np.array_equal(first, first2) and np.array_equal(seg, seg2)
        assert np.array_equal(bounds, bounds2, equal_nan=True)


def one_segment(n, dim, **polys):
    """[1][dim][n] coefficients from x=..., y=..., z=..., yaw=... lists of increasing powers."""
    c = np.zeros((1, dim, n))
    for d, name in enumerate(("x", "y", "z", "yaw")[:dim]):
        p = polys.get(name, [])
        c[0, d, :len(p)] = p
    return c


def check_one(c, t, **kw):
    min_section = kw.pop("min_section_time_s", 0.05)
    traj, first, seg, bounds = m.check_input_feasibility_host(c, np.array([t]), m.InputConstraints(min_section_time_s=min_section, **kw))
    assert seg[0] == traj and first == (-1 if traj == 0 else 0)
    return int(traj), bounds[0]


def test_section_end_points_are_not_evaluated():
    """z''' = 1 + 6 t, thrust = 4 + t + 3 t^2 on [0, 1]: both increase, so the candidates are 0 and T alone.  Whole segment:
    sqrt(j(1) / f(0)) = sqrt(7 / 4) > 1 -> split; [0, 0.5] holds the candidate 0 only: sqrt(1 / 4); [0.5, 1] holds T only:
    sqrt(7 / 8): feasible, although no section was examined at its own end points."""
    c = one_segment(6, 3, z=[0.0, 0.0, (4.0 - G) / 2.0, 1.0 / 6.0, 0.25])
    verdict, bounds = check_one(c, 1.0, omega_xy_max=1.0)
    assert verdict == R.kInputFeasible
    assert bounds[3] == pytest.approx(math.sqrt(7.0 / 4.0), rel=1e-12) and bounds[3] > 1.0
    assert bounds[0] == pytest.approx(4.0, rel=1e-12) and bounds[1] == pytest.approx(8.0, rel=1e-12)
    assert np.isnan(bounds[2]) and np.isnan(bounds[4]) and np.isnan(bounds[5])
    # a limit below the bound of the first half's only candidate: that half is split down to min_section_time_s
    verdict, _ = check_one(c, 1.0, omega_xy_max=0.4)
    assert verdict == R.kInputIndeterminable


def test_zero_thrust_forces_a_split():
    """Free fall, z = -g t^2 / 2: thrust is exactly 0 <= 1e-6, so the bound is DBL_MAX whatever the (zero) jerk: every section
    splits until it is shorter than min_section_time_s.  Without the protection sqrt(0 / 0) = NaN would pass as feasible."""
    c = one_segment(6, 3, z=[1.0, 0.0, -G / 2.0])
    verdict, bounds = check_one(c, 1.0, omega_xy_max=100.0)
    assert verdict == R.kInputIndeterminable
    assert bounds[0] == 0.0 and bounds[3] == np.finfo(np.float64).max


def test_short_segment_is_indeterminable():
    c = one_segment(6, 3, x=[0.0, 1.0])
    verdict, bounds = check_one(c, 0.04, omega_xy_max=1.0)
    assert verdict == R.kInputIndeterminable and np.isnan(bounds[3])
    assert check_one(c, 0.04, omega_xy_max=1.0, min_section_time_s=0.01)[0] == R.kInputFeasible
    assert check_one(c, 0.04, omega_xy_max=1.0, min_section_time_s=-0.01)[0] == R.kInputFeasible   # stored by magnitude


def test_thrust_low_is_reported_before_high():
    """thrust = 2 + 18 t on [0, 1]: below f_min = 5 and above f_max = 15."""
    c = one_segment(6, 3, z=[0.0, 0.0, (2.0 - G) / 2.0, 3.0])
    assert check_one(c, 1.0, f_min=5.0, f_max=15.0)[0] == R.kInputInfeasibleThrustLow
    assert check_one(c, 1.0, f_max=15.0)[0] == R.kInputInfeasibleThrustHigh
    assert check_one(c, 1.0, f_min=5.0)[0] == R.kInputInfeasibleThrustLow
    assert check_one(c, 1.0, f_min=1.99, f_max=20.01)[0] == R.kInputFeasible
    verdict, bounds = check_one(c, 1.0, f_min=1.0, f_max=25.0, v_max=1e-3)      # thrust passes, velocity is next
    assert verdict == R.kInputInfeasibleVelocity and bounds[0] == pytest.approx(2.0) and bounds[1] == pytest.approx(20.0)


def test_velocity_at_the_limit_passes():
    c = one_segment(10, 3, x=[1.0, 3.0])
    assert check_one(c, 2.0, v_max=3.0)[0] == R.kInputFeasible
    assert check_one(c, 2.0, v_max=math.nextafter(3.0, 0.0))[0] == R.kInputInfeasibleVelocity
    assert check_one(c, 2.0, v_max=-3.0)[0] == R.kInputFeasible                 # limits are stored by magnitude


def test_absent_limits_skip_their_checks():
    """x = 5 t fails only the default velocity limit: without v_max it is feasible and the velocity is not even computed."""
    c = one_segment(10, 3, x=[0.0, 5.0])
    full = m.InputConstraints.defaults()
    traj, _, _, bounds = m.check_input_feasibility_host(c, np.array([1.0]), full)
    assert traj == R.kInputInfeasibleVelocity and bounds[0, 2] == pytest.approx(5.0)
    full.remove_constraint("v_max")
    traj, _, _, bounds = m.check_input_feasibility_host(c, np.array([1.0]), full)
    assert traj == R.kInputFeasible and np.isnan(bounds[0, 2])
    assert bounds[0, 0] == pytest.approx(G) and bounds[0, 3] == 0.0
    traj, _, _, bounds = m.check_input_feasibility_host(c, np.array([1.0]), m.InputConstraints())
    assert traj == R.kInputFeasible and np.isnan(bounds).all()


def test_yaw_limits_need_four_dimensions():
    """yaw = t^2: rate 2 t (max 2 at T = 1), acceleration 2.  D = 3 has no yaw to check."""
    c4 = one_segment(8, 4, yaw=[0.0, 0.0, 1.0])
    assert check_one(c4, 1.0, omega_z_max=1.9)[0] == R.kInputInfeasibleYawRates
    assert check_one(c4, 1.0, omega_z_max=2.0, omega_z_dot_max=1.9)[0] == R.kInputInfeasibleYawAcc
    verdict, bounds = check_one(c4, 1.0, omega_z_max=2.0, omega_z_dot_max=2.0)
    assert verdict == R.kInputFeasible and bounds[4] == pytest.approx(2.0) and bounds[5] == pytest.approx(2.0)
    assert check_one(c4[:, :3], 1.0, omega_z_max=1e-3, omega_z_dot_max=1e-3)[0] == R.kInputFeasible
    # rate -3 + 2 t: the largest magnitude is the minimum's
    c4 = one_segment(8, 4, yaw=[0.0, -3.0, 1.0])
    assert check_one(c4, 1.0, omega_z_max=2.9)[0] == R.kInputInfeasibleYawRates


@pytest.mark.parametrize("dim", [1, 2, 5, 6])
def test_other_dimensions_are_indeterminable(dim):
    rng = np.random.default_rng(dim)
    c = rng.normal(size=(7, 3, dim, 10))
    traj, first, seg, bounds = m.check_input_feasibility_host(c, np.ones((7, 3)), m.InputConstraints.defaults())
    assert (seg == R.kInputIndeterminable).all() and (traj == R.kInputIndeterminable).all() and (first == 0).all()
    assert np.isnan(bounds).all()


def test_first_failing_segment_decides():
    """Segment 0 feasible, segment 1 too fast, segment 2 thrust too low: the trajectory reports segment 1's velocity."""
    c = np.concatenate([one_segment(10, 3, x=[0.0, 1.0]), one_segment(10, 3, x=[1.0, 5.0]), one_segment(10, 3, z=[0.0, 0.0, -4.0])])
    traj, first, seg, _ = m.check_input_feasibility_host(c, np.ones(3), m.InputConstraints.defaults())
    assert list(seg) == [R.kInputFeasible, R.kInputInfeasibleVelocity, R.kInputInfeasibleThrustLow]
    assert traj == R.kInputInfeasibleVelocity and first == 1


def rule_roll_pitch(c, t_seg, limit, min_section):
    """feasibility_analytic.cpp:177-233 restated with a plain recursion over numpy.roots candidates: (verdict, number of visited
    sections that held no candidate at all)."""
    n = c.shape[1]

    def der(p, k):
        return np.array([p[i] * math.prod(range(i - k + 1, i + 1)) for i in range(k, n)])

    def candidates(polys):
        g = np.zeros(1)
        for p in polys:
            dp = np.array([p[i] * i for i in range(1, len(p))])
            g = np.polynomial.polynomial.polyadd(g, np.polynomial.polynomial.polymul(p, dp))
        g = np.trim_zeros(g, "b")
        roots = np.roots(g[::-1]) if len(g) > 1 else np.array([])
        ts = [0.0, t_seg] + [r.real for r in roots if abs(r.imag) <= np.finfo(float).eps and 0.0 <= r.real <= t_seg]
        return [(t, math.sqrt(sum(np.polynomial.polynomial.polyval(t, p) ** 2 for p in polys))) for t in ts]

    thrust = [der(c[d], 2) + (G if d == 2 else 0.0) * np.eye(1, n - 2, 0)[0] for d in range(3)]
    fc, jc = candidates(thrust), candidates([der(c[d], 3) for d in range(3)])
    empty = [0]

    def visit(t1, t2):
        if t2 - t1 < min_section:
            return 1
        fs = [v for t, v in fc if t1 <= t <= t2]
        js = [v for t, v in jc if t1 <= t <= t2]
        if not fs and not js:
            empty[0] += 1
            return 0                      # sqrt(lowest / max) is NaN, and NaN > limit is false
        f_min, j_max = min(fs, default=np.finfo(float).max), max(js, default=-np.finfo(float).max)
        bound = (math.sqrt(j_max / f_min) if j_max >= 0 else float("nan")) if f_min > 1e-6 else np.finfo(float).max
        if bound > limit:
            half = (t1 + t2) / 2
            return visit(t1, half) or visit(half, t2)
        return 0

    return visit(0.0, t_seg), empty[0]


def test_section_without_candidates_is_feasible():
    """Sections that hold no candidate are visited on solved trajectories, and are feasible: the host entry agrees with a
    plain restatement of the recursion that counts them (robust rows of the omega_xy_max fixture, min_section_time_s = 0.01)."""
    path = os.path.join(ROOT, "tests", "golden", "reference_feasibility_n10_k8_d3_fast.npz")
    z = np.load(path)
    s = "roll_pitch_fine"
    limit, min_section = float(z[f"{s}/limits"][3]), float(z[f"{s}/min_section_time_s"])
    visited_empty = feasible_after_empty = 0
    for b in np.flatnonzero(z[f"{s}/robust"])[:25]:
        for k in range(z["coeffs"].shape[1]):
            want, n_empty = rule_roll_pitch(z["coeffs"][b, k], float(z["times"][b, k]), limit, min_section)
            assert want == z[f"{s}/segment_result"][b, k]
            got = m.check_input_feasibility_host(z["coeffs"][b, k][None], z["times"][b, k:k + 1], constraints_of(z[f"{s}/limits"], min_section))[0]
            assert got == want
            visited_empty += n_empty
            feasible_after_empty += int(n_empty > 0 and want == 0)
    assert visited_empty > 0 and feasible_after_empty > 0


def test_code_5_is_never_produced():
    for _, s, z in fixture_sets():
        c = constraints_of(z[f"{s}/limits"], z[f"{s}/min_section_time_s"])
        _, _, seg, _ = m.check_input_feasibility_host(z["coeffs"], z["times"], c)
        assert (seg != R.kInputInfeasibleRollPitchRates).all()
    rng = np.random.default_rng(2024)
    coeffs = rng.normal(size=(10000, 1, 4, 10)) * (0.5 ** np.arange(10))
    times = rng.uniform(0.2, 3.0, size=(10000, 1))
    traj, _, seg, _ = m.check_input_feasibility_host(coeffs, times, m.InputConstraints.defaults(min_section_time_s=0.01))
    assert (seg != R.kInputInfeasibleRollPitchRates).all() and (traj != R.kInputInfeasibleRollPitchRates).all()
    assert set(np.unique(traj)) <= {0, 1, 2, 3, 4, 6, 7} and len(np.unique(traj)) >= 3


def test_input_constraints_semantics():
    c = m.InputConstraints()
    assert not any(c.has_constraint(n) for n in NAMES) and c.min_section_time_s == 0.05 and c.gravity == 9.81
    c.set_default_values()
    want = dict(f_min=0.5 * G, f_max=1.5 * G, v_max=3.0, omega_xy_max=math.pi / 2, omega_z_max=math.pi / 2, omega_z_dot_max=2 * math.pi)
    assert {n: c.get_constraint(n) for n in NAMES} == want
    c = m.InputConstraints()
    c.add_constraint("v_max", -2.5)
    assert c.get_constraint("v_max") == 2.5                      # |value|
    c.add_constraint("f_max", 10.0)
    c.add_constraint("f_min", 12.0)                              # f_max rises to at least f_min
    assert c.get_constraint("f_max") == 12.0 and c.get_constraint("f_min") == 12.0
    c = m.InputConstraints()
    c.add_constraint("f_min", 8.0)
    c.add_constraint("f_max", 6.0)                               # the mirror case: f_min falls to at most f_max
    assert c.get_constraint("f_min") == 6.0 and c.get_constraint("f_max") == 6.0
    c.add_constraint("f_max", 9.0)
    assert c.get_constraint("f_min") == 6.0 and c.get_constraint("f_max") == 9.0
    assert c.remove_constraint("f_min") and not c.remove_constraint("f_min") and c.get_constraint("f_min") is None
    with pytest.raises(KeyError):
        c.add_constraint("omega", 1.0)
    raw = c.to_c()
    assert math.isnan(raw.f_min) and raw.f_max == 9.0 and raw.min_section_time_s == 0.05 and raw.gravity == 9.81
    # the C helpers carry the same defaults
    lib = L.load()
    cc = L.InputConstraintsC()
    lib.mtg_input_constraints_init(ctypes.byref(cc))
    assert all(math.isnan(getattr(cc, n)) for n in NAMES) and cc.min_section_time_s == 0.05 and cc.gravity == 9.81
    lib.mtg_input_constraints_set_defaults(ctypes.byref(cc))
    assert {n: getattr(cc, n) for n in NAMES} == want
    assert [m.get_input_feasibility_result_name(i) for i in (0, 1, 5)] == ["Feasible", "Indeterminable", "InfeasibleRollPitchRates"]
    assert [int(r) for r in R] == list(range(8)) and R.kInputInfeasibleYawAcc == 7
    assert m.InputConstraints(gravity=3.71).defaults(gravity=3.71).get_constraint("f_max") == 1.5 * 3.71


def test_gravity_is_a_field():
    """Hover (all coefficients zero): thrust = gravity."""
    c = np.zeros((1, 3, 10))
    _, _, _, bounds = m.check_input_feasibility_host(c, np.ones(1), m.InputConstraints(f_min=1.0, gravity=3.71))
    assert bounds[0, 0] == 3.71 and bounds[0, 1] == 3.71


def test_argument_errors():
    lib = L.load()
    co, ti = np.zeros((2, 3, 3, 10)), np.ones((2, 3))
    traj, first = np.zeros(2, np.int32), np.zeros(2, np.int32)
    c = m.InputConstraints.defaults().to_c()

    def host(n=10, k=3, d=3, b=2, coeffs=co.ctypes.data, times=ti.ctypes.data, sb=3, sk=1, cons=ctypes.byref(c), out=traj.ctypes.data):
        return lib.mtg_check_input_feasibility_host(n, k, d, b, coeffs, times, sb, sk, cons, out, first.ctypes.data, None, None)

    assert host() == 0
    assert host(n=5) == 0 and host(n=12) == 0                    # the accepted range of n_coeffs, include/mtg_hip.h
    for bad in (dict(n=4), dict(n=13), dict(n=0), dict(k=0), dict(d=0), dict(b=-1), dict(coeffs=None), dict(times=None),
                dict(cons=None), dict(out=None), dict(sb=0), dict(sk=0), dict(sb=-3), dict(sb=2, sk=1), dict(sb=1, sk=1)):
        assert host(**bad) == -1, bad
    assert host(sb=1, sk=2) == 0 and host(sb=7, sk=2) == 0       # [K][B], and padded [B][K]
    bad_c = m.InputConstraints.defaults().to_c()
    bad_c.min_section_time_s = float("nan")
    assert host(cons=ctypes.byref(bad_c)) == -1
    with pytest.raises(m.MtgError) as e:
        m.check_input_feasibility_host(np.zeros((1, 1, 3, 4)), np.ones((1, 1)), m.InputConstraints())
    assert e.value.code == -1 and "invalid argument" in str(e.value)
    # the device entry refuses the same before it looks at its context (none here: nothing can reach a device)
    assert lib.mtg_check_input_feasibility(None, 10, 3, 3, 2, co.ctypes.data, ti.ctypes.data, 3, 1, ctypes.byref(c), traj.ctypes.data,
                                           None, None, None) == -1


def test_new_kernels_use_no_scratch():
    """Over the build's resource remarks (MTG_BUILD_REMARKS=<dir> at build time), when the build was made with them."""
    remarks = os.environ.get("MTG_BUILD_REMARKS")
    log = os.path.join(remarks, "mtg_feasibility.log") if remarks else None
    if not log or not os.path.exists(log):
        pytest.skip("the build was not made with MTG_BUILD_REMARKS")
    text = open(log).read()
    names = re.findall(r"Function Name: (\S*feasibility\S*)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) >= 6 and len(scratch) >= len(names)
    assert max(scratch) == 0, list(zip(names, scratch))
