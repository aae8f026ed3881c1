"""Every instantiation of the time objective's maxima search on the CPU: mtg_magnitude_soft_cost_host (the lane code of
csrc/mtg_objective_lane.h, which the device kernels run too) against the independent reference of tests/objective_ref.py, for
N = 4 .. 12 at D = 3 and 4, D = 1 and 2 at N = 10 and 7, every accepted derivative order 1 .. N/2 - 1; the zero-padded paths,
the forms of the constraint list and non-finite coefficients.  Inputs: objective_ref.make_inputs (seeded, 13 x 5 segments, three
families: random Taylor-like, sinusoid Taylor coefficients with interior maxima, all roots inside the segment).

The two bounds on a maximum, per trajectory and constraint (ref = the reference's value, <= the true maximum M):

  lower   got >= ref (1 - 1e-9): HOST_DELTA of tests/time_objective_checks.py, the bound csrc/mtg_extrema_lane.h claims for the
          effects of its partition tolerance.  For every order.

  upper   got <= max over the segments of  ref_k + u ((N - der + 2) ||p~_k(T_k)|| + (DC + 2) ref_k),   u = 2^-53.
          Derivation.  The library's maximum of a segment is its evaluation of ||p^(der)(t)|| at some float64 t of [0, T]
          (0, T, or fl(root T) with root in [0, 1]).  Per dimension the value r of a_i = fl(base(der, i) c_i) t^i is formed by a
          Horner chain of N - der fused steps: term i passes one rounding of its coefficient product and at most N - der
          roundings of the chain, so |r^ - r| <= (N - der + 1) u p~(t) to first order, p~(t) = sum_i |a_i| t^i <= p~(T).  The
          DC squares are accumulated by DC fused steps and the square root rounds once: relative (DC / 2 + 1) u on the norm.
          With the triangle inequality over the dimensions, got <= (M_k(t) + (N - der + 1) u ||p~(T)||) (1 + (DC / 2 + 1) u).
          The bound above rounds both counts up (one more unit of u ||p~|| and DC / 2 + 1 more units of u ref): that room holds
          the second-order terms and the reference's own rounding, (2 (N - der) + 2) 2^-64 ||p~(T)|| = at most 0.012 u ||p~||,
          and the part of M - ref that the completeness check below cannot see is not in it: a reference that misses a maximum
          shows as a violation here and is then looked at.  Nothing in it was tuned on what the library returns.

The reference's completeness is checked here, on every (segment, order) the tests use: the largest of 2001 grid values in
longdouble may exceed the reference by no more than the grid evaluation's rounding, (2 (N - der) + 2) 2^-64 ||p~(T)||.

Measured on the host form (this module prints the figures per case and per N; the device's are printed by
tests/test_gpu_objective_instances.py): worst shortfall (ref - got) / ref 2.9e-11 and worst excess (got - ref) / ref 3.2e-11, both
in the 'allreal' family at N = 10 (derived evaluation bound there 8e-10); 1.4e-15 and 1.5e-15 over the other two families.
DESIGN.md section 4.9 records them.
"""
import math

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
import objective_ref as R
from time_objective_checks import HOST_DELTA

EPS = np.finfo(np.float64).eps
LD = np.longdouble
CASE_IDS = [f"{f}_n{n}_d{d}" for n, d, f in R.CASES]
NONFINITE_SHAPES = [(4, 3), (7, 3), (10, 4), (12, 3), (10, 2)]


def params(cons, **kw):
    kw.setdefault("soft_constraint_weight", R.WEIGHT)
    kw.setdefault("maximum_cost", R.MAX_COST)
    return m.TimeObjectiveParams(constraints=cons, **kw)


def run_groups(fn, n, coeffs, times, limits):
    """fn(coeffs, times, params) -> (cost, maxima, violations) once per group of at most four orders; the columns joined
    in order: (list of per-group costs, maxima [B][orders], violations [B][orders])."""
    costs, mx, vio = [], [], []
    for group in R.order_groups(n):
        c, a, v = fn(coeffs, times, params([(der, float(limits[der - 1])) for der in group]))
        costs.append(c)
        mx.append(a)
        vio.append(v)
    return costs, np.concatenate(mx, axis=1), np.concatenate(vio, axis=1)


def expected_terms(maxima, limits, weight=R.WEIGHT, cap=R.MAX_COST):
    """fmin(cap, exp((max - limit) / limit * weight)) in the order of operations of mtgo::soft_term."""
    with np.errstate(over="ignore"):
        return np.minimum(cap, np.exp((maxima - limits) / limits * weight))


def check_bounds(got, z, n, d, label, segments=False):
    """The two bounds of the module docstring on maxima [B][orders] of the trajectories, or [B K][orders] of every segment as a
    trajectory of its own (R.per_segment); returns (worst shortfall, worst excess), relative."""
    upper = R.upper_bound_segments(z, n, d)
    if segments:
        ref, upper = z["ref"].reshape(R.B * R.K, -1), upper.reshape(R.B * R.K, -1)
    else:
        ref, upper = z["traj"], upper.max(axis=1)
    g = got.astype(LD)
    short = float(((ref - g) / ref).max())
    excess = float(((g - ref) / ref).max())
    print(f"{label}: worst shortfall (ref - got) / ref {short:.3e} (allowed {HOST_DELTA:.0e}), worst excess (got - ref) / ref "
          f"{excess:.3e} (allowed, tightest / widest {float(((upper - ref) / ref).min()):.3e} / {float(((upper - ref) / ref).max()):.3e})")
    assert np.isfinite(got).all()
    assert (g >= ref * (1 - LD(HOST_DELTA))).all(), (label, "below the reference", short)
    assert (g <= upper).all(), (label, "above the evaluation bound", excess)
    return short, excess


def check_terms(term, maximum, limit, label=""):
    """One soft term per trajectory against the formula on the RETURNED maximum: the exponent is three correctly rounded
    operations on both sides, so only exp's last bits may differ (4 ulps allowed: two libraries of < 1 ulp each, twice over)."""
    want = expected_terms(maximum, limit)
    assert (np.abs(term - want) <= 4 * EPS * want).all(), (label, np.abs(term / want - 1).max())
    assert (term[want >= R.MAX_COST] == R.MAX_COST).all()


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_reference_evaluation_pinned_on_mpmath():
    """The longdouble route of objective_ref.evaluate on mpmath at 60 digits, at the reference's own candidate times."""
    import mpmath
    mpmath.mp.dps = 60
    worst = 0.0
    for n, d, family, rows in ((4, 3, "taylor", (0, 7)), (7, 2, "wavy", (3,)), (10, 4, "taylor", (12,)), (12, 3, "wavy", (5, 9))):
        coeffs, times = R.make_inputs(n, d, family)
        for b in rows:
            for der in R.orders_of(n):
                c, T = coeffs[b, b % R.K], times[b, b % R.K]
                a = R.derivative_coefficients(c, der)
                t = R.candidate_times(c, T, der)
                val, scale = R.evaluate(a, t)
                for j in range(len(t)):
                    tj = mpmath.mpf(float(t[j])) + mpmath.mpf(float(t[j] - LD(float(t[j]))))
                    acc = mpmath.mpf(0)
                    for dim in range(d):
                        r = mpmath.mpf(0)
                        for i in range(n - 1, der - 1, -1):
                            r = r * tj + mpmath.mpf(R.falling(i, der)) * mpmath.mpf(float(c[dim, i]))
                        acc += r * r
                    want = mpmath.sqrt(acc)
                    got = mpmath.mpf(float(val[j])) + mpmath.mpf(float(val[j] - LD(float(val[j]))))
                    err = float(abs(got - want))
                    bound = (2 * (n - der) + 2) * R.U64 * float(scale[j])
                    worst = max(worst, err / bound)
                    assert err <= bound, (n, d, b, der, j, err, bound)
    print(f"longdouble evaluation vs mpmath: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n,d,family", R.CASES, ids=CASE_IDS)
def test_reference_completeness(n, d, family):
    """No grid value above the reference, for every (segment, order) of this case -- the zero-padding, constraint-list and
    non-finite tests use segments of these cases only."""
    z = R.reference(n, d, family)
    worst = -np.inf
    for q, der in enumerate(z["orders"]):
        for b in range(R.B):
            for k in range(R.K):
                grid = R.segment_grid_max(z["coeffs"][b, k], z["times"][b, k], der)
                room = (2 * (n - der) + 2) * R.U64 * z["scale"][b, k, q]
                worst = max(worst, float((grid - z["ref"][b, k, q]) / z["ref"][b, k, q]))
                assert grid <= z["ref"][b, k, q] + room, (n, d, der, b, k, float(grid), float(z["ref"][b, k, q]))
    print(f"{family} n = {n} d = {d}: largest (grid maximum - reference) / reference {worst:.3e}")


def test_limits_span_the_classes():
    """The limits (0.98 x the medians of the reference's maxima) leave soft terms below one, above one and at the cap in every case."""
    for n, d, family in R.CASES:
        z = R.reference(n, d, family)
        t = expected_terms(z["traj"].astype(np.float64), z["limits"])
        assert (t < 1.0).any() and ((t > 1.0) & (t < R.MAX_COST)).any(), (n, d, family)
        assert (t == R.MAX_COST).any() or family == "allreal", (n, d, family)      # (its maxima lie within a few percent)


def test_allreal_family_is_evaluable():
    """Where the 'allreal' family stops: the derived evaluation bound u (N - der + 2) ||p~(T)|| / ref -- what float64 can hold
    the VALUE of the magnitude to, whatever finds its place -- stays below the 1e-9 of the lower bound for every case used, and
    exceeds it from N = 11 on.  (There the host form was seen to fall short by 4e-6 at N = 11 and 4e-3 at N = 12: the searched
    polynomial's coefficients cancel by fourteen digits.  DESIGN.md section 4.9.)"""
    def widest(n, d):
        z = R.reference(n, d, "allreal")
        return float(((R.upper_bound_segments(z, n, d) - z["ref"]) / z["ref"]).max())
    for n, d, family in R.CASES:
        if family == "allreal":
            assert widest(n, d) < HOST_DELTA, (n, d)
    assert widest(11, 1) > HOST_DELTA and widest(12, 1) > HOST_DELTA


def test_inputs_have_interior_maxima():
    """Every search the lane code instantiates, (NC, DC, order), meets segments whose maximum is an interior critical point that
    exceeds both end values by more than 1e-6 relative: a search that found no roots would miss the lower bound there."""
    count = {}
    for n, d, family in R.CASES:
        z = R.reference(n, d, family)
        interior = z["ref"] > z["ends"] * (1 + LD(1e-6))
        for q, der in enumerate(z["orders"]):
            key = ((n + 1) & ~1, max(d, 3), der)
            count[key] = count.get(key, 0) + int(interior[:, :, q].sum())
    assert set(count) == {(nc, dc, der) for nc in (4, 6, 8, 10, 12) for dc in (3, 4) for der in range(1, nc // 2)}
    print("segments with an interior maximum per (NC, DC, order):", sorted(count.items()))
    assert min(count.values()) >= 5


# ---- the host form on the whole matrix -------------------------------------------------------------------------------------
WORST = {}


def check_segments(fn, z, n, d, maxima, label):
    """Every segment as a trajectory of its own: the two bounds per SEGMENT, and a trajectory's maximum is bit for bit the
    largest of its segments'."""
    _, seg_max, _ = run_groups(fn, n, *R.per_segment(z), z["limits"])
    short, excess = check_bounds(seg_max, z, n, d, label + " per segment", segments=True)
    assert np.array_equal(seg_max.reshape(R.B, R.K, -1).max(axis=1), maxima)
    return short, excess


@pytest.mark.parametrize("n,d,family", R.CASES, ids=CASE_IDS)
def test_host_matrix(n, d, family):
    z = R.reference(n, d, family)
    costs, maxima, violations = run_groups(m.magnitude_soft_cost_host, n, z["coeffs"], z["times"], z["limits"])
    short, excess = check_bounds(maxima, z, n, d, f"host {family} n = {n} d = {d}")
    s2, e2 = check_segments(m.magnitude_soft_cost_host, z, n, d, maxima, f"host {family} n = {n} d = {d}")
    short, excess = max(short, s2), max(excess, e2)
    w = WORST.setdefault(n, [-np.inf, -np.inf])
    w[0], w[1] = max(w[0], short), max(w[1], excess)
    print(f"host, N = {n} so far: worst shortfall {w[0]:.3e}, worst excess {w[1]:.3e}")
    assert np.array_equal(violations, maxima - z["limits"])                       # bit for bit
    terms = np.zeros_like(maxima)
    for q, der in enumerate(z["orders"]):
        c1, m1, v1 = m.magnitude_soft_cost_host(z["coeffs"], z["times"], params([(der, float(z["limits"][q]))]))
        assert np.array_equal(m1[:, 0], maxima[:, q]) and np.array_equal(v1[:, 0], violations[:, q])
        check_terms(c1, maxima[:, q], z["limits"][q], f"n = {n} d = {d} order {der}")
        terms[:, q] = c1
    # the cost of a group: its terms summed in constraint order, from 0
    for group, cost in zip(R.order_groups(n), costs):
        want = np.zeros(R.B)
        for der in group:
            want = want + terms[:, der - 1]
        assert np.array_equal(cost, want)
    # [K][B] times: the same answer
    for group, cost in zip(R.order_groups(n), costs):
        p = params([(der, float(z["limits"][der - 1])) for der in group])
        c2, m2, _ = m.magnitude_soft_cost_host(z["coeffs"], np.ascontiguousarray(z["times"].T), p, times_layout="soa")
        assert np.array_equal(c2, cost) and np.array_equal(m2, maxima[:, group[0] - 1:group[-1]])


# ---- zero padding ----------------------------------------------------------------------------------------------------------
def padded_n(coeffs):
    return np.ascontiguousarray(np.concatenate([coeffs, np.zeros(coeffs.shape[:-1] + (1,))], axis=-1))


def padded_d(coeffs, to=3):
    b, k, d, n = coeffs.shape
    return np.ascontiguousarray(np.concatenate([coeffs, np.zeros((b, k, to - d, n))], axis=2))


def check_padding(fn, n, d, family, equal):
    z = R.reference(n, d, family)
    _, maxima, violations = run_groups(fn, n, z["coeffs"], z["times"], z["limits"])
    if n % 2:
        # the odd N's orders only: N + 1 accepts one more, which the odd N cannot be asked for
        _, mp, vp = run_groups(fn, n, padded_n(z["coeffs"]), z["times"], z["limits"])
        assert equal(mp, maxima) and equal(vp, violations), (n, d, "explicit zero top coefficient")
    if d < 3:
        _, mp, vp = run_groups(fn, n, padded_d(z["coeffs"]), z["times"], z["limits"])
        assert equal(mp, maxima) and equal(vp, violations), (n, d, "explicit zero dimensions")


PADDING_CASES = [(n, d, f) for n, d, f in R.CASES if n % 2 or d < 3]
PADDING_IDS = [f"{f}_n{n}_d{d}" for n, d, f in PADDING_CASES]


@pytest.mark.parametrize("n,d,family", PADDING_CASES, ids=PADDING_IDS)
def test_zero_padding(n, d, family):
    """An odd N equals N + 1 with an explicit zero top coefficient, D < 3 equals D = 3 with explicit zero dimensions: bit for bit."""
    check_padding(m.magnitude_soft_cost_host, n, d, family, np.array_equal)


# ---- forms of the constraint list ------------------------------------------------------------------------------------------
def check_constraint_list(fn, n, d, to_host=lambda a: a):
    z = R.reference(n, d, "wavy")
    lim = z["limits"]
    cons = [(3, float(lim[2])), (1, float(lim[0])), (2, float(lim[1])), (1, float(lim[0]) * 1.5)]
    cost, maxima, violations = (to_host(a) for a in fn(z["coeffs"], z["times"], params(cons)))
    singles = []
    for q, (der, value) in enumerate(cons):
        c1, m1, v1 = (to_host(a) for a in fn(z["coeffs"], z["times"], params([(der, value)])))
        assert np.array_equal(m1[:, 0], maxima[:, q]) and np.array_equal(v1[:, 0], violations[:, q]), (n, d, q)
        singles.append(c1)
    assert np.array_equal(maxima[:, 1], maxima[:, 3])
    assert np.array_equal(cost, ((singles[0] + singles[1]) + singles[2]) + singles[3])
    # soft constraints off: maxima still written, cost 0
    c0, m0, v0 = (to_host(a) for a in fn(z["coeffs"], z["times"], params(cons, use_soft_constraints=False)))
    assert (c0 == 0.0).all() and np.array_equal(m0, maxima) and np.array_equal(v0, violations)
    # no constraints: cost 0 and no maxima
    c0, m0, v0 = (to_host(a) for a in fn(z["coeffs"], z["times"], params([])))
    assert (c0 == 0.0).all() and c0.shape == (R.B,) and m0.shape == (R.B, 0) and v0.shape == (R.B, 0)


@pytest.mark.parametrize("n,d", [(8, 3), (9, 4), (12, 4)])
def test_constraint_list_forms(n, d):
    check_constraint_list(m.magnitude_soft_cost_host, n, d)


def check_order_acceptance(fn):
    for n in range(4, 13):
        coeffs, times = R.make_inputs(n, 3)
        with pytest.raises(m.MtgError) as e:
            fn(coeffs, times, params([(n // 2, 1.0)]))
        assert e.value.code == -1
        fn(coeffs, times, params([(n // 2 - 1, 1.0)]))
    c12, t12 = R.make_inputs(12, 3)
    c10, t10 = R.make_inputs(10, 3)
    fn(c12, t12, params([(5, 1.0)]))
    with pytest.raises(m.MtgError):
        fn(c10, t10, params([(5, 1.0)]))


def test_order_acceptance():
    """Order N/2 is rejected for every N; 5 is accepted at N = 12 and rejected at N = 10."""
    check_order_acceptance(m.magnitude_soft_cost_host)


# ---- non-finite coefficients -----------------------------------------------------------------------------------------------
ALL_NAN, ONE_INF, UNUSED_NAN = 3, 11, 6      # trajectories; 11 is the left neighbour of the one that straddles two workgroups


def poisoned(coeffs):
    bad = coeffs.copy()
    bad[ALL_NAN] = np.nan
    bad[ONE_INF, 2, bad.shape[2] - 1, -1] = np.inf     # the highest coefficient of the last dimension, a middle segment
    bad[UNUSED_NAN, 1, 0, 0] = np.nan                  # index 0: no derivative >= 1 reads it
    return bad


def check_non_finite(fn, n, d, to_host=lambda a: a):
    """The contract of include/mtg_hip.h: a non-finite coefficient that a constrained derivative uses makes that trajectory's
    maximum and violation NaN and its soft term maximum_cost; nothing else changes by a bit."""
    z = R.reference(n, d, "wavy")
    good = np.ones(R.B, dtype=bool)
    good[[ALL_NAN, ONE_INF]] = False
    out = {}
    for group in R.order_groups(n):
        cons = [(der, float(z["limits"][der - 1])) for der in group]
        clean = [to_host(a) for a in fn(z["coeffs"], z["times"], params(cons))]
        got = [to_host(a) for a in fn(poisoned(z["coeffs"]), z["times"], params(cons))]
        for name, c, g in zip(("cost", "maxima", "violations"), clean, got):
            assert np.array_equal(g[good], c[good]), (n, d, group, name, "a finite trajectory changed")
        assert np.isfinite(clean[1]).all()
        assert np.isnan(got[1][~good]).all(), (n, d, group, "maxima", got[1][~good])
        assert np.isnan(got[2][~good]).all(), (n, d, group, "violations", got[2][~good])
        assert (got[0][~good] == len(group) * R.MAX_COST).all(), (n, d, group, "cost", got[0][~good])
        for der, value in cons:      # each soft term on its own: exactly maximum_cost
            c1, m1, _ = (to_host(a) for a in fn(poisoned(z["coeffs"]), z["times"], params([(der, value)])))
            assert (c1[~good] == R.MAX_COST).all() and np.isnan(m1[~good]).all(), (n, d, der)
        out[tuple(group)] = got
    return out


@pytest.mark.parametrize("n,d", NONFINITE_SHAPES)
def test_non_finite_host(n, d):
    check_non_finite(m.magnitude_soft_cost_host, n, d)
