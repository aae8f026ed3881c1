"""Independent reference of the maxima-search stage of the time objective (csrc/mtg_objective_lane.h): the largest
||p^(der)(t)|| over [0, T] of one segment, and over a trajectory the largest of its segments -- plus the seeded inputs that
tests/test_objective_instances.py and tests/test_gpu_objective_instances.py share.  A plain module, pure numpy / Python.

Method, per segment ([D][N] float64 coefficients, T, der):
  1. s(t) = sum_dim (p_dim^(der)(t))^2 is formed EXACTLY: the doubles are scaled by one power of two to Python integers, the
     falling-factorial weights and the squares are integer arithmetic.
  2. Candidate times: 0, T, and for every numpy.roots(s') root with real part in [0, T] and |Im| <= 1e-3 T its real part as
     numpy gives it AND that value after three Newton steps on s' in np.longdouble (kept where it stays inside [0, T]).  The cut
     on the imaginary part is generous on purpose: a surplus candidate cannot hurt a maximum.
  3. The result is the largest sqrt(s) over the candidates, evaluated in np.longdouble from the derivative's own coefficients by
     power sums (not from s, whose coefficients cancel, and not by the library's Horner recurrence).  That route is pinned on
     mpmath at 60 digits for a handful of rows by tests/test_objective_instances.py.

Every candidate value is a value of the true function at a point of the interval, so up to its own rounding -- at most
(2 (N - der) + 2) 2^-64 ||p~(T)||, p~_dim = sum_i |a_i| T^i the sum of the term magnitudes -- the reference never exceeds the true
maximum.  How complete it is cannot be argued, only tested: the test module compares it with a 2001-point grid for every
(segment, order) it uses.

Nothing here uses csrc/mtg_extrema_lane.h, oracle/oracle_extrema.py or the reference project's Jenkins-Traub.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"

LD = np.longdouble
U64 = 2.0 ** -64      # unit roundoff of the 64-bit significand
IMAG_CUT = 1e-3       # |Im root| <= IMAG_CUT * T counts as real
GRID = 2001


def falling(i, der):
    v = 1
    for k in range(der):
        v *= i - k
    return v


def derivative_coefficients(c, der):
    """[D][N - der] longdouble: a_i = (i + der)! / i! c_(i + der), each product rounded once at 2^-64 (the weights are integers
    below 2^16).  For evaluation; the exact form of s' is exact_s_derivative."""
    c = np.asarray(c, dtype=np.float64)
    n = c.shape[-1]
    w = np.array([falling(i, der) for i in range(der, n)], dtype=LD)      # <= 11!/6! = 55440
    return c[..., der:].astype(LD) * w


def evaluate(a, t):
    """sqrt(sum_dim (sum_i a[dim][i] t^i)^2) in longdouble by power sums; a [D][n] longdouble, t [m] -> ([m] value,
    [m] ||p~(t)||, the magnitude the rounding of this evaluation is relative to)."""
    t = np.atleast_1d(np.asarray(t, dtype=LD))
    n = a.shape[1]
    pw = np.ones((len(t), n), dtype=LD)
    for e in range(1, n):
        pw[:, e] = pw[:, e - 1] * t
    terms = a[None, :, :] * pw[:, None, :]                # [m][D][n]
    r = terms.sum(axis=2)
    scale = np.abs(terms).sum(axis=2)
    return np.sqrt((r * r).sum(axis=1)), np.sqrt((scale * scale).sum(axis=1))


def exact_s_derivative(c, der):
    """Coefficients of s'(t), s = sum_dim (p_dim^(der))^2, as (list of Python integers, shift): s'_j = ints[j] * 2^-shift exactly."""
    c = np.asarray(c, dtype=np.float64)
    dim, n = c.shape
    nz = c[c != 0.0]
    if nz.size == 0:
        return [0], 0
    shift = 53 - int(np.frexp(nz)[1].min())               # every nonzero |c| * 2^shift is an integer
    ints = [[int(math.ldexp(float(c[d, i]), shift)) for i in range(n)] for d in range(dim)]
    for d in range(dim):
        for i in range(n):
            assert math.ldexp(float(ints[d][i]), -shift) == c[d, i]
    nq = n - der
    s = [0] * (2 * nq - 1)
    for d in range(dim):
        a = [falling(i + der, der) * ints[d][i + der] for i in range(nq)]
        for i in range(nq):
            for j in range(nq):
                s[i + j] += a[i] * a[j]
    return [j * s[j] for j in range(1, len(s))] or [0], 2 * shift


def _to_longdouble(v, shift):
    hi = float(v)                                          # correctly rounded
    lo = float(v - int(hi))
    return (LD(hi) + LD(lo)) * LD(2.0) ** (-shift)


def candidate_times(c, T, der):
    """0, T, the near-real roots of s' inside [0, T] as numpy.roots gives them, and their Newton-polished values."""
    ints, shift = exact_s_derivative(c, der)
    while len(ints) > 1 and ints[-1] == 0:
        ints.pop()
    cand = [0.0, float(T)]
    if len(ints) < 2:
        return np.array(cand, dtype=LD)
    top = max(abs(v) for v in ints)
    norm = top.bit_length()                                # scale into float64's range whatever the shift
    assert norm < 1000                                     # float(v) below cannot overflow
    f64 = np.array([float(v) / 2.0 ** norm for v in ints])
    roots = np.roots(f64[::-1])
    keep = roots[(roots.real >= 0.0) & (roots.real <= T) & (np.abs(roots.imag) <= IMAG_CUT * T)].real
    out = [LD(v) for v in cand] + [LD(v) for v in keep]
    if keep.size:
        ld = np.array([_to_longdouble(v, norm) for v in ints], dtype=LD)
        dld = ld[1:] * np.arange(1, len(ld), dtype=LD)
        x = keep.astype(LD)
        for _ in range(3):
            f = np.zeros_like(x)
            for v in ld[::-1]:
                f = f * x + v
            df = np.zeros_like(x)
            for v in dld[::-1]:
                df = df * x + v
            with np.errstate(divide="ignore", invalid="ignore"):
                step = np.where(df != 0, f / df, 0)
            x = x - step
        ok = np.isfinite(x) & (x >= 0) & (x <= LD(T))
        out += [v for v in x[ok]]
    return np.array(out, dtype=LD)


def segment_max(c, T, der):
    """(reference maximum as float64-convertible longdouble, ||p~(T)||: the magnitude evaluation errors are relative to)."""
    a = derivative_coefficients(c, der)
    val, _ = evaluate(a, candidate_times(c, T, der))
    _, scale = evaluate(a, np.array([T]))
    return val.max(), scale[0]


def segment_grid_max(c, T, der, points=GRID):
    a = derivative_coefficients(c, der)
    val, _ = evaluate(a, np.linspace(LD(0), LD(T), points, dtype=LD))
    return val.max()


def batch_max(coeffs, times, der):
    """coeffs [B][K][D][N], times [B][K] -> (ref [B][K] longdouble, scale [B][K] longdouble) per segment."""
    bsz, k = times.shape
    ref = np.zeros((bsz, k), dtype=LD)
    scale = np.zeros((bsz, k), dtype=LD)
    for b in range(bsz):
        for s in range(k):
            ref[b, s], scale[b, s] = segment_max(coeffs[b, s], times[b, s], der)
    return ref, scale


# ---- the shared inputs ---------------------------------------------------------------------------------------------------
B, K = 13, 5          # 65 lanes: one full 64-lane workgroup and one lane; the last trajectory's atomics come from two workgroups
SHAPES = [(n, d) for d in (3, 4) for n in range(4, 13)] + [(10, 1), (10, 2), (7, 1), (7, 2)]
FAMILIES = ("taylor", "wavy", "allreal")
CASES = [(n, d, f) for f in FAMILIES[:2] for n, d in SHAPES] + [(n, d, "allreal") for d in (1, 4) for n in range(4, 11)]
WEIGHT, MAX_COST = 100.0, 1.0e12      # NonlinearOptimizationParameters' defaults


def seed_of(n, d, family="taylor"):
    return 20260000 + 100 * n + d + 50 * FAMILIES.index(family)      # fixed before any result of the code under test was looked at


def make_inputs(n, d, family="taylor"):
    """(coeffs [B][K][D][N], times [B][K]), segment times uniform in [0.5, 3], coefficient i on the order of 1 / i! (derivatives of
    comparable size across the orders):
      'taylor'  coefficient i = normal / i!.  Nearly all of its maxima lie at a segment END (the top terms grow monotonically), so
                on its own it says little about the interior search;
      'wavy'    the Taylor coefficients of A sin(w t + phase_dim), A in [0.5, 2], w in [0.8, 2], the phases of a segment's
                dimensions within ~0.3 of each other: every derivative oscillates and many maxima are INTERIOR critical points;
      'allreal' every dimension a multiple of ONE polynomial whose velocity has all its N - 2 roots inside (0, T), near the
                Chebyshev nodes (each moved by up to 2 % of T / N): every derivative then has all its roots real and inside the
                segment, and so has the searched polynomial p^(der) p^(der + 1) -- the largest root count a search can meet,
                which fills both root buffers to their last element (derivative 1: 2 N - 5 roots).  N <= 10 only: a
                polynomial with all its roots in (0, T) is the power basis' worst case, and from N = 11 on float64 cannot even
                EVALUATE the magnitude to the 1e-9 the search is held to (tests/test_objective_instances.py asserts that this,
                not the library's result, draws the line)."""
    rng = np.random.default_rng(seed_of(n, d, family))
    fact = np.array([math.factorial(i) for i in range(n)], dtype=np.float64)
    times = rng.uniform(0.5, 3.0, size=(B, K))
    if family == "taylor":
        coeffs = rng.standard_normal((B, K, d, n)) / fact
    elif family == "allreal":
        coeffs = np.zeros((B, K, d, n))
        deg = n - 2
        for b in range(B):
            for k in range(K):
                nodes = 0.5 * times[b, k] * (1.0 + np.cos((2.0 * np.arange(1, deg + 1) - 1.0) * math.pi / (2.0 * deg)))
                nodes = nodes + 0.02 * times[b, k] / n * rng.uniform(-1.0, 1.0, size=deg)
                vel = np.poly(nodes)[::-1]                                   # increasing powers, monic
                vel = vel / np.abs(np.polyval(vel[::-1], 0.0))               # velocity of size 1 at t = 0
                pos = np.concatenate([[rng.standard_normal()], vel / np.arange(1, n)])
                coeffs[b, k] = rng.uniform(0.5, 2.0, size=(d, 1)) * rng.choice([-1.0, 1.0], size=(d, 1)) * pos
    else:
        amp = rng.uniform(0.5, 2.0, size=(B, K, d, 1))
        w = rng.uniform(0.8, 2.0, size=(B, K, 1, 1))
        phase = rng.uniform(0.0, 2.0 * math.pi, size=(B, K, 1, 1)) + 0.3 * rng.standard_normal((B, K, d, 1))
        i = np.arange(n, dtype=np.float64)
        coeffs = amp * w ** i * np.sin(phase + i * (math.pi / 2.0)) / fact
    return np.ascontiguousarray(coeffs), np.ascontiguousarray(times)


def orders_of(n):
    return list(range(1, n // 2))      # 1 .. N/2 - 1


def order_groups(n):
    o = orders_of(n)
    return [o[i:i + 4] for i in range(0, len(o), 4)]      # MTG_MAX_MAGNITUDE_CONSTRAINTS = 4


_cache = {}


def reference(n, d, family="taylor"):
    """{'coeffs', 'times', 'orders', 'ref' [B][K][orders] longdouble per segment, 'scale' likewise (||p~(T)||), 'ends' likewise (the
    larger of the two end values), 'traj' [B][orders] = max over segments, 'limits' [orders]}.  Computed once per case and
    shared; the arrays are read-only."""
    key = (n, d, family)
    if key not in _cache:
        coeffs, times = make_inputs(n, d, family)
        orders = orders_of(n)
        ref = np.zeros((B, K, len(orders)), dtype=LD)
        scale = np.zeros((B, K, len(orders)), dtype=LD)
        ends = np.zeros((B, K, len(orders)), dtype=LD)
        for q, der in enumerate(orders):
            ref[:, :, q], scale[:, :, q] = batch_max(coeffs, times, der)
            for b in range(B):
                for k in range(K):
                    ends[b, k, q] = evaluate(derivative_coefficients(coeffs[b, k], der), np.array([0.0, times[b, k]]))[0].max()
        traj = ref.max(axis=1)
        # limit of an order: 0.98 x the median of the REFERENCE's trajectory maxima.  The median trajectory's term is then
        # exp(100 * 0.0204) = 7.7, above one and uncapped, the lower half's terms are below one, and with the default weight a
        # term is capped from 1.276 x the limit on
        limits = np.array([0.98 * float(np.sort(traj[:, q].astype(np.float64))[B // 2]) for q in range(len(orders))])
        for a in (coeffs, times, ref, scale, ends, traj, limits):
            a.setflags(write=False)
        _cache[key] = dict(coeffs=coeffs, times=times, orders=orders, ref=ref, scale=scale, ends=ends, traj=traj, limits=limits)
    return _cache[key]


def per_segment(z):
    """The same inputs with every segment a trajectory of its own ([B K][1][D][N], [B K][1]): the library's per-trajectory maximum is
    then the SEGMENT's, which a trajectory's maximum over five segments mostly hides."""
    b, k, d, n = z["coeffs"].shape
    return np.ascontiguousarray(z["coeffs"].reshape(b * k, 1, d, n)), np.ascontiguousarray(z["times"].reshape(b * k, 1))


U = 2.0 ** -53


def upper_bound_segments(z, n, d):
    """[B][K][orders] longdouble: what the library's maximum of a segment may not exceed (derivation:
    tests/test_objective_instances.py)."""
    out = np.zeros(z["ref"].shape, dtype=LD)
    for q, der in enumerate(z["orders"]):
        out[:, :, q] = z["ref"][:, :, q] + LD(U) * ((n - der + 2) * z["scale"][:, :, q] + (max(d, 3) + 2) * z["ref"][:, :, q])
    return out
